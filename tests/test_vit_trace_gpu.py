"""Every stage of the ``FusedViT`` graphs on the device against float64, at every element of every token: the recorder of
``_vit_trace_ref`` wraps the real wrappers, and ``TraceChecker`` builds each stage's reference from the bits that entered that stage on
the device and the torch module's own float32 state dict, with the gate of that kernel's own test.  What the graph-level tests cannot
see -- the last block's work on every row but the class row, anything under the FP8 yardstick's own error -- is a stage here.
``tests/test_vit_trace.py`` shows on torch stand-ins that the checker passes a faithful graph and names each of a list of faults.

Each case prints one line per stage, the worst error as a multiple of its gate (``profiles/vit_trace_gpu.txt`` holds a run)."""

from __future__ import annotations

import pytest
import torch

from _vit_trace_ref import CASE_IDS, CASES, TraceChecker, form_input, fused_graph, plan_of, record, run_graph, table_lines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize(("form", "dtype"), CASES, ids=CASE_IDS)
def test_every_stage_matches_float64(form, dtype, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    vit = form.build()
    x, table32 = form_input(form)
    fused = fused_graph(vit, dtype, fp8=form.fp8, device="cuda")
    trace = record(monkeypatch, vit_fused)
    got = run_graph(fused, x, table32, dtype, "cuda")
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), trace[-1].out)  # what the graph returns is the last stage's result
    checker = TraceChecker(vit, trace, x, dtype, fp8=form.fp8, table32=table32)
    try:
        rows = checker.check()
    finally:
        print("\n".join(table_lines(f"{form.ident} {'fp16' if dtype == torch.float16 else 'bf16'}", checker.rows)))
    assert [place for place, _, _ in rows] == [place for place, _ in plan_of(vit, uint8=table32 is not None, fp8=form.fp8).stages]
    assert all(ratio <= 1.0 for _, _, ratio in rows)
