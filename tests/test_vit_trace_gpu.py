"""Every stage of the ``FusedViT`` graphs on the device against float64, at every element of every token: the recorder of
``_vit_trace_ref`` wraps the real wrappers, and ``TraceChecker`` builds each stage's reference from the bits that entered that stage on
the device and the torch module's own float32 state dict, with the gate of that kernel's own test.  What the graph-level tests cannot
see -- the last block's work on every row but the class row, anything under the FP8 or INT8 yardstick's own error, which GEMM a layer of
the float32 route ran on, what the in-place pass left in the float32 stream -- is a stage here.  The cases cover the half graph, the
FP8 and INT8 routes, ``residual_dtype="float32"`` and the float32 route (``linear_dtype="bfloat16x3"``).
``tests/test_vit_trace.py`` shows on torch stand-ins that the checker passes a faithful graph and names each of a list of faults.

Each case prints one line per stage, the worst error as a multiple of its gate (``profiles/vit_trace_gpu.txt`` holds a run of the half
and FP8 cases, ``profiles/vit_trace_routes_gpu.txt`` one of the three later routes)."""

from __future__ import annotations

import pytest
import torch

from _vit_trace_ref import CASE_IDS, CASES, DTYPE_IDS, TraceChecker, form_input, fused_graph, plan_of, record, run_graph, table_lines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize(("form", "dtype"), CASES, ids=CASE_IDS)
def test_every_stage_matches_float64(form, dtype, monkeypatch):
    from tiatoolbox_amd.models.architecture import vit_fused

    vit = form.build()
    x, table32 = form_input(form)
    fused = fused_graph(vit, dtype, fp8=form.fp8, route=form.route, device="cuda")
    trace = record(monkeypatch, vit_fused)
    got = run_graph(fused, x, table32, dtype, "cuda")
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), trace[-1].out)  # what the graph returns is the last stage's result
    checker = TraceChecker(vit, trace, x, dtype, fp8=form.fp8, route=form.route, table32=table32)
    try:
        rows = checker.check()
    finally:
        print("\n".join(table_lines(f"{form.ident} {DTYPE_IDS[dtype]}", checker.rows)))
    assert [place for place, _, _ in rows] == [place for place, _ in plan_of(vit, uint8=table32 is not None, fp8=form.fp8, route=form.route).stages]
    assert all(ratio <= 1.0 for _, _, ratio in rows)
