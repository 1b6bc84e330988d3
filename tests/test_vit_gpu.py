"""``FusedViT`` (the Vision Transformer graph on the hand-written kernels) against the float32 module on the CPU, with the cast torch
module on the same device and dtype as the yardstick; the engines' route to it; and: the bf16 run launches no library kernel."""

from __future__ import annotations

import copy
import logging
import re

import numpy as np
import pytest
import torch

from _vit_ref import randomise, tiny_vit

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _parity(vit, x: torch.Tensor, dtype: torch.dtype, what: str) -> None:
    """``e = max |feat - ref| / max(max |ref|, 1)`` with ``ref`` the float32 module on the CPU: the fused graph at most twice the error
    of the torch module cast to ``dtype`` on the same device."""
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    with torch.inference_mode():
        ref = vit(x).double()
        lib = copy.deepcopy(vit).cuda().to(dtype)(x.cuda().to(dtype)).float().cpu().double()
        fused = FusedViT(copy.deepcopy(vit).cuda())
        fused.prepare(dtype)
        fused = fused.to(dtype)
        xin = x.cuda().to(dtype).contiguous(memory_format=torch.channels_last)  # what `infer_batch` hands over
        got = fused(xin)
        assert got.shape == ref.shape and got.dtype == torch.float32
        assert torch.equal(fused(x.cuda()), got)  # a float32 batch is rounded once on the way in: the same tokens
        got = got.cpu().double()
    scale = max(float(ref.abs().max()), 1.0)
    e_new, e_lib = float((got - ref).abs().max()) / scale, float((lib - ref).abs().max()) / scale
    print(f"{what} {dtype}: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert bool(torch.isfinite(got).all()) and e_new <= 2.0 * e_lib


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("layer_scale", [False, True])
@pytest.mark.parametrize("size", [32, 64, 224])
@pytest.mark.parametrize("n", [1, 3])
def test_fused_graph_matches_module(n, size, layer_scale, dtype):
    vit = tiny_vit(layer_scale=layer_scale, dynamic=True)
    x = torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(size + n))
    _parity(vit, x, dtype, f"tiny n={n} {size}^2 layer_scale={layer_scale}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_fused_graph_matches_module_at_uni_shape(dtype):
    vit = tiny_vit(layer_scale=True, dynamic=True, embed_dim=1024, num_heads=16, mlp_dim=4096, img_size=224)
    x = torch.randn((2, 3, 224, 224), generator=torch.Generator().manual_seed(9))
    _parity(vit, x, dtype, "UNI shape, depth 2, n=2")


def test_fused_graph_resamples_positions_and_refuses_off_grid():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    x = torch.randn((2, 3, 48, 64), generator=torch.Generator().manual_seed(4))
    _parity(tiny_vit(dynamic=True), x, torch.bfloat16, "tiny 48x64")
    fused = FusedViT(tiny_vit(dynamic=False).cuda())
    fused.prepare(torch.float16)
    with pytest.raises(ValueError, match="dynamic_img_size"):
        fused(x.cuda().half())
    with pytest.raises(ValueError, match="float16 or bfloat16"):
        FusedViT(tiny_vit().cuda()).prepare(torch.float32)


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


@pytest.fixture(scope="module")
def vit_small_runs():
    """One randomised ``vit_small_patch16_224`` for the engine tests: patches, the engine, its CPU float32 features."""
    from tiatoolbox_amd.models import DeepFeatureExtractor

    patches = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    cpu = DeepFeatureExtractor("vit_small_patch16_224", batch_size=2)
    randomise(cpu.model.feat_extract)
    ref = cpu.run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor("vit_small_patch16_224", batch_size=2, device="cuda")
    eng.model.feat_extract.load_state_dict(cpu.model.feat_extract.state_dict(), strict=True)
    return patches, eng, cpu.model, ref


def test_engine_runs_vit_on_fused_graph_in_bf16(vit_small_runs, caplog):
    patches, eng, model, ref = vit_small_runs
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16", conv_algo="direct")["probabilities"]
    assert not [r for r in caplog.records if "Vision Transformer" in r.getMessage() or "torch module" in r.getMessage()]
    fast = eng._inference_model(torch.bfloat16)  # noqa: SLF001  (the cached copy the run used)
    assert [type(m).__name__ for m in fast.modules()].count("FusedViT") == 1
    with torch.inference_mode():
        x = torch.from_numpy(patches).cuda().to(torch.bfloat16).permute(0, 3, 1, 2)
        lib = copy.deepcopy(model).cuda().to(torch.bfloat16)(x).float().cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_lib = float(np.abs(got - ref).max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"engine vit_small bf16: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert got.shape == (3, 384) and got.dtype == np.float32 and e_new <= 2.0 * e_lib


def test_engine_float32_keeps_the_torch_module_and_says_so(vit_small_runs, caplog):
    patches, eng, _, ref = vit_small_runs
    eng.invalidate_inference_cache()
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="float32")["probabilities"]
        eng.run(patches[:1], patch_mode=True, ioconfig=_cfg(), compute_dtype="float32")  # the same inference copy: no second warning
    said = [r.getMessage() for r in caplog.records if "Vision Transformer" in r.getMessage()]
    assert len(said) == 1 and 'compute_dtype="bfloat16"' in said[0] and "library" in said[0]
    fast = eng._inference_model(torch.float32)  # noqa: SLF001
    assert "FusedViT" not in [type(m).__name__ for m in fast.modules()]
    assert float(np.abs(got - ref).max()) <= 1e-4 * float(np.abs(ref).max())


def test_engine_keeps_the_torch_module_for_head_dim_32(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")
    model.feat_extract = tiny_vit(num_heads=4, img_size=224, dynamic=False)  # 128 / 4 = 32 per head
    patches = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    ref = DeepFeatureExtractor(copy.deepcopy(model), batch_size=2).run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(model, batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    said = [r.getMessage() for r in caplog.records if "head_dim 64" in r.getMessage()]
    assert len(said) == 1 and "torch module" in said[0]
    fast = eng._inference_model(torch.bfloat16)  # noqa: SLF001
    assert "FusedViT" not in [type(m).__name__ for m in fast.modules()]
    assert next(fast.parameters()).dtype == torch.bfloat16
    assert float(np.abs(got - ref).max()) <= 0.1 * max(float(np.abs(ref).max()), 1.0)  # (a bf16 torch run: sanity only)


def _device_kernels(fn) -> set:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()}
    return {n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()}


def _banned(name: str) -> bool:
    low = name.lower()
    return any(b in low for b in ("cijk_", "rocblas", "hipblaslt", "gemm", "fmha", "miopen")) or ("attention" in low and "ck" in low)


def _mha_head_dims(kernels) -> set[int]:
    """The ``head_dim`` of every ``mha_fwd_h_kernel<BF, HD>`` instantiation among ``kernels``: the profiler prints the template
    arguments, and a name without them counts as no instantiation at all."""
    return {int(m.group(1)) for m in (re.search(r"mha_fwd_h_kernel<[^>]*\b(\d+)>", k) for k in kernels) if m}


def test_bf16_forward_launches_only_handwritten_kernels():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(tiny_vit(layer_scale=True, dynamic=True).cuda())
    fused.prepare(torch.bfloat16)
    fused = fused.to(torch.bfloat16)
    x = torch.randn((2, 3, 64, 64), device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused(x)
        kernels = _device_kernels(lambda: fused(x))
    for wanted in ("mha_fwd_h_kernel", "layernorm_rows_h_kernel", "conv_mfma_h", "gelu_rows_h_kernel", "vit_patchify_h_kernel",
                   "vit_assemble_tokens_h_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == {64}, kernels  # (the head_dim-64 instantiation of the one attention kernel, and no other)
    assert not {k for k in kernels if _banned(k)}, kernels
