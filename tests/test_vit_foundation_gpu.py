"""``FusedViT`` on the foundation models' graph (register tokens, a grid-only position table, a 14-pixel patch, packed SwiGLU) against
the float32 module on the CPU, by the criterion of ``test_vit_gpu._parity`` (at most twice the error of the torch module cast to
the same dtype on the same device); the kernels a bf16 forward launches; the engines' route to it."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_foundation_ref import TINY_GIGA, TINY_REG, tiny_foundation
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims, _parity

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
TINY_REG4 = {**TINY_REG, "reg_tokens": 4}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("size", [(28, 28), (112, 112), (42, 56)], ids=["28", "112", "42x56"])  # S = 9; 69 (a second key tile); 17
@pytest.mark.parametrize("n", [1, 3])
def test_fused_graph_matches_module_with_registers_and_swiglu(n, size, dtype):
    vit = tiny_foundation(TINY_REG4)
    x = torch.randn((n, 3, *size), generator=torch.Generator().manual_seed(size[0] + size[1] + n))
    _parity(vit, x, dtype, f"tiny patch 14, R=4, no_embed_class, SwiGLU n={n} {size[0]}x{size[1]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("n", [1, 3])
def test_fused_graph_matches_module_in_the_gigapath_form(n, size, dtype):
    vit = tiny_foundation(TINY_GIGA)
    x = torch.randn((n, 3, size, size), generator=torch.Generator().manual_seed(size + n))
    _parity(vit, x, dtype, f"tiny patch 16, R=0, SwiGLU n={n} {size}^2")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_fused_graph_matches_module_at_uni2_width(dtype):
    """UNI2-h's widths at depth 1: the 1536 -> 4608 / 8192 and 4096 -> 1536 GEMMs, LayerNorm and SwiGLU rows of 1536 / 4096, the
    608-column patch GEMM, S = 1 + 8 + 256 = 265."""
    vit = tiny_foundation(TINY_REG, embed_dim=1536, num_heads=24, mlp_dim=8192, reg_tokens=8, img_size=224, depth=1)
    x = torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(9))
    _parity(vit, x, dtype, "UNI2-h width, depth 1, n=1")


def test_bf16_forward_launches_the_new_kernels_and_no_library():
    from tiatoolbox_amd.models.architecture.vit_fused import FusedViT

    fused = FusedViT(tiny_foundation(TINY_REG4).cuda())
    fused.prepare(torch.bfloat16)
    fused = fused.to(torch.bfloat16)
    x = torch.randn((2, 3, 56, 56), device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        fused(x)
        kernels = _device_kernels(lambda: fused(x))
    for wanted in ("mha_fwd_h_kernel", "layernorm_rows_h_kernel", "conv_mfma_h", "swiglu_rows_h_kernel", "vit_patchify_pad_h_kernel",
                   "vit_assemble_prefix_h_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == {64}, kernels  # (the head_dim-64 instantiation of the one attention kernel, and no other)
    assert not {k for k in kernels if "gelu_rows_h_kernel" in k or "vit_assemble_tokens_h_kernel" in k}, kernels
    assert not {k for k in kernels if _banned(k)}, kernels


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def test_engine_runs_a_foundation_backbone_on_the_fused_graph_in_bf16(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")
    model.feat_extract = tiny_foundation(TINY_REG4, img_size=224, dynamic_img_size=False)  # a 16 x 16 grid: S = 261
    patches = np.random.default_rng(2).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    ref = DeepFeatureExtractor(copy.deepcopy(model), batch_size=2).run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(copy.deepcopy(model), batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    assert not [r for r in caplog.records if "Vision Transformer" in r.getMessage() or "torch module" in r.getMessage()]
    fast = eng._inference_model(torch.bfloat16)  # noqa: SLF001  (the cached copy the run used)
    assert [type(m).__name__ for m in fast.modules()].count("FusedViT") == 1
    with torch.inference_mode():
        x = torch.from_numpy(patches).cuda().to(torch.bfloat16).permute(0, 3, 1, 2)
        lib = copy.deepcopy(model).cuda().to(torch.bfloat16)(x).float().cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_lib = float(np.abs(got - ref).max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"engine tiny foundation bf16: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert got.shape == (3, 128) and got.dtype == np.float32 and np.isfinite(got).all() and e_new <= 2.0 * e_lib
    # dynamic_img_size is off: another grid is refused with the module's message, before anything is launched
    small = torch.zeros((2, 3, 112, 112), device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()

    def refused():
        with torch.inference_mode(), pytest.raises(ValueError, match="dynamic_img_size"):
            fast.feat_extract(small)

    assert _device_kernels(refused) == set()
