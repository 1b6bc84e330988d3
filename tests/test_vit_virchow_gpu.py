"""``FusedViT`` on the ``Virchow`` / ``Virchow2`` graph (80 dimensions per head, padded SwiGLU halves, register tokens with position
entries of their own, the class + mean-patch output) against the float32 module on the CPU, by the criterion of
``test_vit_gpu._parity`` (at most twice the error of the torch module cast to the same dtype on the same device); the engine's route to
it and the kernels its forward launches."""

from __future__ import annotations

import copy
import logging

import numpy as np
import pytest
import torch

from _vit_virchow_ref import NO_PAD, TINY_V1, TINY_V2, tiny_virchow
from test_vit_gpu import _banned, _device_kernels, _mha_head_dims, _parity

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
FORMS = {"v1": TINY_V1, "v2": TINY_V2}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("size", [(28, 28), (112, 112), (42, 56)], ids=["28", "112", "42x56"])  # S = 5 / 8; 65 / 68 (a second key tile); 13 / 16
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("form", ["v1", "v2"])
def test_fused_graph_matches_module(form, n, size, dtype):
    vit = tiny_virchow(FORMS[form])
    x = torch.randn((n, 3, *size), generator=torch.Generator().manual_seed(size[0] + size[1] + n))
    _parity(vit, x, dtype, f"tiny Virchow {form} (80 per head, H 520 -> 544, token_mean) n={n} {size[0]}x{size[1]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_fused_graph_matches_module_without_padding(dtype):
    vit = tiny_virchow(TINY_V2, **NO_PAD)
    x = torch.randn((2, 3, 28, 28), generator=torch.Generator().manual_seed(5))
    _parity(vit, x, dtype, "tiny Virchow v2, H 512 (no pad) n=2 28x28")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_fused_graph_matches_module_at_virchow2_width(dtype):
    """Virchow2's widths at depth 1: the 1280 -> 3840 / 6848 and 3424 -> 1280 GEMMs, LayerNorm rows of 1280, SwiGLU rows of 3424, 16
    heads of 80, the pooled norm over S = 1 + 4 + 256 = 261 rows."""
    vit = tiny_virchow(TINY_V2, embed_dim=1280, num_heads=16, mlp_dim=6832, reg_tokens=4, img_size=224, depth=1)
    x = torch.randn((1, 3, 224, 224), generator=torch.Generator().manual_seed(9))
    _parity(vit, x, dtype, "Virchow2 width, depth 1, n=1")


def _cfg():
    from tiatoolbox_amd.models import IOPatchPredictorConfig

    return IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(224, 224),
                                  stride_shape=(224, 224))


def test_engine_runs_virchow2_on_the_fused_graph_in_bf16(caplog):
    from tiatoolbox_amd.models import DeepFeatureExtractor
    from tiatoolbox_amd.models.architecture.vanilla import TimmBackbone

    model = TimmBackbone("vit_small_patch16_224")  # (`Virchow2` is no TimmBackbone name yet: the module rides in another backbone)
    model.feat_extract = tiny_virchow(TINY_V2, img_size=224)  # a 16 x 16 grid: S = 1 + 3 + 256 = 260
    patches = np.random.default_rng(2).integers(0, 256, (3, 224, 224, 3), dtype=np.uint8)
    ref = DeepFeatureExtractor(copy.deepcopy(model), batch_size=2).run(patches, patch_mode=True, ioconfig=_cfg())["probabilities"]
    eng = DeepFeatureExtractor(copy.deepcopy(model), batch_size=2, device="cuda")
    with caplog.at_level(logging.WARNING, logger="tiatoolbox_amd"):
        got = eng.run(patches, patch_mode=True, ioconfig=_cfg(), compute_dtype="bfloat16")["probabilities"]
    assert not [r for r in caplog.records if any(w in r.getMessage() for w in ("Vision Transformer", "torch module", "head_dim", "FusedViT"))]
    fast = eng._inference_model(torch.bfloat16)  # noqa: SLF001  (the cached copy the run used)
    assert [type(m).__name__ for m in fast.modules()].count("FusedViT") == 1
    with torch.inference_mode():
        x = torch.from_numpy(patches).cuda().to(torch.bfloat16).permute(0, 3, 1, 2)
        lib = copy.deepcopy(model).cuda().to(torch.bfloat16)(x).float().cpu().numpy()
    scale = max(float(np.abs(ref).max()), 1.0)
    e_new, e_lib = float(np.abs(got - ref).max()) / scale, float(np.abs(lib - ref).max()) / scale
    print(f"engine tiny Virchow2 bf16: e_new {e_new:.3e}  e_lib {e_lib:.3e}")
    assert got.shape == (3, 640) and got.dtype == np.float32 and np.isfinite(got).all() and e_new <= 2.0 * e_lib
    # what that forward launches: the 80 attention form and the pooling kernel, no library kernel
    xin = x.contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        kernels = _device_kernels(lambda: fast.feat_extract(xin))
    for wanted in ("mha_fwd_h_kernel", "vit_cls_mean_pool_h_kernel", "layernorm_rows_h_kernel", "conv_mfma_h", "swiglu_rows_h_kernel",
                   "vit_patchify_pad_h_kernel", "vit_assemble_prefix_h_kernel"):
        assert any(wanted in k for k in kernels), (wanted, kernels)
    assert _mha_head_dims(kernels) == {80}, kernels  # (the head_dim-80 instantiation of the one attention kernel, and none with 64)
    assert not {k for k in kernels if "vit_assemble_tokens_h_kernel" in k or "gelu_rows_h_kernel" in k}, kernels
    assert not {k for k in kernels if _banned(k)}, kernels
