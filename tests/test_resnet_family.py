"""The torchvision ResNet family beyond resnet18/34/50: resnet101, ResNeXt (grouped 3x3) and Wide-ResNet trunks, their
kather100k registry entries and bare backbone names.  Host-only: no GPU needed."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from tiatoolbox_amd.models.architecture import get_pretrained_model
from tiatoolbox_amd.models.architecture.resnet import resnet_trunk
from tiatoolbox_amd.models.architecture.vanilla import CNNModel
from tiatoolbox_amd.models.engine.io_config import IOPatchPredictorConfig
from tiatoolbox_amd.utils import synth

NEW = ("resnet101", "resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2", "wide_resnet101_2")

# torchvision's published parameter counts (trunk + Linear(2048, 1000))
TORCHVISION_PARAMS = {
    "resnet50": 25_557_032,
    "resnet101": 44_549_160,
    "resnext50_32x4d": 25_028_904,
    "resnext101_32x8d": 88_791_336,
    "wide_resnet50_2": 68_883_240,
    "wide_resnet101_2": 126_886_696,
}


@pytest.mark.parametrize("name", list(TORCHVISION_PARAMS))
def test_trunk_parameter_count_matches_torchvision(name):
    trunk = resnet_trunk(name)
    fc = 2048 * 1000 + 1000
    assert sum(p.numel() for p in trunk.parameters()) + fc == TORCHVISION_PARAMS[name]


@pytest.mark.parametrize(("name", "shape"), [("resnext50_32x4d", (128, 4, 3, 3)), ("resnext101_32x8d", (256, 8, 3, 3)),
                                             ("wide_resnet50_2", (128, 128, 3, 3))])
def test_weight_shapes_follow_torchvision_width_rule(name, shape):
    sd = CNNModel(name, num_classes=9).state_dict()
    assert tuple(sd["feat_extract.4.0.conv2.weight"].shape) == shape
    assert tuple(sd["classifier.weight"].shape) == (9, 2048)
    groups = 32 if name.startswith("resnext") else 1
    assert all(m.groups == groups for n, m in resnet_trunk(name).named_modules() if n.endswith("conv2"))


def test_state_dict_round_trips_strictly():
    """Parameter names are torchvision's children layout: a saved state dict loads back with ``strict=True``."""
    torch.manual_seed(1)
    a = CNNModel("resnext50_32x4d", num_classes=9)
    torch.manual_seed(2)
    b = CNNModel("resnext50_32x4d", num_classes=9)
    b.load_state_dict(a.state_dict(), strict=True)
    assert all(torch.equal(a.state_dict()[k], v) for k, v in b.state_dict().items())


def test_unknown_backbones_stay_unsupported():
    for name in ("densenet121", "mobilenet_v2", "resnet152", "resnext"):
        with pytest.raises(ValueError, match="not supported"):
            CNNModel(name)


@pytest.mark.parametrize("name", NEW)
def test_registry_entry_gives_kather100k_classifier(name):
    model, cfg = get_pretrained_model(f"{name}-kather100k")
    assert isinstance(model, CNNModel) and model.num_classes == 9
    assert isinstance(cfg, IOPatchPredictorConfig)
    ref = get_pretrained_model("resnet18-kather100k")[1]
    assert list(cfg.patch_input_shape) == list(ref.patch_input_shape) == [224, 224]
    assert list(cfg.stride_shape) == list(ref.stride_shape) == [224, 224]
    assert cfg.input_resolutions == ref.input_resolutions == [{"resolution": 0.5, "units": "mpp"}]
    assert model.preproc_func is not None


def test_deep_feature_extractor_on_resnext_backbone():
    """``DeepFeatureExtractor("resnext50_32x4d")``: a bare backbone name gives the 2048-wide pooled features of the module's own
    CPU forward."""
    from tiatoolbox_amd.models import DeepFeatureExtractor

    patches = synth.g_he(2, 64, 64, seed=31)
    eng = DeepFeatureExtractor("resnext50_32x4d", batch_size=2)
    assert eng.ioconfig is None
    cfg = IOPatchPredictorConfig(input_resolutions=[{"units": "baseline", "resolution": 1.0}], patch_input_shape=(64, 64),
                                 stride_shape=(64, 64))
    out = eng.run(patches, patch_mode=True, ioconfig=cfg)
    assert out["probabilities"].shape == (2, 2048)
    with torch.inference_mode():
        ref = eng.model.eval()(torch.from_numpy(patches).float().permute(0, 3, 1, 2)).numpy()
    np.testing.assert_allclose(out["probabilities"], ref, atol=1e-5)


@pytest.mark.parametrize("name", ["resnext50_32x4d", "wide_resnet50_2"])
def test_torchvision_topology_matches_the_restated_trunk(name):
    """Where torchvision exists, the restated trunk loads its state dict strictly and gives the same feature maps."""
    tv = pytest.importorskip("torchvision")

    torch.manual_seed(0)
    real = getattr(tv.models, name)(weights=None).eval()
    for m in real.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    trunk = resnet_trunk(name).eval()
    names = ["conv1", "bn1", "relu", "maxpool", "layer1", "layer2", "layer3", "layer4"]
    mapped = {}
    for k, v in real.state_dict().items():
        head, rest = k.split(".", 1)
        if head != "fc":
            mapped[f"{names.index(head)}.{rest}"] = v
    trunk.load_state_dict(mapped, strict=True)
    x = torch.randn(2, 3, 96, 96)
    with torch.no_grad():
        a = trunk(x)
        b = real.layer4(real.layer3(real.layer2(real.layer1(real.maxpool(real.relu(real.bn1(real.conv1(x))))))))
    assert torch.allclose(a, b, atol=1e-5), float((a - b).abs().max())
