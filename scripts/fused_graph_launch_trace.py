"""Host-side stand-in for ``fused_graph_parity.py`` (no GPU): which launches the fused graphs make, with which operands.

Every HIP wrapper ``hovernet_fused`` / ``unet_fused`` call through their module globals is replaced by a plain-torch definition
that also LOGS the call -- wrapper name, every argument by parameter name with the wrapper's defaults filled in, tensors as shape /
dtype / strides / SHA-1 of their bytes -- for the 20 cases of ``fused_graph_parity.py`` (five seeded inputs x float32 direct,
float32 winograd, fp16, bf16).  Two checkouts whose logs are equal hand the C library the same sequence of calls with bit-identical
operands; the packing calls are compared as a multiset (their order is no launch order).

    python scripts/fused_graph_launch_trace.py --tree ../parent --out parent.json
    python scripts/fused_graph_launch_trace.py --out head.json
    python scripts/fused_graph_launch_trace.py --compare parent.json head.json
"""
import argparse
import copy
import hashlib
import inspect
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
args = ap.parse_args()
if args.compare:
    a, b = (json.load(open(p)) for p in args.compare)
    assert list(a) == list(b), "different cases"
    print(f"{'case':34s} {'launches':>8s} {'packs':>6s}  launch log ({args.compare[0]} | {args.compare[1]})  packs   outputs")
    bad = 0
    for c in a:
        same = [a[c][k] == b[c][k] for k in ("log_sha1", "packs_sha1", "outputs")]
        bad += not all(same)
        print(f"{c:34s} {a[c]['calls']:8d} {a[c]['packs']:6d}  {a[c]['log_sha1'][:12]} {'==' if same[0] else '!='} {b[c]['log_sha1'][:12]}   "
              f"{'equal' if same[1] else 'DIFFER'}   {'equal' if same[2] else 'DIFFER'}")
    print("all equal" if not bad else f"{bad} case(s) differ")
    sys.exit(1 if bad else 0)
tree = os.path.abspath(args.tree)
sys.path[:0] = [tree, os.path.join(tree, "tests")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402, N812
import tiatoolbox_amd.models.architecture.hovernet_fused as hf  # noqa: E402
import tiatoolbox_amd.models.architecture.unet_fused as uf  # noqa: E402
import _hovernet_half_ref as H  # noqa: E402, N812
import _unet_half_ref as U  # noqa: E402, N812
from tiatoolbox_amd.models.architecture.hovernet import HoVerNet  # noqa: E402
from tiatoolbox_amd.models.architecture.unet import UNetModel  # noqa: E402

LOG = []


def digest(v):
    if isinstance(v, torch.Tensor):
        return [list(v.shape), str(v.dtype), list(v.stride()), hashlib.sha1(v.detach().reshape(-1).contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()]
    if isinstance(v, torch.nn.Module):
        return ["module", digest(v.weight)]
    if isinstance(v, (tuple, list)):
        return [digest(e) for e in v]
    return repr(v)


def logged(name, fn):
    def wrapper(*a, **k):
        out = fn(*a, **k)
        # `out=` of the grouped kernel is a destination, not an operand: log where it points, not what it held
        bound = inspect.signature(fn).bind(*a, **k)  # by parameter name, defaults filled in: what the C entry point is given
        bound.apply_defaults()
        kk = {key: (digest(val)[:3] if key == "out" and val is not None else digest(val)) for key, val in sorted(bound.arguments.items())}
        LOG.append([name, kk, digest(out)])
        return out
    return wrapper


def aff(x, sc, sh):
    return F.relu(x * sc[None, :, None, None] + sh[None, :, None, None])


def conv(x, w_oihw, bias, res, stride, lo, hi, relu):
    v = F.conv2d(F.pad(x.float(), (lo, hi, lo, hi)), w_oihw.float(), bias, stride)
    v = v + res.float() if res is not None else v
    return F.relu(v) if relu else v


def conv_ex(x, wp, bias, res, *, kernel, stride, pad_lo, pad_hi, relu):
    return conv(x, wp.permute(3, 2, 0, 1), bias, res, stride, pad_lo, pad_hi, relu)


def conv_post(x, wp, bias, res, *, kernel, stride, pad_lo, pad_hi, relu, post_scale, post_shift, want_raw=True):
    v = conv_ex(x, wp, bias, res, kernel=kernel, stride=stride, pad_lo=pad_lo, pad_hi=pad_hi, relu=relu)
    return (v if want_raw else None), aff(v, post_scale, post_shift)


def conv_pre(x, pre_scale, pre_shift, wp, bias, res=None, *, stride=1, relu=False):
    return conv_ex(aff(x, pre_scale, pre_shift), wp, bias, res, kernel=1, stride=stride, pad_lo=0, pad_hi=0, relu=relu)


def wino(x, u, bias, res, *, padding, relu, pad_hi=None):
    return conv(x, u, bias, res, 1, padding, padding if pad_hi is None else pad_hi, relu)


def conv_h(x, wp, bias, res, *, cout, kernel, stride, padding, relu):
    return conv(x, H.unpack_h(wp), bias, res, stride, padding, padding, relu).to(x.dtype)


def conv_h_ex(x, wp, bias, res, *, cout, kernel, stride, pad_lo, pad_hi, relu, post_scale=None, post_shift=None, want_raw=True):
    v = conv(x, H.unpack_h(wp), bias, res, stride, pad_lo, pad_hi, relu)
    if post_scale is None:
        return v.to(x.dtype)
    return (v.to(x.dtype) if want_raw else None), aff(v, post_scale, post_shift).to(x.dtype)


def thin(x, wp, bias, *, kernel, stride, pad_lo, pad_hi, relu, out_dtype=torch.float32):
    c = x.shape[1]
    w = wp[:, :kernel * c].reshape(kernel, kernel, c, -1).permute(3, 2, 0, 1)
    return conv(x, w, bias, None, stride, pad_lo, pad_hi, relu).to(out_dtype)


def pack_thin(weight):
    cout, c, kh, kw = weight.shape
    packed = torch.zeros((kh, 32, cout))
    packed[:, :kw * c] = weight.detach().float().permute(2, 3, 1, 0).reshape(kh, kw * c, cout)
    return packed


def head(x, weight, bias, *, pre_scale=None, pre_shift=None):
    a = x.float() if pre_scale is None else aff(x.float(), pre_scale, pre_shift)
    return F.conv2d(a, weight.float().reshape(weight.shape[0], 64, 1, 1), bias)


def grouped(x, wp, *, groups, kernel, out=None):
    y = F.conv2d(x, wp.permute(0, 4, 3, 1, 2).reshape(groups * 8, 32, kernel, kernel), None, 1, 0, 1, groups)
    return y if out is None else out.copy_(y)


def grouped_h(x, wp, *, groups, kernel, out=None):
    y = F.conv2d(x.float(), H.unpack_grouped_h(wp).float(), None, 1, 0, 1, groups).to(x.dtype)
    return y if out is None else out.copy_(y)


def scale_shift(x, sc, sh, *, relu=True, inplace=False):
    y = x.float() * sc[None, :, None, None] + sh[None, :, None, None]
    return (F.relu(y) if relu else y).to(x.dtype)


def bias_act(y, bias, res=None, *, relu=True):
    y = y + bias[None, :, None, None]
    y = y + res if res is not None else y
    return F.relu(y) if relu else y


def up(x, y, scale=None, shift=None):
    s = x.float().repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) + y.float()
    return (s if scale is None else aff(s, scale, shift)).to(x.dtype)


def stem(x_nhwc, wp, bias, *, out_dtype=torch.float32, return_conv=False):
    w = wp[:147].view(7, 7, 3, 64).permute(3, 2, 0, 1)
    xf = x_nhwc.float().div(255) if x_nhwc.dtype == torch.uint8 else x_nhwc
    c = F.relu(F.conv2d(xf.permute(0, 3, 1, 2), w, bias, 2, 3))
    p = F.max_pool2d(c, 3, 2, 1)
    return (p.to(out_dtype), c.to(out_dtype)) if return_conv else p.to(out_dtype)


IMPL = {
    "hip_conv2d_ex": conv_ex, "hip_conv2d_post": conv_post, "hip_conv1x1_pre": conv_pre, "hip_conv3x3_wino": wino,
    "hip_conv2d_h": conv_h, "hip_conv2d_h_ex": conv_h_ex, "hip_conv2d_thin": thin, "hip_conv1x1_head": head,
    "hip_grouped_conv_valid": grouped, "hip_grouped_conv_valid_h": grouped_h, "hip_scale_shift_act": scale_shift,
    "hip_scale_shift_act_view": lambda x, sc, sh, relu=True: scale_shift(x, sc, sh, relu=relu), "hip_bias_act_": bias_act,
    "hip_upsample2x_add": up, "hip_stem_conv_pool": stem,
    "pack_conv_weights": lambda c: c.weight.detach().float().permute(2, 3, 1, 0).contiguous(),
    "pack_conv_weights_wino": lambda c: c.weight.detach().float().clone(),
    "pack_conv_weights_h": lambda c, dtype: H.pack_h(c.weight.detach().float(), dtype),
    "pack_grouped_conv_valid_weights_h": lambda w, groups, dtype: H.pack_grouped_h(w.detach().float(), groups, dtype),
    "pack_thin_conv_weights": pack_thin,
    "pack_stem_weights": lambda w: torch.cat([w.detach().float().permute(2, 3, 1, 0).reshape(147, 64), torch.zeros(1, 64)]),
}
for mod in (hf, uf):
    for name, fn in IMPL.items():
        if hasattr(mod, name):
            setattr(mod, name, logged(name, fn))
missing = [n for mod in (hf, uf) for n in dir(mod) if (n.startswith("hip_") or n.startswith("pack_")) and n not in IMPL]
assert not missing, missing

MODES = (("f32-direct", torch.float32, "direct"), ("f32-winograd", torch.float32, "winograd"), ("fp16", torch.float16, "direct"),
         ("bf16", torch.bfloat16, "direct"))
inputs = []
for kind in ("fast", "original", "plus"):
    model, x, _ = H.graph_case(kind)
    inputs.append((f"hovernet-{kind}-n1", model, x[:1]))
    if kind == "fast":
        inputs.append(("hovernet-fast-n2", model, x))
torch.manual_seed(2)
unet = UNetModel(3, 5, "resnet50", decoder_block=[3, 3]).eval()
g = U.randomise_bn(unet, 9)
inputs.append(("unet-n1", unet, torch.randint(0, 256, (1, 3, 96, 128), generator=g).float()))

record = {}
for name, model, x in inputs:
    for mode, dtype, algo in MODES:
        LOG.clear()
        fused = (hf.FusedHoVerNet if isinstance(model, HoVerNet) else uf.FusedUNet)(copy.deepcopy(model))
        hf.set_conv_algo(fused, algo)
        if dtype != torch.float32:
            fused.prepare(dtype)
            fused = fused.to(dtype)
        fused = fused.to(memory_format=torch.channels_last).eval()
        with torch.inference_mode():
            got = fused(x.to(dtype).contiguous(memory_format=torch.channels_last))
        heads = got if isinstance(got, dict) else {"logits": got}
        packs = sorted(json.dumps(e) for e in LOG if e[0].startswith("pack_"))  # (packing order is no launch order: as a multiset)
        LOG[:] = [e for e in LOG if not e[0].startswith("pack_")]
        record[f"{name}/{mode}"] = {"calls": len(LOG), "log_sha1": hashlib.sha1(json.dumps(LOG).encode()).hexdigest(),
                                    "packs": len(packs), "packs_sha1": hashlib.sha1(json.dumps(packs).encode()).hexdigest(),
                                    "by_wrapper": {n: sum(1 for e in LOG if e[0] == n) for n in sorted({e[0] for e in LOG})},
                                    "outputs": {k: digest(v) for k, v in heads.items()}, "log": copy.deepcopy(LOG)}
        print(name, mode, len(LOG), record[f"{name}/{mode}"]["log_sha1"], len(packs), record[f"{name}/{mode}"]["packs_sha1"], flush=True)
json.dump(record, open(args.out, "w"))
