"""Shared by ``test_wino_split.py`` (host) and ``test_wino_split_gpu.py``: a torch emulation of the arithmetic of
``conv3x3_wino_bf16x3_kernel``, a restatement of its packed weight layout, and the builders of the EXACT cases -- inputs
whose result involves no rounded sum anywhere in the Winograd domain, so that kernel and float64 convolution must agree bit for bit.

The emulation: ``V = B^T d B`` in float32 with the kernel's two add levels (rows, then columns), ``U = G g G^T`` from
``fused.wino_weights_f32`` (float64, rounded once), per position the GEMM ``M = V U`` through ``_conv_split_cases.emulate_gemm`` (both
operands split into three bf16 numbers, six products per 16-channel step into one float32 accumulator, in the kernel's order), and the
output transform ``A^T M A`` in float32 in the kernel's order (columns in registers, rows across the waves).
"""

from __future__ import annotations

import torch
import torch.nn.functional as F  # noqa: N812

from _conv_split_cases import ORDER, emulate_gemm
from tiatoolbox_amd.models.architecture.fused import wino_weights_f32


def input_tiles(x: torch.Tensor, pad: int) -> torch.Tensor:
    """NCHW ``x`` -> ``[n, c, tiles_y, tiles_x, 4, 4]``: the 4 x 4 input window of every 2 x 2 output tile (zeros outside the map)."""
    _, _, h, w = x.shape
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    ty, tx = (ho + 1) // 2, (wo + 1) // 2
    xp = F.pad(x, (pad, 2 * tx + 2 - w - pad, pad, 2 * ty + 2 - h - pad))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)


def input_transform(d: torch.Tensor) -> torch.Tensor:
    """``V = B^T d B`` over the last two dimensions in the dtype of ``d``, the kernel's order: R_i = d[ra] +- d[rb], then
    V[i][j] = R_i[c] +- R_i[c']."""
    r = torch.stack((d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]), -2)
    return torch.stack((r[..., 0] - r[..., 2], r[..., 1] + r[..., 2], r[..., 2] - r[..., 1], r[..., 1] - r[..., 3]), -1)


def output_transform(m: torch.Tensor) -> torch.Tensor:
    """``Y = A^T M A`` over the last two dimensions (4 x 4 -> 2 x 2) in the dtype of ``m``, the kernel's order: columns
    Z[i][0] = (M0 + M1) + M2, Z[i][1] = (M1 - M2) - M3, then rows Y[0] = (Z0 + Z1) + Z2, Y[1] = Z1 + (-Z3 - Z2)."""
    z = torch.stack(((m[..., 0] + m[..., 1]) + m[..., 2], (m[..., 1] - m[..., 2]) - m[..., 3]), -1)
    return torch.stack(((z[..., 0, :] + z[..., 1, :]) + z[..., 2, :], z[..., 1, :] + (-z[..., 3, :] - z[..., 2, :])), -2)


def _untile(y: torch.Tensor, ho: int, wo: int) -> torch.Tensor:
    """``[n, tiles_y, tiles_x, cout, 2, 2]`` -> NCHW ``[n, cout, ho, wo]``."""
    n, ty, tx, cout = y.shape[:4]
    return y.permute(0, 3, 1, 4, 2, 5).reshape(n, cout, 2 * ty, 2 * tx)[:, :, :ho, :wo].contiguous()


def emulate_conv(x: torch.Tensor, weight: torch.Tensor, pad: int, *, split: bool = True) -> torch.Tensor:
    """The kernel's arithmetic for ``conv2d(x, weight, padding=pad)`` (3 x 3, stride 1, no bias), NCHW float32.  ``split=False``: the
    float32 Winograd form's (the same transforms, the GEMM one float32 product-sum per channel pair as v_mfma_f32_32x32x2_f32)."""
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    v = input_transform(input_tiles(x.float(), pad))          # [n, cin, ty, tx, 4, 4] float32
    u = wino_weights_f32(weight)                              # [cout, cin, 4, 4] float32
    ty, tx = v.shape[2], v.shape[3]
    m = torch.empty((n, ty, tx, cout, 4, 4))
    for i in range(4):
        for j in range(4):
            a = v[..., i, j].permute(0, 2, 3, 1).reshape(-1, cin)
            b = u[:, :, i, j].t().contiguous()
            if split:
                mm = emulate_gemm(a, b)
            else:
                mm = torch.zeros((a.shape[0], cout), dtype=torch.float64)
                for k0 in range(0, cin, 2):
                    mm = (mm + a[:, k0:k0 + 2].double() @ b[k0:k0 + 2].double()).float().double()
                mm = mm.float()
            m[..., i, j] = mm.reshape(n, ty, tx, cout)
    return _untile(output_transform(m), ho, wo)


def dropped_terms_bound(x: torch.Tensor, weight: torch.Tensor, pad: int):
    """Per (tile, position, output channel): |sum of the three dropped products| and 2^-23 sum |V| |U| (float64)."""
    from _conv_split_cases import DROPPED

    v = input_transform(input_tiles(x.float(), pad))
    u = wino_weights_f32(weight)
    cin, cout = x.shape[1], weight.shape[0]
    out = []
    for i in range(4):
        for j in range(4):
            a = v[..., i, j].permute(0, 2, 3, 1).reshape(-1, cin)
            b = u[:, :, i, j].t().contiguous()
            lost = emulate_gemm(a, b, terms=DROPPED, fp64_accumulate=True).abs()
            bound = 2.0 ** -23 * (a.double().abs() @ b.double().abs())
            out.append((lost, bound))
    assert out[0][0].shape == (a.shape[0], cout)
    return out


def packed_index(cout: int, cin: int) -> torch.Tensor:
    """For every element of the packed tensor ``[cin/16, 2, cout/64, 8, 3, 2, 64, 8]`` (16-channel slice, column pair jh of the position
    grid, 64-column block, position 2 i + jl, plane, 8-channel k-chunk, column, channel) the flat index of its source in
    ``parts [3, cout, cin, 4, 4]``."""
    cs, jh, cb, pos, p, q, col, e = torch.meshgrid(*(torch.arange(s) for s in (cin // 16, 2, cout // 64, 8, 3, 2, 64, 8)), indexing="ij")
    i, j = pos >> 1, 2 * jh + (pos & 1)
    o, ch = 64 * cb + col, 16 * cs + 8 * q + e
    return (((p * cout + o) * cin + ch) * 4 + i) * 4 + j


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
def assert_exact_in_the_winograd_domain(x: torch.Tensor, weight: torch.Tensor, pad: int, quantum: float) -> torch.Tensor:
    """The exactness bound of a case, asserted on the host: every V and every U is an integer multiple of a power of two whose product is
    ``quantum``, V and U are float32 numbers, and A^T (|V| |U|) A in absolute values -- an upper bound of every partial sum the kernel
    or the reference can form, in any order -- stays below 2^24 quanta.  Then every product and every sum is exact in float32 and the
    float64 convolution IS the result; returns it as float32."""
    d = input_tiles(x.double(), pad)
    v = input_transform(d)
    assert torch.equal(v, input_transform(d.float()).double()), "V is not exact in float32"
    g = weight.double()
    u = wino_weights_f32(weight).double()
    gm = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    assert torch.equal(u, gm @ g @ gm.t()), "U is not exact in float32"
    qv = min(float(2.0 ** torch.floor(torch.log2(v[v != 0].abs())).min()), 1.0)
    while not torch.equal((v / qv).round(), v / qv):
        qv /= 2
    qu = quantum / qv
    assert torch.equal((u / qu).round(), u / qu), "U is not a multiple of its quantum"
    m = torch.einsum("nctxij,ocij->ntxoij", v.abs(), u.abs())
    a = torch.tensor([[1, 1, 1, 0], [0, 1, 1, 1]], dtype=torch.float64)
    bound = (a @ m @ a.t()).max().item() / quantum
    assert bound < 2 ** 24, bound
    y = F.conv2d(x.double(), g, None, 1, pad)
    assert torch.equal(y.float().double(), y)
    return y.float()


def _isolated(n: int, cin: int, h: int, w: int, value, gen: torch.Generator) -> torch.Tensor:
    """Zeros except one pixel per 4 x 4 input window (a grid of pitch 4, shifted per image), one channel each: ``value(gen)``."""
    x = torch.zeros((n, cin, h, w))
    for b in range(n):
        for yy in range(b % 4, h, 4):
            for xx in range((b + 1) % 4, w, 4):
                x[b, int(torch.randint(0, cin, (1,), generator=gen)), yy, xx] = value(gen)
    return x


def case_isolated_activations(pad: int, *, n: int = 5, cin: int = 48, cout: int = 128, h: int = 19, w: int = 13):
    """(i) Integer activations with 17 significant bits (all three planes), isolated so that every V is +-a or 0, at every position of the
    4 x 4 window over the tiles; weights in {-1, 0, 1} on all nine taps (U in quarters)."""
    g = torch.Generator().manual_seed(100 + pad)

    def value(gen):
        a = int(torch.randint(1 << 16, 1 << 17, (1,), generator=gen)) | 1
        return float(a if int(torch.randint(0, 2, (1,), generator=gen)) else -a)

    x = _isolated(n, cin, h, w, value, g)
    wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
    return x, wt, assert_exact_in_the_winograd_domain(x, wt, pad, 0.25)


def case_isolated_powers_of_two(pad: int, *, n: int = 3, cin: int = 48, cout: int = 128, h: int = 19, w: int = 13):
    """(ii) The mirror image for the weight planes: integer weights below 2^15 (U in quarters, up to 20 significant bits), isolated
    activations +-2^k, k = 0..2."""
    g = torch.Generator().manual_seed(200 + pad)

    def value(gen):
        return (-1.0) ** int(torch.randint(0, 2, (1,), generator=gen)) * 2.0 ** int(torch.randint(0, 3, (1,), generator=gen))

    x = _isolated(n, cin, h, w, value, g)
    wt = torch.randint(-(1 << 15) + 1, 1 << 15, (cout, cin, 3, 3), generator=g).float()
    return x, wt, assert_exact_in_the_winograd_domain(x, wt, pad, 0.25)


def case_mid_mid(pad: int, *, n: int = 3, cin: int = 16, cout: int = 64, h: int = 19, w: int = 13):
    """(iii) a = 1 + 2^-10 in isolated pixels of one channel, w = 1 + 2^-10 on the centre tap of that channel: V = +-a, U = +-a / 4
    (hi and mid planes), and the output (1 + 2^-10)^2 = 1 + 2^-9 + 2^-20 needs hi hi, hi mid, mid hi AND mid mid."""
    v = 1.0 + 2.0 ** -10
    x = torch.zeros((n, cin, h, w))
    x[:, 5, 1::4, 2::4] = v
    wt = torch.zeros((cout, cin, 3, 3))
    wt[:, 5, 1, 1] = v
    ref = assert_exact_in_the_winograd_domain(x, wt, pad, 2.0 ** -22)
    assert set(ref.unique().tolist()) == {0.0, 1.0 + 2.0 ** -9 + 2.0 ** -20}
    return x, wt, ref


def case_integers(pad: int = 1, *, n: int = 5, cin: int = 48, cout: int = 128, h: int = 19, w: int = 13):
    """(iv) Dense small integers: activations in [-64, 63] (one in four non-zero), weights in [-20, 20]; accumulation across slices,
    positions and padding with sum |V| |U| bounded in the Winograd domain."""
    g = torch.Generator().manual_seed(400 + pad)
    x = torch.randint(-64, 64, (n, cin, h, w), generator=g).float() * (torch.rand((n, cin, h, w), generator=g) < 0.25).float()
    wt = torch.randint(-20, 21, (cout, cin, 3, 3), generator=g).float()
    return x, wt, assert_exact_in_the_winograd_domain(x, wt, pad, 0.25)


__all__ = ["ORDER", "case_integers", "case_isolated_activations", "case_isolated_powers_of_two", "case_mid_mid", "dropped_terms_bound",
           "emulate_conv", "input_tiles", "input_transform", "output_transform", "packed_index"]
