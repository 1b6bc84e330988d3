"""CPU emulation of conv3x3_wino_kernel's data flow (csrc/conv3x3_wino.hip), of conv3x3_wino42_kernel's (csrc/conv3x3_wino42.hip) and of
conv3x3_wino_bf16x3_kernel's (csrc/conv3x3_wino_bf16x3.hip): the packed-weight layout, the LDS images the DMAs build,
every lane's fragment addresses, the MFMA operand / result layout, the two-group output transform and the epilogue's pixel mapping --
index formula by index formula -- against torch's conv2d.  A developer check of the kernel's bookkeeping that needs no GPU
(`python scripts/wino_emulate.py`); the GPU parity tests are tests/test_engine.py::test_winograd_*."""
import numpy as np
import torch
import torch.nn.functional as F

OOB = None


def pack(w):  # wino_pack_kernel
    cout, cin = w.shape[:2]
    n_cs, n_cb = cin // 16, cout // 64
    out = np.zeros(16 * cin * cout, np.float32)
    G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
    for o in range(cout):
        for c in range(cin):
            U = G @ w[o, c].astype(np.float64) @ G.T
            cs, h8, hi, c4, cb, col = c >> 4, (c >> 3) & 1, (c >> 2) & 1, c & 3, o >> 6, o & 63
            for i in range(4):
                for j in range(4):
                    block = (((i * 4 + j) * n_cs + cs) * 2 + h8) * n_cb + cb
                    out[block * 512 + (hi * 64 + col) * 4 + c4] = np.float32(U[i, j])
    return out


def plan_windows(nb, ho, wo):  # wino_plan
    if ho <= 8 and wo <= 8:
        return None
    ty_, tx_ = (ho + 1) // 2, (wo + 1) // 2
    busy16 = ho * wo / (((ho + 15) // 16) * ((wo + 15) // 16) * 256)
    best, best_busy, bu = None, busy16, 0
    if busy16 >= 0.9:
        return None
    for wty in range(1, 9):
        for wtx in range(1, 17):
            wt = wty * wtx
            if wt > 64:
                continue
            wrow = (wtx + 1) * 9
            wimg = ((2 * wty + 2) * wrow + 15) // 16 * 16
            wx, wy = -(-tx_ // wtx), -(-ty_ // wty)
            for wg in range(64 // wt, max(0, 64 // wt - 3), -1):
                if wg * wimg > 2560 or wg > 16:
                    continue
                blocks = -(-nb * wx * wy // wg)
                busy = nb * ho * wo / (blocks * 256)
                units = wg * wimg
                if busy > best_busy + 0.02 or (best is not None and busy > best_busy - 1e-9 and units < bu):
                    best, best_busy, bu = dict(wg=wg, wty=wty, wtx=wtx, wrow=wrow, wimg=wimg, wins_x=wx, wins_y=wy), busy, units
    return best


def run_block(x, upk, geo, mt_id, cb, pad, ho, wo, tiles_x, tiles_per_image):
    n, h, w, cin = x.shape
    cout = upk.size // (16 * cin)
    RT = isinstance(geo, dict)
    if RT:
        G, TH, TW, PH, PWD, ROW, IMG = 0, 16, 16, 0, 0, geo["wrow"], 2560
        n_windows = n * geo["wins_x"] * geo["wins_y"]
    else:
        G, TH, TW, PH, PWD, ROW, IMG = geo
    NT = 512

    def px_unit(px):
        return (px >> 1) * 9 + (px & 1) * 4
    A_UNITS = ((1 if RT else G) * IMG + 63) // 64 * 64
    NA = (A_UNITS + NT - 1) // NT
    n_cs, n_cb = cin // 16, cout // 64
    pos_stride = n_cs * n_cb * 4096
    img = 0 if RT else (mt_id // tiles_per_image if G == 1 else mt_id * G)
    trem = mt_id - img * tiles_per_image if G == 1 else 0
    ty0, tx0 = (trem // tiles_x) * TH, (trem % tiles_x) * TW
    xf = x.reshape(-1)
    acc = np.zeros((8, 4, 2, 32, 32), np.float32)  # [wave][j][channel tile][row][col]
    for cs in range(n_cs):
        # ---- patch image
        abuf = np.zeros((A_UNITS, 4), np.float32)
        for r in range(NA):
            for tid in range(NT):
                un = NT * r + tid
                wave = tid >> 6
                if NT * r + wave * 64 >= A_UNITS:
                    continue  # dump
                if RT:
                    if NT * r >= geo["wg"] * geo["wimg"]:
                        continue
                    g, ug = divmod(un, geo["wimg"])
                    py, rem = divmod(ug, geo["wrow"])
                    pair, r9 = divmod(rem, 9)
                    px, chunk = 2 * pair + (r9 >> 2), (4 if r9 == 8 else r9 & 3)
                    win = mt_id * geo["wg"] + g
                    wi, wr = divmod(win, geo["wins_x"] * geo["wins_y"])
                    wy, wx = divmod(wr, geo["wins_x"])
                    iy, ix = wy * 2 * geo["wty"] - pad + py, wx * 2 * geo["wtx"] - pad + px
                    inside = (g < geo["wg"] and win < n_windows and py < 2 * geo["wty"] + 2 and px < 2 * geo["wtx"] + 2 and chunk < 4
                              and 0 <= iy < h and 0 <= ix < w)
                    if inside:
                        off = (((wi * h + iy) * w + ix) * cin * 4 + 16 * chunk + cs * 64) // 4
                        abuf[un] = xf[off:off + 4]
                    continue
                g, ug = divmod(un, IMG)
                py, rem = divmod(ug, ROW)
                pair, r9 = divmod(rem, 9)
                px, chunk = 2 * pair + (r9 >> 2), (4 if r9 == 8 else r9 & 3)
                iy, ix = ty0 - pad + py, tx0 - pad + px
                inside = g < G and img + g < n and py < PH and px < PWD and chunk < 4 and 0 <= iy < h and 0 <= ix < w
                if inside:
                    off = ((((img + g) * h + iy) * w + ix) * cin * 4 + 16 * chunk + cs * 64) // 4
                    abuf[un] = xf[off:off + 4]
        for h8 in range(2):
            s_step = 2 * cs + h8
            # ---- weight stage
            wst = np.zeros((2048, 4), np.float32)
            for q in range(4):
                soff = 4 * q * pos_stride + (s_step * n_cb + cb) * 2048
                for wave in range(8):
                    for lane in range(64):
                        voff = (wave & 1) * 1024 + lane * 16 + (wave >> 1) * pos_stride
                        src = (soff + voff) // 4
                        wst[q * 512 + wave * 64 + lane] = upk[src:src + 4]
            # ---- compute
            for wave in range(8):
                i, wm = wave >> 1, wave & 1
                ra = 0 if i == 0 else (2 if i == 2 else 1)
                rb = 2 if i == 0 else (2 if i == 1 else (1 if i == 2 else 3))
                sg = 1.0 if i == 1 else -1.0
                V = np.zeros((4, 64, 4), np.float32)
                Wv = np.zeros((4, 2, 64, 4), np.float32)
                for lane in range(64):
                    hi = lane >> 5
                    t = 32 * wm + (lane & 31)
                    if RT:
                        wt = geo["wty"] * geo["wtx"]
                        tv = t if t < geo["wg"] * wt else 0
                        g_, rr = divmod(tv, wt)
                        tyy, txx = divmod(rr, geo["wtx"])
                        fa = g_ * geo["wimg"] + 2 * tyy * geo["wrow"] + txx * 9 + hi
                    elif G == 1:
                        fa = 2 * (t >> 3) * ROW + (t & 7) * 9 + hi
                    else:
                        fa = (t >> 4) * IMG + 2 * ((t >> 2) & 3) * ROW + (t & 3) * 9 + hi
                    fa += 2 * h8
                    fb = i * 4 * 128 + hi * 64 + (lane & 31)
                    R = np.zeros((4, 4), np.float32)
                    for c in range(4):
                        R[c] = (abuf[fa + rb * ROW + px_unit(c)] * np.float32(sg) + abuf[fa + ra * ROW + px_unit(c)]).astype(np.float32)
                    V[0, lane] = R[0] - R[2]
                    V[1, lane] = R[1] + R[2]
                    V[2, lane] = R[2] - R[1]
                    V[3, lane] = R[1] - R[3]
                    for j in range(4):
                        for ct in range(2):
                            Wv[j, ct, lane] = wst[fb + j * 128 + ct * 32]
                for j in range(4):
                    for ct in range(2):
                        for k in range(4):
                            A = np.stack([V[j, :32, k], V[j, 32:, k]], axis=1)          # [row][kidx]
                            B = np.stack([Wv[j, ct, :32, k], Wv[j, ct, 32:, k]], axis=0)  # [kidx][col]
                            acc[wave, j, ct] += (A @ B).astype(np.float32)
    # ---- output transform + tiles (two rounds)
    tiles = np.zeros((2, 256, 64), np.float32)

    def to_tile(wave, a, add, neg):
        i, wm = wave >> 1, wave & 1
        m = acc[wave]
        z = [[m[0, ct] + m[1, ct] + m[2, ct] for ct in range(2)], [m[1, ct] - m[2, ct] - m[3, ct] for ct in range(2)]]
        for row in range(32):
            tt = 32 * wm + row
            if RT:
                m00, astep = 4 * tt, 2
            else:
                m00 = 2 * (tt >> 3) * TW + 2 * (tt & 7) if G == 1 else (tt >> 4) * TH * TW + 2 * ((tt >> 2) & 3) * TW + 2 * (tt & 3)
                astep = TW
            for bb in range(2):
                for ct in range(2):
                    v = -z[bb][ct][row] if neg else z[bb][ct][row]
                    dst = tiles[i >> 1, m00 + a * astep + bb, ct * 32:ct * 32 + 32]
                    dst[:] = dst + v if add else v

    for wave in range(8):
        to_tile(wave, (wave >> 1) & 1, False, (wave >> 1) == 3)
    for wave in range(8):
        if wave >> 1 == 1:
            to_tile(wave, 0, True, False)
        if wave >> 1 == 2:
            to_tile(wave, 1, True, True)
    tile = tiles[0] + tiles[1]
    out = {}
    for row in range(256):
        if RT:
            tt, wt = row >> 2, geo["wty"] * geo["wtx"]
            g_, rr = divmod(tt, wt)
            tyy, txx = divmod(rr, geo["wtx"])
            win = mt_id * geo["wg"] + g_
            wi, wr = divmod(win, geo["wins_x"] * geo["wins_y"])
            wy, wx = divmod(wr, geo["wins_x"])
            oy, ox = 2 * (wy * geo["wty"] + tyy) + ((row >> 1) & 1), 2 * (wx * geo["wtx"] + txx) + (row & 1)
            if tt < geo["wg"] * wt and win < n_windows and oy < ho and ox < wo:
                out[(wi, oy, ox)] = tile[row]
            continue
        g, rg = divmod(row, TH * TW)
        oy, ox = ty0 + rg // TW, tx0 + rg % TW
        if oy < ho and ox < wo and img + g < n:
            out[(img + g, oy, ox)] = tile[row]
    return out


def check(n, hw, cin, cout, pad, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, hw, hw, cin)).astype(np.float32)
    wgt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    ho = wo = hw + 2 * pad - 2
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wgt), padding=pad).permute(0, 2, 3, 1).numpy()
    upk = pack(wgt)
    small = ho <= 8 and wo <= 8
    win = plan_windows(n, ho, wo)
    geo = win if win is not None else ((4, 8, 8, 10, 10, 50, 512) if small else (1, 16, 16, 18, 18, 84, 18 * 84))
    tiles_y = 1 if small else (ho + 15) // 16
    tiles_x = 1 if small else (wo + 15) // 16
    tiles = (n + 3) // 4 if small else n * tiles_y * tiles_x
    if win is not None:
        tiles = -(-n * win["wins_x"] * win["wins_y"] // win["wg"])
        print("   windows:", win)
    got = np.full_like(ref, np.nan)
    for mt in range(tiles):
        for cb in range(cout // 64):
            for (b, oy, ox), v in run_block(x, upk, geo, mt, cb, pad, ho, wo, tiles_x, tiles_y * tiles_x).items():
                got[b, oy, ox, cb * 64:cb * 64 + 64] = v
    assert not np.isnan(got).any(), "outputs not covered"
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"n={n} hw={hw} cin={cin} cout={cout} pad={pad}: rel err {err:.2e}")
    assert err < 2e-5, err


def bank_check():
    """Every service group of a ds_read_b128 (16 lanes) must hit 16 different 16-byte bank groups, for both geometries."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    for G, ROW, IMG in ((1, 84, 18 * 84), (4, 50, 512)):
        for wm in range(2):
            for grp in groups:
                units = []
                for lane in grp:
                    t = 32 * wm + lane
                    fa = 2 * (t >> 3) * ROW + (t & 7) * 9 if G == 1 else (t >> 4) * IMG + 2 * ((t >> 2) & 3) * ROW + (t & 3) * 9
                    units.append(fa % 16)
                assert len(set(units)) == 16, (G, wm, grp, units)
    print("patch reads: conflict-free")


# ---- F(4x2, 3x3): conv3x3_wino42_kernel ------------------------------------------------------------------------------------------
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]])
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]])
W16_42, W8_42 = (1, 16, 16, 18, 18, 82, 18 * 82), (4, 8, 8, 10, 10, 48, 484)  # (G, TH, TW, PH, PWD, ROW, IMG)


def pack42(w):  # wino42_pack_kernel: [pos 24 = 4 i + j][cin/16][h8 2][cout/64] blocks of [hi 2][64 cout][4 channels]
    cout, cin = w.shape[:2]
    n_cs, n_cb = cin // 16, cout // 64
    U = np.einsum("ir,ocrs,js->ocij", G4, w.astype(np.float64), G2).astype(np.float32)  # [cout][cin][6][4]
    out = np.zeros(24 * cin * cout, np.float32)
    o, c = np.meshgrid(np.arange(cout), np.arange(cin), indexing="ij")
    cs, h8, hi, c4, cb, col = c >> 4, (c >> 3) & 1, (c >> 2) & 1, c & 3, o >> 6, o & 63
    for i in range(6):
        for j in range(4):
            block = (((i * 4 + j) * n_cs + cs) * 2 + h8) * n_cb + cb
            out[block * 512 + (hi * 64 + col) * 4 + c4] = U[:, :, i, j]
    return out


def run_block42(x, upk, geo, mt_id, cb, pad, ho, wo, tiles_x, tiles_per_image):
    n, h, w, cin = x.shape
    cout = upk.size // (24 * cin)
    G, TH, TW, PH, PWD, ROW, IMG = geo
    NT = 512

    def px_unit(px):
        return (px >> 1) * 9 + (px & 1) * 4
    A_UNITS = (G * IMG + 63) // 64 * 64
    NA = (A_UNITS + NT - 1) // NT
    n_cs, n_cb = cin // 16, cout // 64
    pos_stride = n_cs * n_cb * 4096
    img = mt_id // tiles_per_image if G == 1 else mt_id * G
    trem = mt_id - img * tiles_per_image if G == 1 else 0
    ty0, tx0 = (trem // tiles_x) * TH, (trem % tiles_x) * TW
    xf = x.reshape(-1)
    acc = np.zeros((8, 3, 2, 32, 32), np.float32)  # [wave][ii][channel tile][row = tile][col]
    f32 = np.float32
    for cs in range(n_cs):
        abuf = np.zeros((A_UNITS, 4), np.float32)  # patch image (make_cen, dma_a)
        for r in range(NA):
            for tid in range(NT):
                un = NT * r + tid
                if NT * r + (tid >> 6) * 64 >= A_UNITS:
                    continue  # dump
                g, ug = divmod(un, IMG)
                py, rem = divmod(ug, ROW)
                pair, r9 = divmod(rem, 9)
                px, chunk = 2 * pair + (r9 >> 2), (4 if r9 == 8 else r9 & 3)
                iy, ix = ty0 - pad + py, tx0 - pad + px
                if g < G and img + g < n and py < PH and px < PWD and chunk < 4 and 0 <= iy < h and 0 <= ix < w:
                    off = ((((img + g) * h + iy) * w + ix) * cin * 4 + 16 * chunk + cs * 64) // 4
                    abuf[un] = xf[off:off + 4]
        for h8 in range(2):
            s_step = 2 * cs + h8
            wst = np.zeros((3072, 4), np.float32)  # weight stage (dma_w: six rounds)
            for q in range(6):
                soff = 4 * q * pos_stride + (s_step * n_cb + cb) * 2048
                for wave in range(8):
                    for lane in range(64):
                        src = (soff + (wave & 1) * 1024 + lane * 16 + (wave >> 1) * pos_stride) // 4
                        wst[q * 512 + wave * 64 + lane] = upk[src:src + 4]
            for wave in range(8):
                jcol, hrow = wave & 3, wave >> 2
                ca, cbc = [(0, 2), (1, 2), (2, 1), (1, 3)][jcol]
                V = np.zeros((3, 64, 4), np.float32)
                Wv = np.zeros((3, 2, 64, 4), np.float32)
                for lane in range(64):
                    hi, t = lane >> 5, lane & 31
                    fa = 4 * (t >> 3) * ROW + (t & 7) * 9 + hi if G == 1 else (t >> 3) * IMG + 4 * ((t >> 2) & 1) * ROW + (t & 3) * 9 + hi
                    fa += 2 * h8
                    fa_a, fa_b = fa + hrow * ROW + px_unit(ca), fa + hrow * ROW + px_unit(cbc)
                    T = [abuf[fa_a + r * ROW] + abuf[fa_b + r * ROW] if jcol == 1 else abuf[fa_a + r * ROW] - abuf[fa_b + r * ROW]
                         for r in range(5)]
                    T = [t_.astype(f32) for t_ in T]
                    edge = f32(4) * T[0] + (f32(-5) * T[2] + T[4])  # (fma chains: float32 rounding up to the fused steps)
                    if hrow == 0:
                        a, b = f32(-4) * T[2] + T[4], f32(-4) * T[1] + T[3]
                        V[:, lane] = [edge, a + b, a - b]
                    else:
                        c, g_ = T[3] - T[1], T[2] - T[0]
                        V[:, lane] = [f32(2) * g_ + c, f32(-2) * g_ + c, edge]
                    fb = (12 * hrow + jcol) * 128 + hi * 64 + (lane & 31)
                    for ii in range(3):
                        for ct in range(2):
                            Wv[ii, ct, lane] = wst[fb + ii * 512 + ct * 32]
                for ii in range(3):
                    for ct in range(2):
                        for k in range(4):
                            A = np.stack([V[ii, :32, k], V[ii, 32:, k]], axis=1)
                            B = np.stack([Wv[ii, ct, :32, k], Wv[ii, ct, 32:, k]], axis=0)
                            acc[wave, ii, ct] += (A @ B).astype(np.float32)
    # ---- output transform: A4^T over the wave's positions, the row halves lane to lane, A2 over the waves j
    P = np.zeros((8, 4, 2, 32, 32), np.float32)  # [wave][a][ct]
    for wave in range(8):
        m = acc[wave]
        if wave >> 2 == 0:
            s_, dd = m[1] + m[2], m[1] - m[2]
            P[wave] = [m[0] + s_, dd, s_, dd]
        else:
            s_, dd = m[0] + m[1], (m[0] - m[1]) * 2
            P[wave] = [s_, dd, s_ * 4, dd * 4 + m[2]]
    Q = P[:4] + P[4:]  # [j][a][ct]
    Y = [(Q[0] + Q[1]) + Q[2], Q[1] + (-Q[3] - Q[2])]  # [b][a][ct]
    tile = np.zeros((256, 64), np.float32)
    for e in range(16):
        for hi in range(2):
            tt = (e & 3) + 8 * (e >> 2) + 4 * hi
            m00 = 4 * (tt >> 3) * TW + 2 * (tt & 7) if G == 1 else (tt >> 3) * TH * TW + 4 * ((tt >> 2) & 1) * TW + 2 * (tt & 3)
            for a in range(4):
                for b in range(2):
                    for ct in range(2):
                        tile[m00 + a * TW + b, ct * 32:ct * 32 + 32] = Y[b][a][ct][tt]
    out = {}
    for row in range(256):
        g, rg = divmod(row, TH * TW)
        oy, ox = ty0 + rg // TW, tx0 + rg % TW
        if oy < ho and ox < wo and img + g < n:
            out[(img + g, oy, ox)] = tile[row]
    return out


def check42(n, hw, cin, cout, pad=1, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, hw, hw, cin)).astype(np.float32)
    wgt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    ho = wo = hw + 2 * pad - 2
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wgt), padding=pad).permute(0, 2, 3, 1).numpy()
    upk = pack42(wgt)
    small = ho <= 8 and wo <= 8
    geo = W8_42 if small else W16_42
    tiles_y = 1 if small else (ho + 15) // 16
    tiles_x = 1 if small else (wo + 15) // 16
    tiles = (n + 3) // 4 if small else n * tiles_y * tiles_x
    got = np.full_like(ref, np.nan)
    for mt in range(tiles):
        for cb in range(cout // 64):
            for (b, oy, ox), v in run_block42(x, upk, geo, mt, cb, pad, ho, wo, tiles_x, tiles_y * tiles_x).items():
                got[b, oy, ox, cb * 64:cb * 64 + 64] = v
    assert not np.isnan(got).any(), "outputs not covered"
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"F(4x2) n={n} hw={hw} cin={cin} cout={cout} pad={pad}: rel err {err:.2e}")
    assert err < 1e-5, err


def bank_check42():
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    for G, _, _, _, _, ROW, IMG in (W16_42, W8_42):
        for grp in groups:
            units = [(4 * (t >> 3) * ROW + (t & 7) * 9 if G == 1 else (t >> 3) * IMG + 4 * ((t >> 2) & 1) * ROW + (t & 3) * 9) % 16
                     for t in grp]
            assert len(set(units)) == 16, (G, grp, units)
    print("F(4x2) patch reads: conflict-free")


# ---- split-operand F(2x2, 3x3) on the bf16 matrix cores: conv3x3_wino_bf16x3_kernel -------------------------------------------------
def bf16_parts(v):
    """float32 array -> (hi, mid, lo) float32 arrays holding bf16 values (round to nearest even; split_pair / split_stem_weights)."""
    def rne(a):
        u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
        return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    hi = rne(v)
    r1 = (v - hi).astype(np.float32)
    mid = rne(r1)
    return hi, mid, rne((r1 - mid).astype(np.float32))


def pack_split(w):  # fused.wino_weights_f32 + split_stem_weights + wino_pack_bf16x3_kernel
    cout, cin = w.shape[:2]
    n_cb = cout // 64
    U = np.einsum("ir,ocrs,js->ocij", G2, w.astype(np.float64), G2).astype(np.float32)
    parts = np.stack(bf16_parts(U))  # [3][cout][cin][4][4]
    out = np.zeros(48 * cin * cout, np.float32)  # (bf16 values; element index = the kernel's bf16 index)
    idx = np.arange(out.size)
    e, col, q, r = idx & 7, (idx >> 3) & 63, (idx >> 9) & 1, idx >> 10
    p, r = r % 3, r // 3
    pos8, r = r & 7, r >> 3
    cb, r = r % n_cb, r // n_cb
    jh, cs = r & 1, r >> 1
    out[idx] = parts[p, 64 * cb + col, 16 * cs + 8 * q + e, pos8 >> 1, 2 * jh + (pos8 & 1)]
    return out


def run_block_split(x, upk, mt_id, cb, pad, ho, wo, tiles_x, tiles_per_image):
    n, h, w, cin = x.shape
    cout = upk.size // (48 * cin)
    TH, TW, PH, PWD, ROW, IMG, NT = 16, 16, 18, 18, 84, 18 * 84, 512
    A_UNITS, W_UNITS = 1536, 3072  # patch buffer, weight stage (16-byte units)

    def px_unit(px):
        return (px >> 1) * 9 + (px & 1) * 4
    n_cs, n_cb = cin // 16, cout // 64
    img = mt_id // tiles_per_image
    trem = mt_id - img * tiles_per_image
    ty0, tx0 = (trem // tiles_x) * TH, (trem % tiles_x) * TW
    xf = x.reshape(-1)
    acc = np.zeros((8, 4, 2, 32, 32), np.float32)
    order = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # (V part, U part): lo hi, hi lo, mid mid, mid hi, hi mid, hi hi
    for cs in range(n_cs):
        abuf = np.zeros((A_UNITS, 4), np.float32)  # make_cen / dma_a: three whole rounds
        for un in range(A_UNITS):
            py, rem = divmod(un, ROW)
            pair, r9 = divmod(rem, 9)
            px, chunk = 2 * pair + (r9 >> 2), (4 if r9 == 8 else r9 & 3)
            iy, ix = ty0 - pad + py, tx0 - pad + px
            if img < n and py < PH and px < PWD and chunk < 4 and 0 <= iy < h and 0 <= ix < w:
                off = (((img * h + iy) * w + ix) * cin * 4 + 16 * chunk + cs * 64) // 4
                abuf[un] = xf[off:off + 4]
        R = np.zeros((8, 64, 4, 8), np.float32)  # load_r: [wave][lane][patch column][channel 8 hi + e]
        for wave in range(8):
            i, wm = wave >> 1, wave & 1
            ra = 0 if i == 0 else (2 if i == 2 else 1)
            rb = 2 if i < 2 else (1 if i == 2 else 3)
            for lane in range(64):
                hi, t = lane >> 5, 32 * wm + (lane & 31)
                fa = 2 * (t >> 3) * ROW + (t & 7) * 9 + 2 * hi
                for c in range(4):
                    a = np.concatenate([abuf[fa + ra * ROW + px_unit(c) + q] for q in range(2)])
                    b = np.concatenate([abuf[fa + rb * ROW + px_unit(c) + q] for q in range(2)])
                    R[wave, lane, c] = a + b if i == 1 else a - b
        for jh in range(2):
            s_step = 2 * cs + jh
            wst = np.zeros((W_UNITS, 8), np.float32)  # dma_w: six rounds, a wave's KB each; a unit = 8 bf16
            for q in range(6):
                for wave in range(8):
                    for lane in range(64):
                        src = ((s_step * n_cb + cb) * 49152 + q * 8192 + wave * 1024 + lane * 16) // 2
                        wst[q * 512 + wave * 64 + lane] = upk[src:src + 8]
            for wave in range(8):
                i = wave >> 1
                for jl in range(2):
                    j = 2 * jh + jl
                    r_ = R[wave]
                    V = [r_[:, 0] - r_[:, 2], r_[:, 1] + r_[:, 2], r_[:, 2] - r_[:, 1], r_[:, 1] - r_[:, 3]][j].astype(np.float32)  # [lane][8]
                    vp = bf16_parts(V)
                    for ct in range(2):
                        up = []
                        for p in range(3):  # plane p of position (i, jl): [k-chunk hi][column]
                            frag = np.stack([wst[((i * 2 + jl) * 3 + p) * 128 + (lane >> 5) * 64 + ct * 32 + (lane & 31)] for lane in range(64)])
                            up.append(np.concatenate([frag[:32], frag[32:]], axis=1).T)  # [k 16][col 32]
                        for pv, pu in order:
                            A = np.concatenate([vp[pv][:32], vp[pv][32:]], axis=1)  # [row 32][k 16]: lane >> 5 holds k = 8 (lane >> 5) ..
                            acc[wave, j, ct] = (acc[wave, j, ct].astype(np.float64) + A.astype(np.float64) @ up[pu].astype(np.float64)).astype(np.float32)
    # ---- epilogue of conv3x3_wino_kernel (W16)
    tile = np.zeros((256, 64), np.float32)
    for wm in range(2):
        z = [[[acc[2 * i + wm][0, ct] + acc[2 * i + wm][1, ct] + acc[2 * i + wm][2, ct] for ct in range(2)],
              [acc[2 * i + wm][1, ct] - acc[2 * i + wm][2, ct] - acc[2 * i + wm][3, ct] for ct in range(2)]] for i in range(4)]
        for b in range(2):
            for ct in range(2):
                y0 = (z[0][b][ct] + z[1][b][ct]) + z[2][b][ct]
                y1 = z[1][b][ct] + (-z[3][b][ct] - z[2][b][ct])
                for row in range(32):
                    tt = 32 * wm + row
                    m00 = 2 * (tt >> 3) * TW + 2 * (tt & 7)
                    tile[m00 + b, ct * 32:ct * 32 + 32] = y0[row]
                    tile[m00 + TW + b, ct * 32:ct * 32 + 32] = y1[row]
    out = {}
    for row in range(256):
        oy, ox = ty0 + row // TW, tx0 + row % TW
        if oy < ho and ox < wo and img < n:
            out[(img, oy, ox)] = tile[row]
    return out


def check_split(n, hw, cin, cout, pad=1, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, hw, hw, cin)).astype(np.float32)
    wgt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    ho = wo = hw + 2 * pad - 2
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wgt), padding=pad).permute(0, 2, 3, 1).numpy()
    upk = pack_split(wgt)
    tiles_y, tiles_x = (ho + 15) // 16, (wo + 15) // 16
    got = np.full_like(ref, np.nan)
    for mt in range(n * tiles_y * tiles_x):
        for cb in range(cout // 64):
            for (b, oy, ox), v in run_block_split(x, upk, mt, cb, pad, ho, wo, tiles_x, tiles_y * tiles_x).items():
                got[b, oy, ox, cb * 64:cb * 64 + 64] = v
    assert not np.isnan(got).any(), "outputs not covered"
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"split F(2x2) n={n} hw={hw} cin={cin} cout={cout} pad={pad}: rel err {err:.2e}")
    assert err < 1e-5, err


def bank_check_split():
    """The split form's reads.  Patch: units 2 hi + q of a pixel -- the same offset for all lanes of a service group (hi = lane >> 5), so
    bank_check()'s W16 argument holds; checked here with the offset.  Weights: the 32 lanes of a half-wave read 32 consecutive units."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    for wm in range(2):
        for hi in range(2):
            for q in range(2):
                for grp in groups:
                    units = [(2 * ((32 * wm + ln) >> 3) * 84 + ((32 * wm + ln) & 7) * 9 + 2 * hi + q) % 16 for ln in grp]
                    assert len(set(units)) == 16, (wm, hi, q, grp, units)
    for grp in groups:
        assert len({ln % 16 for ln in grp}) == 16  # (+ a multiple of 16 units per position, plane, k-chunk and channel tile)
    # LDS map [patch 0][stage 0][patch 1][stage 1]; the epilogue's 64 KB from patch 1 on; every read inside its buffer
    a_bytes, w_stage = 1536 * 16, 8 * 3 * 2048
    assert 2 * a_bytes + 2 * w_stage == 147456 <= 160 * 1024 and a_bytes + w_stage + 65536 <= 147456
    assert 2 * 7 * 84 + 7 * 9 + 2 + 3 * 84 + 13 + 1 < 1536 and (3 * 2 + 1) * 3 * 128 + 256 + 64 + 32 + 31 < 3072
    print("split F(2x2) reads: conflict-free, inside their buffers")


if __name__ == "__main__":
    bank_check()
    if "--windows-only" not in __import__("sys").argv:
        check(1, 16, 16, 64, 1)
        check(5, 7, 32, 64, 1)       # W8 geometry, odd map, a partial block of images
    check(8, 14, 16, 64, 1)      # window geometry: eight windows of 1 x 7 tiles, blocks across images, a partial last block
    check(3, 28, 16, 64, 1)      # window geometry: 3 windows of 3 x 7 tiles
    if "--all" in __import__("sys").argv:
        check(1, 20, 16, 128, 1)     # partial blocks, two channel blocks
        check(2, 12, 16, 64, 0)      # valid convolution
    bank_check42()
    check42(1, 16, 32, 64)           # F(4x2), one 16 x 16 block, two 16-channel slices
    check42(5, 8, 16, 64)            # F(4x2), four-image blocks, a partial block of images
    check42(1, 32, 16, 128)          # F(4x2), four blocks, two channel blocks
    print("emulation ok")
    bank_check_split()
    check_split(1, 16, 32, 64)       # split F(2x2): one full block, two slices
    check_split(2, 19, 16, 128, 0)   # partial blocks, two channel blocks, valid convolution
    check_split(3, 7, 48, 64, 2)     # a small map in a 16 x 16 block, an odd slice count, padding 2
