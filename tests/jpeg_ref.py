"""NumPy restatement of K12 (include/vaa.h: vaa_jpeg_roundtrip), integers only (int64 throughout, no floats), written from the header and
shaped differently from the kernel (whole planes at a time, no workgroups). Next to it an IDEALISED codec: the same tables, subsampling and
upsampling geometry with exact real arithmetic (float64 DCT, the real colour matrices, one rounding per stage). The idealised codec is a
yardstick only: how far a codec with no fixed-point structure at all lands from a real one.

`perturb` switches one step of the integer pipeline to a plausible wrong form (the host test proves that the comparison against a real codec
sees each of them)."""
import numpy as np

# Annex K of ITU-T T.81, natural (row-major) order
BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64)


def qtables(quality: int) -> np.ndarray:
    """[2,64] uint16: the Annex K tables scaled by libjpeg's quality rule, clamped to 1..255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be an integer in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    out = np.stack([(BASE_LUMA * s + 50) // 100, (BASE_CHROMA * s + 50) // 100])
    return np.clip(out, 1, 255).astype(np.uint16)


def _fix(x, bits):
    return int(x * (1 << bits) + 0.5)


# 16 fractional bits (colour), 13 (DCT)
_CY = (_fix(0.29900, 16), _fix(0.58700, 16), _fix(0.11400, 16))
_CB = (_fix(0.16874, 16), _fix(0.33126, 16), _fix(0.50000, 16))
_CR = (_fix(0.50000, 16), _fix(0.41869, 16), _fix(0.08131, 16))
_R_CR, _B_CB, _G_CR, _G_CB = _fix(1.40200, 16), _fix(1.77200, 16), _fix(0.71414, 16), _fix(0.34414, 16)
_HALF = 1 << 15
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_CY[0] * r + _CY[1] * g + _CY[2] * b + _HALF) >> 16
    cb = (-_CB[0] * r - _CB[1] * g + _CB[2] * b + (128 << 16) + _HALF - 1) >> 16
    cr = (_CR[0] * r - _CR[1] * g - _CR[2] * b + (128 << 16) + _HALF - 1) >> 16
    return y, cb, cr


def ycc_to_rgb(y, cb, cr):
    cb = cb - 128
    cr = cr - 128
    r = y + ((_R_CR * cr + _HALF) >> 16)
    g = y + ((-_G_CB * cb + _HALF - _G_CR * cr) >> 16)
    b = y + ((_B_CB * cb + _HALF) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _pad_edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def downsample_h2v2(c, MH, MW, bias=(1, 2)):
    """Full-resolution chroma [H,W] -> [MH/2, MW/2]: columns replicated to MW, rows to the next even count, 2x2 sums with the alternating
    bias, then the LAST SUBSAMPLED ROW replicated down to MH/2 (a baseline encoder pads after the subsampling, vertically)."""
    H, W = c.shape
    c = _pad_edge(c, H + (H & 1), MW)
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    b = np.where(np.arange(MW // 2) % 2 == 0, bias[0], bias[1])
    return _pad_edge((s + b[None, :]) >> 2, MH // 2, MW // 2)


def _fdct_1d(d, first):
    """Eight-point forward transform along the last axis. first: the row pass (outputs scaled up by 4); else the column pass."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _idct_1d(d, first):
    """Eight-point inverse transform along the last axis. first: the column pass (descale by 11); else the row pass (descale by 18)."""
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * F_0_541
    t2, t3 = z1 - d[6] * F_1_847, z1 + d[2] * F_0_765
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 13 - 2 if first else 13 + 2 + 3
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in o], axis=-1)


def _blocks(p):
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [by, bx, row, col]


def _unblocks(b):
    nby, nbx = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nby * 8, nbx * 8)


def block_roundtrip(plane, qt, truncate=False):
    """plane: [h,w] samples 0..255 (h, w multiples of 8); qt: [64] -> the decoded samples 0..255."""
    q = qt.astype(np.int64).reshape(8, 8)
    b = _blocks(plane.astype(np.int64) - 128)
    c = _fdct_1d(b, True)                                            # rows
    c = _fdct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)         # columns: 8 x the DCT
    mag = np.abs(c) if truncate else np.abs(c) + 4 * q
    k = np.sign(c) * (mag // (8 * q))                                # half away from zero
    d = k * q
    w = _idct_1d(d.swapaxes(-1, -2), True).swapaxes(-1, -2)          # columns
    o = _idct_1d(w, False)                                           # rows
    return _unblocks(np.clip(o + 128, 0, 255))


def upsample_h2v2_fancy(c, nearest=False):
    """[ch,cw] -> [2ch,2cw]: the triangle filter, 3:1 vertically then horizontally, edges replicated."""
    ch, cw = c.shape
    if nearest:
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    up = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * ch, 2 * cw), dtype=np.int64)
    for v in (0, 1):
        s = 3 * c + up[v]                                            # the column sums of output row 2r + v
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * s + left + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def roundtrip(frame, qt, rot180=False, perturb=None):
    """frame [H,W,3] uint8, qt [2,64] -> [H,W,3] uint8: include/vaa.h's vaa_jpeg_roundtrip for one frame."""
    frame = np.asarray(frame)
    if rot180:
        frame = frame[::-1, ::-1]
    qt = np.asarray(qt).astype(np.int64)
    if perturb == "swap_tables":
        qt = qt[::-1]
    H, W = frame.shape[:2]
    MH, MW = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    y, cb, cr = rgb_to_ycc(frame)
    bias = (2, 1) if perturb == "bias" else (1, 2)
    trunc = perturb == "truncate"
    yd = block_roundtrip(_pad_edge(y, MH, MW), qt[0], trunc)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    planes = []
    for c in (cb, cr):
        d = block_roundtrip(downsample_h2v2(c, MH, MW, bias), qt[1], trunc)
        planes.append(upsample_h2v2_fancy(d[:ch, :cw], nearest=perturb == "nearest")[:H, :W])
    return ycc_to_rgb(yd[:H, :W], planes[0], planes[1])


# ---------------------------------------------------------------- the idealised yardstick (float64; not a statement of anything)
_DCT = np.array([[(np.sqrt(0.125) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16) for n in range(8)] for k in range(8)])


def _ideal_plane(p, qt):
    q = qt.astype(np.float64).reshape(8, 8)
    b = _blocks(p.astype(np.float64) - 128.0)
    c = _DCT @ b @ _DCT.T
    k = np.sign(c) * np.floor(np.abs(c) / q + 0.5)
    o = _DCT.T @ (k * q) @ _DCT
    return _unblocks(np.clip(np.floor(o + 128.5), 0, 255))


def ideal_roundtrip(frame, qt, rot180=False):
    frame = np.asarray(frame)
    if rot180:
        frame = frame[::-1, ::-1]
    qt = np.asarray(qt)
    H, W = frame.shape[:2]
    MH, MW = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    f = frame.astype(np.float64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    rnd = lambda v: np.clip(np.floor(v + 0.5), 0, 255)
    y = rnd(0.299 * r + 0.587 * g + 0.114 * b)
    cb = rnd(-0.168735892 * r - 0.331264108 * g + 0.5 * b + 128)
    cr = rnd(0.5 * r - 0.418687589 * g - 0.081312411 * b + 128)
    yd = _ideal_plane(_pad_edge(y, MH, MW), qt[0])[:H, :W]
    ch, cw = (H + 1) // 2, (W + 1) // 2
    up = []
    for c in (cb, cr):
        c = _pad_edge(c, H + (H & 1), MW)
        s = _pad_edge(rnd((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]) / 4.0 - 1e-9), MH // 2, MW // 2)
        d = _ideal_plane(s, qt[1])[:ch, :cw]
        dv = np.empty((2 * ch, cw))
        dv[0::2] = 0.75 * d + 0.25 * np.concatenate([d[:1], d[:-1]])
        dv[1::2] = 0.75 * d + 0.25 * np.concatenate([d[1:], d[-1:]])
        dh = np.empty((2 * ch, 2 * cw))
        dh[:, 0::2] = 0.75 * dv + 0.25 * np.concatenate([dv[:, :1], dv[:, :-1]], axis=1)
        dh[:, 1::2] = 0.75 * dv + 0.25 * np.concatenate([dv[:, 1:], dv[:, -1:]], axis=1)
        up.append(rnd(dh)[:H, :W])
    cb, cr = up[0] - 128, up[1] - 128
    out = np.stack([yd + 1.402 * cr, yd - 0.344136286 * cb - 0.714136286 * cr, yd + 1.772 * cb], axis=-1)
    return rnd(out).astype(np.uint8)


def stats(a, b):
    """(share of bytes that differ, share that differ by more than 1, the largest difference) of two uint8 arrays."""
    d = np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))
    return float((d > 0).mean()), float((d > 1).mean()), int(d.max())


# ---------------------------------------------------------------- the recorded codec (tests/golden/jpeg_pillow.npz), shared by the test files
_GOLDEN = {}


def golden():
    """{"z": the fixture's arrays, "cases": [(frame name, quality)], "ref": {(name, quality): roundtrip(frame, recorded tables)}}: loaded and
    computed once per process and left unchanged."""
    import os

    if not _GOLDEN:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_pillow.npz")) as z:
            _GOLDEN["z"] = {k: z[k] for k in z.files}
        z = _GOLDEN["z"]
        _GOLDEN["cases"] = [(str(n), int(q)) for q in z["qualities"] for n in z["names"]]
        _GOLDEN["ref"] = {(n, q): roundtrip(z["in_" + n], z["qt_q%d" % q]) for n, q in _GOLDEN["cases"]}
    return _GOLDEN
