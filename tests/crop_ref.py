"""References of K9 (include/vaa.h: vaa_crop_resize_fwd / _bwd), shared by test_crop_host.py and test_gpu_crop.py. Plain numpy; calls no HIP code.

  taps32      the contract's per-axis expressions with EVERY operation on np.float32 (one rounding per operation, no FMA): t, b, l per output index.
  fwd32       the forward restated operation for operation in np.float32 -> bf16 bits: what the kernel must reproduce byte for byte.
  axis64      the fp64 tap matrix of one axis, W[i, r] = [t(i) == r](1 - l(i)) + [b(i) == r] l(i), with t, b and the fraction l taken as the
              fp32 values the contract computes (the geometry is part of the contract; everything after it is fp64).
  fwd64       Wy X Wx^T per plane;   bwd64   the explicit transpose Wy^T G Wx, with a bound per element.

BOUND of the adjoint (u = 2^-24). For source element (r, j), with A = Wy^T |G| Wx = sum |w g| over its taps:
    the kernel's chain per element is:  fl(1 - lx) (1), fl(wx * g) (1) and the running fp32 sum over n_x <= 6 touching columns (n_x);
    fl(1 - ly) (1), fl(wy * h) (1) and the running sum over n_y <= 6 touching rows (n_y): k = 4 + 6 + 6 = 16 factors (1 + d), |d| <= u, first order
    (the weights' own add [t==r](1-l) + [b==r] l has a zero term and is exact), so the fp32 value is within 16 u A of the fp64 one;
    the one rounding to bf16 adds half a bf16 ulp, taken at |value| + 16 u A (the binade the rounded fp32 value can lie in).
  An element that no output touches has A = 0 and value 0: bound 0, it must come out exactly 0.
"""
import numpy as np

N = 224
U = 2.0 ** -24
K_OPS = 16
f32 = np.float32


def center_box(scale=0.9):
    """K7's box of an area share, in fp32 as vaa_eval_preprocess computes it."""
    s = np.minimum(np.maximum(np.sqrt(f32(scale)), f32(0.0)), f32(1.0))
    y1 = (f32(1.0) - s) / f32(2.0)
    y2 = y1 + s
    return np.array([y1, y1, y2, y2], f32)


def taps32(lo, hi):
    """(t, b int64 [224], l fp32 [224], in fp32 [224]) of one axis of a box [lo, hi]."""
    lo, hi = f32(lo), f32(hi)
    org = lo * f32(N - 1)
    scale = ((hi - lo) * f32(N - 1)) / f32(N - 1)
    i = np.arange(N, dtype=f32)
    c = np.minimum(np.maximum(org + i * scale, f32(0.0)), f32(N - 1))
    assert c.dtype == f32
    t = np.floor(c)
    return t.astype(np.int64), np.ceil(c).astype(np.int64), (c - t).astype(f32), c


def bf16_bits(v):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.asarray(v, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(f32)


def fwd32(x_bits, boxes, fault=None):
    """x_bits uint16 [B,6,224,224], boxes [B,4] {y1, x1, y2, x2} -> (bf16 bits, fp32 values before the rounding). fault (self-test):
    "tap" reads row b + 1 instead of b at output row 100; "swap" uses 1 - ly instead of ly everywhere."""
    x = bits_f32(x_bits)
    out = np.empty(x.shape, f32)
    for k in range(x.shape[0]):
        ty, by, ly, _ = taps32(boxes[k][0], boxes[k][2])
        tx, bx, lx, _ = taps32(boxes[k][1], boxes[k][3])
        if fault == "tap":
            by = by.copy()
            by[100] = min(by[100] + 1, N - 1)
        if fault == "swap":
            ly = (f32(1.0) - ly).astype(f32)
        top_rows, bot_rows = x[k][:, ty], x[k][:, by]
        tl, tr, bl, br = top_rows[:, :, tx], top_rows[:, :, bx], bot_rows[:, :, tx], bot_rows[:, :, bx]
        lxx, lyy = lx[None, None, :], ly[None, :, None]
        top = tl + (tr - tl) * lxx
        bot = bl + (br - bl) * lxx
        out[k] = top + (bot - top) * lyy
    assert out.dtype == f32
    return bf16_bits(out), out


def axis64(lo, hi, fault=None):
    """W [224 outputs, 224 sources] fp64 of one axis. fault: "tap" moves output 100's b tap by one index, "swap" trades l and 1 - l."""
    t, b, l, _ = taps32(lo, hi)
    l = l.astype(np.float64)
    if fault == "tap":
        b = b.copy()
        b[100] = min(b[100] + 1, N - 1)
    if fault == "swap":
        l = 1.0 - l
    W = np.zeros((N, N))
    i = np.arange(N)
    np.add.at(W, (i, t), 1.0 - l)
    np.add.at(W, (i, b), l)
    return W


def fwd64(x, boxes, fault=None):
    """x fp64 [B,6,224,224] -> Wy x Wx^T per plane."""
    x = np.asarray(x, np.float64)
    return np.stack([axis64(bx[0], bx[2], fault) @ x[k] @ axis64(bx[1], bx[3]).T for k, bx in enumerate(boxes)])


def bf16_half_ulp(a):
    """Half a bf16 ulp at magnitude a >= 0 (0 at 0)."""
    a = np.asarray(a, np.float64)
    _m, ex = np.frexp(np.where(a == 0, 1.0, a))
    return np.where(a == 0, 0.0, np.ldexp(0.5, ex - 8))


def bwd64(g, boxes, fault=None):
    """g fp64 [B,6,224,224] (the gradient of the output) -> (value, bound, A) [B,6,224,224]: the explicit transpose Wy^T g Wx of the fp64 taps,
    the bound of the module docstring and A = sum |w g|."""
    g = np.asarray(g, np.float64)
    val, A = np.empty(g.shape), np.empty(g.shape)
    for k, bx in enumerate(boxes):
        Wy, Wx = axis64(bx[0], bx[2], fault), axis64(bx[1], bx[3])
        val[k] = Wy.T @ g[k] @ Wx
        A[k] = Wy.T @ np.abs(g[k]) @ Wx
    arith = K_OPS * U * A
    return val, bf16_half_ulp(np.abs(val) + arith) + arith, A


def untouched(boxes):
    """bool [B,224,224]: source elements no output of the image's box touches (their gradient is exactly 0)."""
    out = []
    for bx in boxes:
        ry = axis64(bx[0], bx[2]).sum(axis=0) == 0
        rx = axis64(bx[1], bx[3]).sum(axis=0) == 0
        out.append(ry[:, None] | rx[None, :])
    return np.stack(out)


def worst_ratio(got, val, bound):
    """max |got - val| / bound (0 / 0 = 0, an error against a zero bound is infinite) and its flat index."""
    err = np.abs(np.asarray(got, np.float64) - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    e = int(np.argmax(r))
    return float(r.ravel()[e]), e


# ---- the GPU tests' inputs (built once, shared, never modified) ----
S09 = float(center_box(0.9)[2] - center_box(0.9)[0])


def boxes_a():
    s = f32(center_box(0.9)[2] - center_box(0.9)[0])
    return np.stack([center_box(0.9), np.array([0, 0, s, s], f32), np.array([f32(1) - s, f32(1) - s, 1, 1], f32)]).astype(f32)


def boxes_b():
    return np.array([[0, 0, 1, 1], [0.25, 0.25, 0.75, 0.75], [0.125, 0.03125, 0.825, 0.98125]], f32)  # identity, side 0.5, sides 0.7 x 0.95


_CACHE = {}


def inputs():
    """x bits [3,6,224,224]: image 0 seeded normal scaled into +-2.6 (bf16), image 1 a constant per plane, image 2 one-hot per plane; and a
    seeded bf16 gradient [3,6,224,224]."""
    if "in" not in _CACHE:
        rs = np.random.RandomState(9)
        x = np.zeros((3, 6, N, N), f32)
        n = rs.standard_normal((6, N, N))
        x[0] = (n * (2.6 / np.abs(n).max())).astype(f32)
        x[1] = np.array([0.5, -1.25, 2.0, -2.6, 0.0078125, 1.0], f32)[:, None, None]
        for c in range(6):
            x[2, c, 17 + 31 * c, 200 - 29 * c] = f32(1.5 + c)
        g = (rs.standard_normal((3, 6, N, N)) * 1e-2).astype(f32)
        g[1] = f32(0.75)
        g[2] = 0
        for c in range(6):
            g[2, c, 5 + 40 * c, 219 - 41 * c] = f32(-2.0 - c)
        _CACHE["in"] = (bf16_bits(x), bf16_bits(g))
    return _CACHE["in"]


# ---- composition with K1 / K2 (tests/patch_grad_ref.py) ----
def compose_ref(g_bits, boxes, keep, xy, theta, geometry, ph, pw, pdesc=None, fault=None):
    """patch gradient of CropResize(PatchApply(...)) for an output gradient g (bf16 bits [B,6,224,224]): patch_grad_ref's K2 reference fed with
    the fp64 transpose of K9's taps instead of a bf16 pixel gradient. BOUND: that file's per-texel bound with the pixel gradient's own error
    D = K9's per-element bound (bwd64: half a bf16 ulp + 16 u sum|w g|, the rounding to bf16 of K9's output included) carried through the
    scatter weights as dG — the path that file already uses for K2''s inexact tile gradients (its T6) — so every term T1..T5 stays as derived
    there and K9 adds sum_k w_k (D0_k / std0 + D1_k / std1) per texel, inside the same SAFETY factor."""
    import patch_grad_ref as R

    val, bound, _ = bwd64(bits_f32(g_bits).astype(np.float64), boxes, fault)
    B = val.shape[0]
    sz = R._sizes(B, ph, pw, pdesc)
    total = 3 * ph * pw if pdesc is None else int(max(sz[:, 2] + (3 * sz[:, 0] * sz[:, 1] + 3) // 4 * 4))
    v, d = val.reshape(B, 6, N * N), bound.reshape(B, 6, N * N)

    def pix(b, idx):
        return v[b][:3, idx].T, v[b][3:, idx].T, d[b][:3, idx].T, d[b][3:, idx].T

    rec = R._records(B, keep, xy, theta, geometry, sz, pix)
    multi = pdesc is not None
    return R._finish(rec, B, xy, sz, total, multi, dict(kind="k2", B=B, ph=ph, pw=pw, pdesc=pdesc, band_rows=R.band_rows(B, ph, pw, multi)))


# ---- agreement of the training path with the evaluation (K5 -> K7) ----
def eval_bound(mean6, std6):
    """Per channel [6]: how far CropResize(K1) with the centre box may lie from eval_pixel_values(K5 paste, center_crop=True) when frame and patch
    hold exact multiples of 1/255 (so K5's quantisation is exact). With n(v) = (v - mean) / std, which commutes with the bilinear blend (affine,
    taps sum to 1), and N = max(|n(0)|, |n(1)|) the largest normalised magnitude of the channel:
        (1/255) / std   K7's truncation q = (int)(v * 255.5): q/255 - v lies in (-1/255, 1/510]
        3 * 2^-9 * N    three bf16 roundings K7 -> K9 do not share: K1's of the source values (a convex combination of errors <= 2^-9 |n|),
                        K9's of its output and K7's of its output (relative half ulp 2^-9 each)
        32 u * N        the fp32 operations of both chains (normalise: 2 each; blends: 6 each; u = 2^-24), with room"""
    mean6, std6 = np.asarray(mean6, np.float64), np.asarray(std6, np.float64)
    n_max = np.maximum(np.abs(mean6 / std6), np.abs((1.0 - mean6) / std6))
    return (1.0 / 255.0) / std6 + (3 * 2.0 ** -9 + 32 * U) * n_max
