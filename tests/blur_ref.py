"""References of K11 (include/vaa.h: vaa_defocus_blur_fwd / _bwd), shared by test_blur_host.py and test_gpu_blur.py. Plain numpy; calls no HIP code.

  taps64 / taps32   the tap rule (ops.blur_taps restated): e_t = exp(-t^2 / (2 sigma^2)) in fp64, e_t < 2^-40 -> 0, normalised, rounded to fp32.
  fwd32       the forward contract with EVERY operation on np.float32 arrays (one numpy operation per stated operation, no FMA) -> bf16 bits:
              what the kernel must reproduce byte for byte.
  bwd32       the adjoint's stated order in np.float32, written as the SCATTER the contract's brackets describe (output index i sends w_|t| * g[i]
              to c(i + t), i ascending, t ascending within it) — the kernel gathers; this is the subject of the bound's self-test.
  band64      the dense 224 x 224 matrix A of one axis in fp64, A[i, c(i + t)] += w_|t| with the fp32 taps widened;
  fwd64       A x A^T per plane;   bwd64   A^T g A per plane, with a bound per element.

BOUND (u = 2^-24, first order; SAFETY = 2 covers the higher orders). A running fp32 sum of n products from 0.0f, s = fl(...fl(fl(w1 x1) + fl(w2 x2))...),
differs from the exact sum by at most (n + 1) u sum |w_k x_k| (each term carries its product's rounding and at most n - 1 adds' — the add onto 0.0f
is exact — so n factors (1 + d); n + 1 is the standard, slightly generous count). The second pass runs on the first pass's rounded values, so
element (r, j) of either direction is within
        ((n_r + 1) + (n_j + 1)) u  *  S[r, j],        S = |A|^T |g| |A|  (adjoint)   or   |A| |x| |A|^T  (forward)  = sum |w| |w| |g|
of the fp64 value, with n the number of terms of that index's sum: 13 in the forward; in the adjoint the number of (i, t) pairs with c(i + t)
equal to the index — at most 13 in the interior, 28 (= 7 + 6 + ... + 1) at index 0 and 223, which collect the folded taps. Taps that are exactly
0 are counted too (their terms are exact: the count only errs upwards). The single rounding to bf16 adds half a bf16 ulp, taken at |value| + the
arithmetic bound (the binade the rounded fp32 value can lie in). An all-zero plane has S = 0: bound 0, it must come out exactly 0.
Nothing here was fitted to a kernel's output.
"""
import numpy as np

N = 224
R = 6  # taps on each side
U = 2.0 ** -24
SAFETY = 2.0
FLOOR = 2.0 ** -40
MAX_SIGMA = 2.0
SIGMAS = (0.0, 0.5, 1.0, 2.0)  # one per image of inputs()
EDGES = (0, 1, 5, 6, 7) + tuple(range(216, 224))
f32 = np.float32


def taps64(sigma):
    """One sigma -> fp64 [7] {w0..w6} before the rounding to fp32."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma < 0.0 or sigma > MAX_SIGMA:
        raise ValueError(f"sigma {sigma!r} outside [0, {MAX_SIGMA}]")
    e = np.zeros(7)
    e[0] = 1.0
    for t in range(1, 7):
        v = np.exp(-(t * t) / (2.0 * sigma * sigma)) if sigma * sigma > 0.0 else 0.0
        e[t] = v if v >= FLOOR else 0.0
    return e / (e[0] + 2.0 * e[1:].sum())


def taps32(sigmas):
    """sigmas [B] -> fp32 [B,8] rows {w0..w6, 0}."""
    out = np.zeros((len(sigmas), 8), f32)
    for b, s in enumerate(sigmas):
        out[b, :7] = taps64(s)
    return out


def bf16_bits(v):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.asarray(v, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(f32)


def _index(t, pad):
    """source index of i + t per i, and whether the term exists. pad: "clamp" (the contract), "zero", "reflect" (self-test faults)."""
    i = np.arange(N) + t
    inside = (i >= 0) & (i < N)
    if pad == "reflect":
        i = np.where(i < 0, -i, np.where(i >= N, 2 * (N - 1) - i, i))
    return np.clip(i, 0, N - 1), (inside if pad == "zero" else np.ones(N, bool))


def _faulty_taps(taps, fault):
    taps = np.asarray(taps, f32)
    if fault == "swap":  # the tap rows of images 1 and 2 swapped
        taps = taps.copy()
        taps[[1, 2]] = taps[[2, 1]]
    return taps


def fwd32(x_bits, taps, fault=None):
    """x_bits uint16 [B,6,224,224], taps fp32 [B,8] -> (bf16 bits, fp32 values before the rounding). fault (self-test): "zero" / "reflect"
    padding instead of the clamp, "swap" (tap rows of images 1 and 2), "mid" (bf16 rounding between the passes), "drop" (tap t = +1 left out)."""
    x = bits_f32(x_bits)
    taps = _faulty_taps(taps, fault)
    pad = fault if fault in ("zero", "reflect") else "clamp"
    out = np.empty(x.shape, f32)
    for b in range(x.shape[0]):
        w = taps[b]
        h = np.zeros(x.shape[1:], f32)
        for t in range(-R, R + 1):
            if fault == "drop" and t == 1:
                continue
            idx, on = _index(t, pad)
            h = h + w[abs(t)] * np.where(on[None, None, :], x[b][:, :, idx], f32(0.0))
        if fault == "mid":
            h = bits_f32(bf16_bits(h))
        v = np.zeros(x.shape[1:], f32)
        for t in range(-R, R + 1):
            if fault == "drop" and t == 1:
                continue
            idx, on = _index(t, pad)
            v = v + w[abs(t)] * np.where(on[None, :, None], h[:, idx, :], f32(0.0))
        assert h.dtype == f32 and v.dtype == f32
        out[b] = v
    return bf16_bits(out), out


def bwd32(g_bits, taps, fault=None):
    """The adjoint in the stated order, np.float32, as a scatter: (bf16 bits, fp32 values). fault: "noedge" (a tap the clamp folds is dropped
    instead of accumulated), "swap", "drop" (tap t = +1 left out)."""
    g = bits_f32(g_bits)
    taps = _faulty_taps(taps, fault)
    out = np.empty(g.shape, f32)
    for b in range(g.shape[0]):
        w = taps[b]
        a = np.zeros(g.shape[1:], f32)
        for y in range(N):
            for t in range(-R, R + 1):
                if (fault == "drop" and t == 1) or (fault == "noedge" and not 0 <= y + t < N):
                    continue
                r = min(max(y + t, 0), N - 1)
                a[:, r, :] = a[:, r, :] + w[abs(t)] * g[b][:, y, :]
        gx = np.zeros(g.shape[1:], f32)
        for x in range(N):
            for t in range(-R, R + 1):
                if (fault == "drop" and t == 1) or (fault == "noedge" and not 0 <= x + t < N):
                    continue
                j = min(max(x + t, 0), N - 1)
                gx[:, :, j] = gx[:, :, j] + w[abs(t)] * a[:, :, x]
        assert gx.dtype == f32
        out[b] = gx
    return bf16_bits(out), out


def band64(row):
    """One tap row (fp32 [8]) -> (A fp64 [224 outputs, 224 sources], n_fwd [224], n_adj [224]): A[i, c(i + t)] += w_|t|; the number of terms of
    output i's sum (13) and of source r's transposed sum."""
    w = np.asarray(row, f32).astype(np.float64)
    A = np.zeros((N, N))
    n_adj = np.zeros(N)
    for i in range(N):
        for t in range(-R, R + 1):
            c = min(max(i + t, 0), N - 1)
            A[i, c] += w[abs(t)]
            n_adj[c] += 1
    return A, np.full(N, 2 * R + 1.0), n_adj


def bf16_half_ulp(a):
    """Half a bf16 ulp at magnitude a >= 0 (0 at 0)."""
    a = np.asarray(a, np.float64)
    _m, ex = np.frexp(np.where(a == 0, 1.0, a))
    return np.where(a == 0, 0.0, np.ldexp(0.5, ex - 8))


def _bounded(val, S, n_rows, n_cols):
    arith = SAFETY * ((n_rows[:, None] + 1.0) + (n_cols[None, :] + 1.0)) * U * S
    return val, bf16_half_ulp(np.abs(val) + arith) + arith, S


def fwd64(x, taps):
    """x fp64 [B,6,224,224] -> (A x A^T per plane, bound, S = |A| |x| |A|^T)."""
    x = np.asarray(x, np.float64)
    val, S = np.empty(x.shape), np.empty(x.shape)
    for b in range(x.shape[0]):
        A, n, _ = band64(taps[b])
        val[b] = A @ x[b] @ A.T
        S[b] = A @ np.abs(x[b]) @ A.T
    return _bounded(val, S, n, n)


def bwd64(g, taps):
    """g fp64 [B,6,224,224] -> (A^T g A per plane, bound, S = |A|^T |g| |A|): the explicit transpose, with the bound of the module docstring."""
    g = np.asarray(g, np.float64)
    val, S = np.empty(g.shape), np.empty(g.shape)
    n = None
    for b in range(g.shape[0]):
        A, _, n = band64(taps[b])
        val[b] = A.T @ g[b] @ A
        S[b] = A.T @ np.abs(g[b]) @ A
    return _bounded(val, S, n, n)


def worst_ratio(got, val, bound):
    """max |got - val| / bound (0 / 0 = 0, an error against a zero bound is infinite) and its flat index."""
    err = np.abs(np.asarray(got, np.float64) - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    e = int(np.argmax(r))
    return float(r.ravel()[e]), e


# ---- the tests' inputs and references (built once, shared, never modified) ----
_CACHE = {}
ZERO_PLANE = (2, 4)  # (image, plane) of g that is all zeros


def _field(rs):
    """[4,6,224,224] fp32: magnitudes 2^U(-8, 3) with random signs, and sharp edges on the rows and columns of EDGES (+-8 next to +-2^-8)."""
    v = (np.exp2(rs.uniform(-8.0, 3.0, (4, 6, N, N))) * rs.choice([-1.0, 1.0], (4, 6, N, N))).astype(f32)
    alt = np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(f32)
    for k, e in enumerate(EDGES):
        v[:, :, e, :] = (f32(8.0) if k % 2 == 0 else f32(2.0 ** -8)) * alt[None, None, :]
    for k, e in enumerate(EDGES):
        v[:, :, :, e] = (f32(2.0 ** -8) if k % 2 == 0 else f32(-8.0)) * alt[None, None, :]
    return np.clip(v, -8.0, 8.0)


def inputs():
    """(x bits, g bits) uint16 [4,6,224,224]: seeded, magnitudes in [2^-8, 8], sharp edges on the rows and columns 0, 1, 5, 6, 7, 216..223 of
    every plane; plane ZERO_PLANE of g is all zeros."""
    if "in" not in _CACHE:
        rs = np.random.RandomState(11)
        x, g = _field(rs), _field(rs)
        g[ZERO_PLANE] = 0
        xb, gb = bf16_bits(x), bf16_bits(g)
        for bits in (xb, gb):
            m = np.abs(bits_f32(bits))
            assert ((m >= 2.0 ** -8) | (m == 0)).all() and m.max() <= 8.0
            bits.setflags(write=False)
        _CACHE["in"] = (xb, gb)
    return _CACHE["in"]


def reference():
    """dict of the shared references at inputs() / SIGMAS: taps, fwd_bits (fwd32), fwd64 (value, bound), bwd64 (value, bound)."""
    if "ref" not in _CACHE:
        xb, gb = inputs()
        taps = taps32(SIGMAS)
        f_val, f_bound, _ = fwd64(bits_f32(xb).astype(np.float64), taps)
        b_val, b_bound, _ = bwd64(bits_f32(gb).astype(np.float64), taps)
        ref = dict(taps=taps, fwd_bits=fwd32(xb, taps)[0], fwd=f_val, fwd_bound=f_bound, gx=b_val, gx_bound=b_bound)
        for v in ref.values():
            v.setflags(write=False)
        _CACHE["ref"] = ref
    return _CACHE["ref"]
