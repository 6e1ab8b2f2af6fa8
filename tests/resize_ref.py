"""References of the camera-frame resize (K8, include/vaa.h: vaa_frame_resize), shared by test_resize_host.py and test_gpu_resize.py. Nothing
here comes from the package under test: the tap rule and the two passes are restated from the header.

  taps_f64     the header's ScaleAndTranslate rule for lanczos3 with antialias, one axis, in fp64: (start, normalised weights [224,T]).
  taps_f32     the same tables with the weights rounded to fp32: what the kernel is given.
  resize_f32   the header's arithmetic with EVERY operation on np.float32 (one rounding per operation, no FMA, horizontal pass first, taps in
               ascending source index from 0.0f, rint, clip, uint8): what the kernel must reproduce byte for byte.
  resize_f64   taps and both passes in fp64, unrounded: values [B,224,224,3] float64. `compare_f64` rounds them and leaves out the pixels whose
               value lies within TIE_BAND of a .5 tie, where an fp32 evaluation may legitimately round the other way.
"""
import math

import numpy as np

N = 224
TIE_BAND = 1e-3
MAX_EXCLUDED = 0.01  # share of a case's pixels that may sit in the tie band

# (B, H, W) of every case the GPU test runs, with the seed of its frames; test_resize_host.py checks the excluded share of each
CASES = {
    "libero": (1, 256, 256, 11),
    "bridge": (3, 480, 640, 12),
    "upsample": (2, 128, 160, 13),
    "odd_row_bytes": (1, 250, 302, 14),
    "identity": (2, 224, 224, 15),
    "min": (1, 8, 8, 16),
    "tall": (1, 2048, 8, 17),
    "wide_rows": (1, 9, 1030, 18),   # a row of more than 1024 pixels: the kernel walks the source in chunks of 4 rows instead of 8
}


def frames(B: int, H: int, W: int, seed: int) -> np.ndarray:
    """uint8 [B,H,W,3]: per image and channel a linear gradient of random direction that runs past both ends of [0, 255] (so that bytes
    saturate at 0 and at 255) plus uniform noise of +-24."""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1.0, 1.0, H), np.linspace(-1.0, 1.0, W), indexing="ij")
    out = np.empty((B, H, W, 3), np.uint8)
    for b in range(B):
        for c in range(3):
            ang = rs.uniform(0.0, 2.0 * np.pi)
            g = 127.5 + 150.0 * (np.cos(ang) * xx + np.sin(ang) * yy) / max(abs(np.cos(ang)) + abs(np.sin(ang)), 1e-9) * 1.2
            out[b, :, :, c] = np.clip(np.rint(g + rs.uniform(-24.0, 24.0, size=(H, W))), 0, 255).astype(np.uint8)
    return out


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def lanczos3(x: float) -> float:
    return _sinc(x) * _sinc(x / 3.0) if abs(x) < 3.0 else 0.0


def tap_count(n_in: int) -> int:
    return 2 * math.ceil(3.0 * max(n_in / N, 1.0)) + 1


def span(n_in: int, i: int):
    """(lo, hi) of output index i: the source indices whose weight the rule computes."""
    scale = n_in / N
    ks = max(scale, 1.0)
    s = (i + 0.5) * scale
    return max(math.ceil(s - 3.0 * ks - 0.5), 0), min(math.floor(s + 3.0 * ks - 0.5), n_in - 1)


def taps_f64(n_in: int):
    scale = n_in / N
    ks = max(scale, 1.0)
    T = tap_count(n_in)
    start = np.empty(N, np.int32)
    w = np.zeros((N, T), np.float64)
    for i in range(N):
        s = (i + 0.5) * scale
        lo, hi = span(n_in, i)
        raw = [lanczos3((j + 0.5 - s) / ks) for j in range(lo, hi + 1)]
        total = 0.0
        for v in raw:
            total += v
        start[i] = max(min(lo, n_in - T), 0)
        for k, v in enumerate(raw):
            w[i, lo - start[i] + k] = v / total
    return start, w


def taps_f32(n_in: int):
    start, w = taps_f64(n_in)
    return start, w.astype(np.float32)


def _passes(src, sx, wx, sy, wy, flt, order="hv"):
    """Both passes in the float type `flt`, each tap one multiply and one add on arrays of that type, in ascending tap order from 0."""
    p = src.astype(flt)
    B, H, W, _ = p.shape

    def horizontal(a):  # [B,R,W,3] -> [B,R,224,3]
        h = np.zeros((a.shape[0], a.shape[1], N, 3), flt)
        for t in range(wx.shape[1]):
            h = h + wx[:, t].astype(flt)[None, None, :, None] * a[:, :, sx + t, :]
        return h

    def vertical(a):  # [B,H,C,3] -> [B,224,C,3]
        v = np.zeros((a.shape[0], N, a.shape[2], 3), flt)
        for t in range(wy.shape[1]):
            v = v + wy[:, t].astype(flt)[None, :, None, None] * a[:, sy + t, :, :]
        return v

    out = vertical(horizontal(p)) if order == "hv" else horizontal(vertical(p))
    assert out.dtype == flt
    return out


def _oriented(src_u8, rot180):
    src_u8 = np.asarray(src_u8, dtype=np.uint8)
    return src_u8[:, ::-1, ::-1] if rot180 else src_u8


def _to_u8(v):
    return np.minimum(np.maximum(np.rint(v), 0), 255).astype(np.uint8)  # np.rint: half to even


def resize_f32(src_u8, rot180=False, tables=None, order="hv") -> np.ndarray:
    """uint8 [B,H,W,3] -> uint8 [B,224,224,3], the header's fp32 arithmetic. tables = (sx, wx, sy, wy) replaces the rule's own (the
    perturbation self-test passes shifted ones); order="vh" runs the vertical pass first (another rounding: must NOT be what the kernel does)."""
    src = _oriented(src_u8, rot180)
    sx, wx, sy, wy = tables if tables is not None else (*taps_f32(src.shape[2]), *taps_f32(src.shape[1]))
    return _to_u8(_passes(src, sx, wx, sy, wy, np.float32, order))


def resize_f64(src_u8, rot180=False) -> np.ndarray:
    """The unrounded fp64 values [B,224,224,3] (fp64 taps, fp64 passes)."""
    src = _oriented(src_u8, rot180)
    return _passes(src, *taps_f64(src.shape[2]), *taps_f64(src.shape[1]), np.float64)


def compare_f64(got_u8, v64):
    """(number of pixels outside the tie band where got_u8 != round(v64), share of pixels inside the tie band)."""
    frac = v64 - np.floor(v64)
    tie = np.abs(frac - 0.5) < TIE_BAND
    want = _to_u8(v64)
    return int(((np.asarray(got_u8) != want) & ~tie).sum()), float(tie.mean())
