"""Tap tables of K8 (include/vaa.h: vaa_frame_resize): the lanczos3 filter with antialias that the reference's evaluations put in front of
every camera frame (experiments/robot/libero/libero_utils.py:44, experiments/robot/bridge/bridgev2_utils.py:112), per axis and in fp64.

The rule is TensorFlow's ScaleAndTranslate as include/vaa.h restates it FROM MEMORY; TensorFlow cannot be run on this platform, so the tables
could not be compared with it. The header is the definition, this module follows it line by line.
"""
from __future__ import annotations

import math

import numpy as np

from ._lib import FRAME_RESIZE_MAX_TAPS
from .constants import IMG

RADIUS = 3.0
MIN_SIDE, MAX_SIDE = 8, 2048  # what vaa_frame_resize takes per axis


def _sinc(x: np.ndarray) -> np.ndarray:
    px = np.pi * x
    return np.where(x == 0.0, 1.0, np.sin(px) / np.where(x == 0.0, 1.0, px))


def lanczos3(x: np.ndarray) -> np.ndarray:
    """L(x) = sinc(x) * sinc(x / 3) on |x| < 3, else 0 (fp64)."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.abs(x) < RADIUS, _sinc(x) * _sinc(x / RADIUS), 0.0)


def tap_count(n_in: int, n_out: int = IMG) -> int:
    return 2 * math.ceil(RADIUS * max(n_in / n_out, 1.0)) + 1


def lanczos3_taps(n_in: int, n_out: int = IMG):
    """One axis, n_in -> n_out: (start int32 [n_out], w float32 [n_out, T]), T = tap_count(n_in). Row i holds the weights of source indices
    start[i] .. start[i] + T - 1: the span of the rule, normalised to sum 1 in fp64 and rounded to fp32, zeros around it."""
    n_in = int(n_in)
    if not MIN_SIDE <= n_in <= MAX_SIDE:
        raise ValueError(f"axis length {n_in} outside [{MIN_SIDE}, {MAX_SIDE}]")
    scale = n_in / n_out
    ks = max(scale, 1.0)
    T = tap_count(n_in, n_out)
    assert T <= FRAME_RESIZE_MAX_TAPS and T <= n_in
    start = np.empty(n_out, np.int32)
    w = np.zeros((n_out, T), np.float32)
    for i in range(n_out):
        s = (i + 0.5) * scale
        lo = max(math.ceil(s - RADIUS * ks - 0.5), 0)
        hi = min(math.floor(s + RADIUS * ks - 0.5), n_in - 1)
        raw = lanczos3((np.arange(lo, hi + 1, dtype=np.float64) + 0.5 - s) / ks)
        total = 0.0
        for v in raw:  # ascending j
            total += float(v)
        start[i] = max(min(lo, n_in - T), 0)
        w[i, lo - start[i]: hi + 1 - start[i]] = (raw / total).astype(np.float32)
    return start, w


def frame_taps(H: int, W: int):
    """The four tables of a vaa_frame_resize call on H x W frames: (start_x, w_x, start_y, w_y); x runs along W, y along H."""
    sx, wx = lanczos3_taps(W)
    sy, wy = lanczos3_taps(H)
    return sx, wx, sy, wy


def pack_taps(sx, wx, sy, wy) -> np.ndarray:
    """The device copy's layout (include/vaa.h: taps_dev): int32 start_x[224], int32 start_y[224], float32 w_x, float32 w_y, as one int32 array."""
    return np.concatenate([sx.astype(np.int32), sy.astype(np.int32), np.ascontiguousarray(wx, np.float32).view(np.int32).ravel(),
                           np.ascontiguousarray(wy, np.float32).view(np.int32).ravel()])
