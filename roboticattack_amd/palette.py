"""The printable-colour palette of the non-printability score (K6, include/vaa.h: vaa_patch_reg): the built-in default, the text-file form
and the checks both share. A palette is [K,3] float32 RGB in [0,1] with 1 <= K <= 64."""
from __future__ import annotations

import itertools

import numpy as np

MAX_COLOURS = 64  # vaa_patch_reg stages the palette in LDS: at most 64 colours


def default_palette() -> np.ndarray:
    """The 27-colour grid {0.15, 0.5, 0.85}^3 — a PLACEHOLDER for a measured printer palette (print a colour chart, photograph it with the
    target camera, list the colours that came out): it only keeps texels away from the corners of the RGB cube."""
    return np.array(list(itertools.product((0.15, 0.5, 0.85), repeat=3)), dtype=np.float32)


def check_palette(palette) -> np.ndarray:
    """`palette` (array-like or tensor [K,3]) as a contiguous float32 array; ValueError on a wrong shape, more than 64 rows, a value outside [0,1]."""
    a = np.ascontiguousarray(np.asarray(palette.detach().cpu() if hasattr(palette, "detach") else palette, dtype=np.float32))
    if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 1:
        raise ValueError(f"nps palette: expected [K,3] with K >= 1, got shape {tuple(a.shape)}")
    if a.shape[0] > MAX_COLOURS:
        raise ValueError(f"nps palette: {a.shape[0]} colours exceed the limit of {MAX_COLOURS}")
    if not bool(np.isfinite(a).all()) or float(a.min()) < 0.0 or float(a.max()) > 1.0:
        raise ValueError("nps palette: every value must lie in [0,1]")
    return a


def load_palette(path: str) -> np.ndarray:
    """A palette text file — one `r g b` triplet in [0,1] per line (blanks or commas between the values), `#` starts a comment, empty lines are
    skipped: the format of the usual 30values.txt."""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            text = line.split("#", 1)[0].replace(",", " ").split()
            if not text:
                continue
            try:
                vals = [float(v) for v in text]
            except ValueError:
                vals = None
            if vals is None or len(vals) != 3:
                raise ValueError(f"nps palette {path}:{no}: expected three numbers `r g b`, got {line.strip()!r}")
            rows.append(vals)
    if not rows:
        raise ValueError(f"nps palette {path}: no colour in the file")
    try:
        return check_palette(rows)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
