"""The patch regulariser of include/vaa.h (K6: total variation + non-printability score) restated with torch CPU ops, parameterised by dtype —
the values with tensor ops, the gradient with AUTOGRAD, so the kernel's analytic gradient is checked against something independent — and the
fixed inputs the regulariser tests share (a plain module, not a conftest). With p [3,ph,pw], N3 = 3*ph*pw, q [K,3], eps = 1e-6:

    TV  = ( sum |p[c,i,j+1] - p[c,i,j]| + sum |p[c,i+1,j] - p[c,i,j]| ) / N3
    NPS = ( sum over the texels of min_k sqrt( sum_c (p[c,t] - q[k,c])^2 + eps ) ) / N3
"""
import functools
import itertools

import torch

EPS = 1e-6
W_TV, W_NPS = 2.5, 1.5   # the weights of the comparisons: neither term drowns the other (|dTV| <= 4/N3, |dNPS| <= 1/N3 per element)
TIE = 2e-6               # a palette colour whose fp64 distance is within TIE of a texel's minimum is an admissible argmin for that texel

# 50x50: the shipped patch; 100x100: ten thousand texels; 17x23: 391 texels — a partly filled last workgroup of 256, rows that straddle the
# workgroup boundary (neighbours in another workgroup); 1x7 / 7x1: one difference direction absent; 1x1: no neighbour at all
SHAPES = {"50x50": (3, 50, 50), "100x100": (3, 100, 100), "17x23": (3, 17, 23), "1x7": (3, 1, 7), "7x1": (3, 7, 1), "1x1": (3, 1, 1)}
PALETTES = ("k1", "grid27", "rand64")
CASES = [f"{s}-{p}" for s in SHAPES for p in PALETTES] + ["50x50-grid27-q8", "17x23-rand64-q8"]  # -q8: quantised to multiples of 1/8


def palette(name):
    if name == "grid27":
        return torch.tensor(list(itertools.product((0.15, 0.5, 0.85), repeat=3)), dtype=torch.float32)
    g = torch.Generator().manual_seed({"k1": 31, "rand64": 32}[name])
    return torch.rand(({"k1": 1, "rand64": 64}[name], 3), generator=g)


def tv(p):
    return ((p[:, :, 1:] - p[:, :, :-1]).abs().sum() + (p[:, 1:, :] - p[:, :-1, :]).abs().sum()) / p.numel()


def distances(p, q):
    """[N, K]: d_k(t) of every texel (row-major) and colour."""
    e = p.reshape(3, -1).t()[:, None, :] - q[None, :, :]
    return ((e * e).sum(dim=2) + EPS).sqrt()


def nps(p, q):
    return distances(p, q).min(dim=1).values.sum() / p.numel()


def values(patch, pal, dtype=torch.float64):
    """(TV, NPS) as python floats, computed in `dtype` (pal None: NPS = 0)."""
    p = patch.to(dtype)
    return float(tv(p)), (float(nps(p, pal.to(dtype))) if pal is not None else 0.0)


def grad(patch, pal, w_tv, w_nps, dtype=torch.float64):
    """d (w_tv*TV + w_nps*NPS) / d patch by autograd, [3,ph,pw] in `dtype`."""
    p = patch.detach().to(dtype).requires_grad_(True)
    total = w_tv * tv(p)
    if pal is not None and w_nps != 0:
        total = total + w_nps * nps(p, pal.to(dtype))
    total.backward()
    return p.grad


def grad_error(g, patch, pal, w_tv, w_nps, g64=None):
    """max over the texels of the error of gradient `g` [3,ph,pw] against the fp64 reference, where a texel's reference is the gradient towards
    ANY palette colour whose fp64 distance is within TIE of that texel's minimum (the argmin may legitimately differ near a tie): per texel the
    smallest, over its admissible colours, of the largest channel error. No texel is left out. Returns (error, max |fp64 gradient|)."""
    g64 = grad(patch, pal, w_tv, w_nps) if g64 is None else g64
    diff = (g.double() - g64).reshape(3, -1)                      # [3, N] against the gradient towards the fp64 argmin k*
    if pal is None or w_nps == 0:
        return float(diff.abs().max()), float(g64.abs().max())
    p, q = patch.double(), pal.double()
    d = distances(p, q)                                           # [N, K]
    dmin, kstar = d.min(dim=1)
    e = p.reshape(3, -1).t()[:, None, :] - q[None, :, :]          # [N, K, 3]
    gk = w_nps * e / d[:, :, None] / p.numel()                    # the NPS gradient towards every colour
    base = diff.t()[:, None, :] + gk[torch.arange(d.shape[0]), kstar][:, None, :]   # kernel - (reference without its NPS term) ...
    err = (base - gk).abs().max(dim=2).values                     # ... minus the NPS term towards colour k: [N, K]
    err = torch.where(d <= dmin[:, None] + TIE, err, torch.full_like(err, float("inf")))
    return float(err.min(dim=1).values.max()), float(g64.abs().max())


def min_gap(patch, pal):
    """The smallest gap between the best and the second-best fp64 distance over the texels (inf for K = 1)."""
    d = distances(patch.double(), pal.double())
    if d.shape[1] < 2:
        return float("inf")
    two = d.topk(2, dim=1, largest=False).values
    return float((two[:, 1] - two[:, 0]).min())


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared inputs and references of one case, computed once and left unchanged: dict(patch, palette, tv64, nps64, grad64, gmax, e_tv,
    e_nps, e_grad_rel) — e_*: the error of the fp32 restatement against fp64 on the same inputs (the gradient's relative to max |fp64
    gradient|, under grad_error's tie rule): the measured baseline the kernel's bounds are eight times of."""
    parts = name.split("-")
    shape, pal = SHAPES[parts[0]], palette(parts[1])
    g = torch.Generator().manual_seed(2000 + CASES.index(name))
    patch = torch.rand(shape, generator=g)
    if parts[-1] == "q8":  # many exactly-zero differences: sgn(0) = 0
        patch = (patch * 8).round() / 8
    tv64, nps64 = values(patch, pal)
    g64 = grad(patch, pal, W_TV, W_NPS)
    tv32, nps32 = values(patch, pal, torch.float32)
    e_g, gmax = grad_error(grad(patch, pal, W_TV, W_NPS, torch.float32), patch, pal, W_TV, W_NPS, g64)
    return dict(patch=patch.contiguous(), palette=pal, tv64=tv64, nps64=nps64, grad64=g64, gmax=gmax, e_tv=abs(tv32 - tv64), e_nps=abs(nps32 - nps64),
                e_grad_rel=e_g / gmax)


def tolerances(name):
    """(tol_tv, tol_nps, tol_g) of a case: eight times the fp32 restatement's own error, with floors that follow from the definition.
    Values (both at most about 1): a term carries at most six fp32 roundings (difference, three products / FMAs, + eps, sqrt) of quantities
    <= 2, i.e. <= 6 * 2^-24 * 2 = 7e-7, and the normalised sum cannot exceed its largest term's error: floor 1e-6 absolute.
    Gradient, relative to max |fp64 gradient|: about ten roundings at 2^-24 (the six above, the division, the two rounded weights, the product,
    the FMA) on terms no larger than 4*c_tv + c_nps, i.e. 6e-7: floor 2e-6."""
    c = case(name)
    return max(8 * c["e_tv"], 1e-6), max(8 * c["e_nps"], 1e-6), max(8 * c["e_grad_rel"], 2e-6)
