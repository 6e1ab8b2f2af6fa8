"""The colour jitter of include/vaa.h (K0c) restated with torch CPU ops + autograd, in fp32 or fp64, and the fixed inputs the jitter tests share
(a plain module, not a conftest). Per image b with factors (beta, kappa, sigma), p the base patch [3,ph,pw], N = ph*pw:

    y1 = clamp(beta*p, 0, 1);  m = mean over the texels of gray(y1);  y2 = clamp(kappa*y1 + (1-kappa)*m, 0, 1)
    y3 = clamp(sigma*y2 + (1-sigma)*gray(y2), 0, 1)          gray(y) = 0.299 y_R + 0.587 y_G + 0.114 y_B

The adjoint is autograd's: torch.clamp passes the gradient where 0 <= pre-clamp <= 1, bounds included."""
import functools

import torch

# (patch shape, B, factors): 50x50 is the shipped patch; 7x5 has odd sizes and fewer texels (35) than a wave; 100x100 has more texels (10000)
# than one pass of a 1024-thread workgroup. Every stage sees a factor below and above 1 in every case; kappa = 0.5 is in each of them.
_F = ((1.4, 0.6, 1.4), (0.6, 1.4, 0.6), (1.2, 0.5, 1.3), (0.8, 1.3, 0.8))
CASES = {
    "50x50": ((3, 50, 50), (_F[0], _F[1], _F[2])),
    "7x5": ((3, 7, 5), (_F[2], _F[3])),
    "100x100": ((3, 100, 100), (_F[1], _F[2])),
}
EDGE = 1e-5  # a texel whose fp64 pre-clamp value lies this close to 0 or 1 (without being exactly 0 or 1) is left out of gradient comparisons


def _gray(y):
    return 0.299 * y[:, 0] + 0.587 * y[:, 1] + 0.114 * y[:, 2]


def jitter_stages(patch, factors, dtype=torch.float64, detach_mean=False):
    """patch [3,ph,pw], factors [B,3] -> (y3 [B,3,ph,pw], (pre1, pre2, pre3) pre-clamp values, each [B,3,ph,pw]), in `dtype`.
    detach_mean: the whole-patch mean m is treated as a constant by autograd (what an adjoint WITHOUT the mean term computes)."""
    p = patch.to(dtype)[None]
    f = factors.to(dtype)
    beta, kappa, sigma = (f[:, k].view(-1, 1, 1, 1) for k in range(3))
    pre1 = beta * p
    y1 = pre1.clamp(0, 1)
    m = _gray(y1).mean(dim=(1, 2)).view(-1, 1, 1, 1)
    if detach_mean:
        m = m.detach()
    pre2 = kappa * y1 + (1 - kappa) * m
    y2 = pre2.clamp(0, 1)
    pre3 = sigma * y2 + (1 - sigma) * _gray(y2)[:, None]
    return pre3.clamp(0, 1), (pre1, pre2, pre3)


def jitter_fwd(patch, factors, dtype=torch.float64):
    return jitter_stages(patch, factors, dtype)[0]


def jitter_grad(patch, factors, gout, dtype=torch.float64, detach_mean=False):
    """sum_b adjoint_b(gout_b): d <y3, gout> / d patch, [3,ph,pw] in `dtype` (gout [B,3,ph,pw])."""
    p = patch.detach().to(dtype).requires_grad_(True)
    y3, _ = jitter_stages(p, factors, dtype, detach_mean)
    y3.backward(gout.to(dtype))
    return p.grad


def kept_texels(patch, factors):
    """[ph,pw] bool: False where any fp64 pre-clamp value of any image, stage and channel lies within EDGE of 0 or 1 without being exactly 0 or 1
    (there the fp32 gate may legitimately differ from the fp64 one)."""
    _, pres = jitter_stages(patch, factors, torch.float64)
    near = torch.zeros(patch.shape[1:], dtype=torch.bool)
    for pre in pres:
        for edge in (0.0, 1.0):
            d = (pre - edge).abs()
            near |= ((d < EDGE) & (d != 0)).any(dim=0).any(dim=0)
    return ~near


def _inputs(shape, factors, seed, saturate=False):
    g = torch.Generator().manual_seed(seed)
    patch = torch.rand(shape, generator=g) * 0.9 + 0.05  # uniform in [0.05, 0.95]
    if saturate:  # about 20 % exact 0.0 and 20 % exact 1.0 texels
        u = torch.rand(shape, generator=g)
        patch = torch.where(u < 0.2, torch.zeros(()), torch.where(u > 0.8, torch.ones(()), patch))
    f = torch.tensor(factors, dtype=torch.float32)
    gout = torch.randn((len(factors),) + tuple(shape), generator=g)
    return patch.contiguous(), f, gout


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared inputs and references of one case, computed once: dict(patch, factors, gout, fwd64, grad64, keep, e_fwd, e_grad_rel) where
    e_fwd = max |fp32 restatement - fp64| and e_grad_rel = the same for the gradient over the kept texels, relative to max |fp64 gradient|:
    the measured baseline the kernel's tolerances are eight times of."""
    if name == "saturated":  # brightness alone, on a patch with exact 0.0 / 1.0 texels: nothing is left out
        shape, factors = (3, 50, 50), ((0.8, 1.0, 1.0), (1.25, 1.0, 1.0))
        patch, f, gout = _inputs(shape, factors, 77, saturate=True)
        keep = torch.ones(shape[1:], dtype=torch.bool)
    else:
        shape, factors = CASES[name]
        patch, f, gout = _inputs(shape, factors, 1000 + sorted(CASES).index(name))
        keep = kept_texels(patch, f)
    fwd64, grad64 = jitter_fwd(patch, f), jitter_grad(patch, f, gout)
    e_fwd = float((jitter_fwd(patch, f, torch.float32).double() - fwd64).abs().max())
    gmax = float(grad64[:, keep].abs().max())
    e_grad_rel = float((jitter_grad(patch, f, gout, torch.float32).double() - grad64)[:, keep].abs().max()) / gmax
    return dict(patch=patch, factors=f, gout=gout, fwd64=fwd64, grad64=grad64, keep=keep, e_fwd=e_fwd, e_grad_rel=e_grad_rel)


def tolerances(name):
    """(tol_f, tol_g) of a case. The floors follow from the definition: about 8 roundings of values <= 1.4 at 2^-24 plus m's reduction for the
    forward; the factor 8 covers a different but fixed summation order for m and for the adjoint's whole-patch sum."""
    c = case(name)
    return max(8 * c["e_fwd"], 3e-6), max(8 * c["e_grad_rel"], 1e-5)
