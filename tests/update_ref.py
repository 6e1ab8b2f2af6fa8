"""fp64 reference of K4 (vaa_patch_update[_seg], and update_one inside vaa_step_epilogue*_update) and of the step epilogue's gradient sum
(partial_reduce_block), with a bound per output element.

Plain numpy in fp64; calls no HIP code and takes no value from the C oracle's patch_update.

WHAT K4 COMPUTES (csrc/vaa_update.hip:patch_update_body, csrc/vaa_common.h:upd_args / update_one; -ffp-contract=off, correctly rounded
divide and sqrt, so every fp32 operation below is one rounding, and the one FMA is written as such), per group of n elements:
    G0   = fl(g * scale)                                    stats[0] = fl32(sum |G0|), stats[1] = fl32(sum G0 / n), both sums in fp64
    coef = min(fl(l1_clip / fl(fl32(sum |G0|) + 1e-6f)), 1)   (l1_clip > 0; else 1)
    G    = fl(G0 * coef)
    m'   = fma(G, one_m_b1, fl(m * b1))
    v'   = fl(fl(v * b2) + fl(fl(one_m_b2 * G) * G))
    den  = fl(fl(sqrt v') + eps)
    upd  = fl(fl(-step_size * m') / den)
    p'   = clamp(fl(p + upd), 0, 1)                         PGD: p' = clamp(fl(p - lr * sign(G)), 0, 1), m and v untouched
HYPER-PARAMETERS enter as the library narrows them (upd_args): lr, b1, b2, eps, l1_clip and scale are fp32 values; 1 - b is formed in double
from the NARROWED b and step_size = lr sqrt(1 - b2^t) / (1 - b1^t) in double from the narrowed values; one_m_b1, one_m_b2 and step_size are
then narrowed to fp32 (one u each, below). The reference uses the un-narrowed doubles of those three.
    This is not where torch narrows them: transformers' AdamW holds the betas as Python doubles, so `add_(g, alpha=1 - b1)` narrows
    fl32(1 - 0.9) and `addcmul_(g, g, value=1 - b2)` fl32(1 - 0.999), where the library forms 1 - fl32(0.999). The two (1 - b2) differ by
    1.29e-5 relatively (3.7 u for 1 - b1), far outside the rounding bound on v. The library's C interface takes the betas as float, so the
    difference is one of the interface, not of the kernel; test_update_ref_host.py hands the independent implementations the narrowed
    values and states the size of the difference (test_double_betas_differ_by_the_narrowing_of_one_minus_beta).

BOUNDS, first order, u = 2^-24, one u per fp32 operation that can round (a product with 1 or with a power of two is exact):
    us = u if scale is no power of two, else 0;  uc = u if coef != 1, else 0;  a64 = n 2^-53 (an fp64 running sum of n terms, relative)
    stats[0]   (us + u + 2 a64) S, S = sum |g scale|        fl(g scale) per element, the narrowing; the kernel's and this module's fp64 sums
    stats[1]   (us + 2 a64) S / n + u |mean|
    coef       c = l1_clip / (S + 1e-6f): rel rc = us + 3u + 2 a64 (fl(g scale), fl32(S), the fp32 add, the divide) where c < 1; 0 where the
               reference's coefficient is 1. Where |c - 1| <= SAFETY rc c the kernel may take either branch: the bound is |c - 1| + rc c
               (meta["near"]; the case table keeps away from it and the host test asserts that).
    G          rel rG = us + uc + rc
    m'         u (|b1 m| + |m'|) + (1 - b1) (dG + u |G|)     fl(m b1), the FMA's one rounding, dG and the narrowing of one_m_b1. Absolute: the
                                                             two terms cancel
    v'         u b2 v + (3u + 2 rG) (1 - b2) G^2 + u v'      both terms are non-negative: fl(v b2); the narrowing of one_m_b2 and the two
                                                             products with G; the add. (At most 4u + 2 rG relatively.)
    den        rel (rel(v') / 2 + u) sqrt(v') / den + u      the sqrt halves rel(v') and rounds; eps is exact; the add
    upd        step_size dm' / den + |upd| (3u + rel(den))   the narrowing of step_size, the product, the divide
    p'         d(upd) + u max(|p|, |p + upd|)                the add; the clamp is 1-Lipschitz, so the bound passes through it unchanged
    PGD        u max(|p|, |p - lr s|) where s != 0; 0 where g is +-0 (p must come back bit for bit). fl(g scale coef) keeps g's sign as long
               as it does not underflow to zero (input condition below), and lr * s is exact.
  SAFETY = 2 multiplies every derived bound once (second-order terms), as in patch_grad_ref.py and loss_ref.py.
  INPUT CONDITION: every non-zero intermediate of every case is above 2^-100 in magnitude (meta["min_nonzero"]; asserted by the host test),
  so no term for denormal results is needed.

EPILOGUE SUM (epilogue_sum_ref): msg[g, e] = fl32(sum over the group's nparts partial tiles, fp64, a fixed two-level order). On the grid of
multiples of 2^-20 with |x| <= 64 and nparts <= 512 every partial sum has under 36 significant bits, so ANY fp64 order is exact and the
kernel's msg must equal np.float32(sum) as a value. Off the grid the bound is u |value| + nparts 2^-52 sum |partial| (the fp32 rounding; the
kernel's and this module's fp64 sums).

NON-FINITE VALUES are out of scope and none are fed: update_one clamps with fminf(1, fmaxf(0, p)), which turns a NaN patch value into 0, and
PGD's sign of a NaN gradient is 0 (the patch stays), whereas np.clip and np.sign propagate NaN. stats does go NaN in the kernel, so the
loops' log shows a non-finite gradient.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
TINY = 2.0 ** -100
EPS6 = np.float64(np.float32(1e-6))  # the kernel's 1e-6f

Ref = collections.namedtuple("Ref", "value bound")


def _f32(x):
    return np.float64(np.float32(x))


def _pow2(x):
    return x > 0 and np.frexp(x)[0] == 0.5


def _is_adam(mode):
    if mode in ("adamw", 0):
        return True
    if mode in ("pgd", 1):
        return False
    raise ValueError(f"unknown optimiser mode {mode!r}")


def k4_ref(p, g, m, v, mode, lr, beta1, beta2, eps, step, l1_clip, grad_scale, P=1, coef_extra_rel=0.0):
    """One K4 step on P groups. p, g (and m, v for AdamW) hold P*n fp32 values; returns dict(patch, m, v, stats [P,2], coef [P]) of
    Ref(value, bound) in fp64, shaped [P, n] (m, v: None for PGD), and meta. coef_extra_rel widens the clip coefficient's relative bound for
    an implementation that sums the norm differently (the host test's torch route)."""
    adam = _is_adam(mode)
    lr, b1, b2, eps, clip, scale = (_f32(x) for x in (lr, beta1, beta2, eps, l1_clip, grad_scale))
    p, g = (np.asarray(a, np.float32).astype(np.float64).reshape(P, -1) for a in (p, g))
    n = p.shape[1]
    us = 0.0 if _pow2(scale) else U
    a64 = n * 2.0 ** -53
    G0 = g * scale  # exact: 48 bits
    S = np.abs(G0).sum(axis=1)
    mean = G0.sum(axis=1) / n
    stats = Ref(np.stack([S, mean], axis=1), SAFETY * np.stack([(us + U + 2 * a64) * S, (us + 2 * a64) * S / n + U * np.abs(mean)], axis=1))
    inter = [G0]
    if clip > 0:
        c = clip / (S + EPS6)
        rc_raw = us + 3 * U + 2 * a64 + coef_extra_rel
        coef = np.minimum(c, 1.0)
        near = np.abs(c - 1.0) <= SAFETY * rc_raw * c
        dcoef = np.where(near, np.abs(c - 1.0) + rc_raw * c, np.where(c < 1.0, rc_raw * c, 0.0))
        margin = np.abs(c - 1.0) / (rc_raw * c)
    else:
        coef, near, dcoef, margin = np.ones(P), np.zeros(P, bool), np.zeros(P), np.full(P, np.inf)
    rc = dcoef / coef
    uc = np.where((coef != 1.0) | near, U, 0.0)
    rG = (us + uc + rc)[:, None]
    G = G0 * coef[:, None]
    dG = np.abs(G) * rG
    inter.append(G)
    out = dict(stats=stats, coef=Ref(coef, SAFETY * dcoef), m=None, v=None)
    if adam:
        m, v = (np.asarray(a, np.float32).astype(np.float64).reshape(P, -1) for a in (m, v))
        omb1, omb2 = 1.0 - b1, 1.0 - b2
        t = float(step)
        ss = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        m1 = b1 * m + omb1 * G
        dm = U * (np.abs(b1 * m) + np.abs(m1)) + omb1 * (dG + U * np.abs(G))
        va, vb = b2 * v, omb2 * G * G
        v1 = va + vb
        dv = U * va + (3 * U + 2 * rG) * vb + U * v1
        with np.errstate(divide="ignore", invalid="ignore"):
            rv = np.where(v1 > 0, dv / v1, 0.0)
        sq = np.sqrt(v1)
        den = sq + eps
        rden = (rv / 2 + U) * sq / den + U
        upd = -ss * m1 / den
        dupd = ss * dm / den + np.abs(upd) * (3 * U + rden)
        pu = p + upd
        dp = dupd + U * np.maximum(np.abs(p), np.abs(pu))
        out["m"], out["v"] = Ref(m1, SAFETY * dm), Ref(v1, SAFETY * dv)
        inter += [b1 * m, omb1 * G, m1, va, omb2 * G, vb, v1, sq, ss * m1, upd]
    else:
        sg = np.sign(G)
        pu = p - lr * sg
        dp = np.where(sg != 0, U * np.maximum(np.abs(p), np.abs(pu)), 0.0)
    out["patch"] = Ref(np.clip(pu, 0.0, 1.0), SAFETY * dp)
    nz = np.concatenate([np.abs(a[a != 0]).ravel() for a in inter])
    out["meta"] = dict(near=near, coef_margin=margin, min_nonzero=float(nz.min()) if nz.size else np.inf,
                       sign_kept=bool(np.all((G == 0) == (g == 0))))
    return out


def epilogue_sum_ref(partials, P=1, wide=False):
    """partials fp32 [P*nparts, n] -> Ref(value, bound) [P, n]: the fp64 sum of each group's tiles. On the grid (module docstring) the value
    is exact and the bound is that of its one fp32 rounding being the correct one: compare with np.float32(value) for equality; `wide`
    adds the fp64 summation term for inputs off the grid."""
    a = np.asarray(partials, np.float32).astype(np.float64)
    nparts = a.shape[0] // P
    a = a.reshape(P, nparts, a.shape[1])
    val = a.sum(axis=1)
    bound = U * np.abs(val)
    if wide:
        bound = bound + nparts * 2.0 ** -52 * np.abs(a).sum(axis=1)
    return Ref(val, bound)


def compare(ref, got, tag=""):
    """Worst |got - value| / bound over the elements (0 / 0 counts as 0; any error against a zero bound, or a non-finite value, is infinite).
    Fails, naming the worst element, when it exceeds 1."""
    got = np.asarray(got, np.float64).reshape(ref.value.shape)
    err = np.abs(got - ref.value)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(ref.bound > 0, err / ref.bound, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    e = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    worst = float(ratio[e]) if ratio.size else 0.0
    assert worst <= 1.0, (f"{tag}: {int((ratio > 1).sum())} of {ratio.size} elements outside their bound; worst at {tuple(int(i) for i in e)}: got "
                          f"{got[e]:.9g}, reference {ref.value[e]:.9g}, error {err[e]:.3g} = {worst:.3g} x bound {ref.bound[e]:.3g}")
    return worst


def outside(ref, got):
    """Fraction of the elements outside their bound (the host test's injected faults)."""
    got = np.asarray(got, np.float64).reshape(ref.value.shape)
    err = np.abs(got - ref.value)
    return float(np.mean(~(err <= ref.bound)))


# ---------------------------------------------------------------------------------------------------------------------------------
# K4 cases (shared by the host and the GPU tests). Every case is ONE step from stated inputs; `chain` = 3 runs three, each fed with the
# kernel's own read-back p / m / v (steps step, step + 1, step + 2).
# ---------------------------------------------------------------------------------------------------------------------------------
K4Case = collections.namedtuple("K4Case", "shape P mode lr b1 b2 eps step clip scale moments stats chain seed")

# the smallest shapes that reach every launch of patch_update_launch and its edges: n <= 8192 -> R = 8 (4 workgroups; 8192 is the last such
# n, 3 leaves all but three threads idle, 1581 a ragged second row), n <= 32768 -> R = 32 (16 workgroups; 8427 is the first ragged row past
# 8192, 32768 the last such n), beyond -> the streaming form
SHAPES = {"r8_n3": (3, 1, 1), "r8_n1581": (3, 17, 31), "r8_n8192": (2, 64, 64), "r32_n8427": (3, 53, 53), "r32_n32768": (2, 128, 128),
          "stream_n33075": (3, 105, 105)}
FORM = {k: {"r8": "K4 4wg", "r32": "K4 16wg", "stream": "K4 streaming"}[k.split("_")[0]] for k in SHAPES}

_D = (0.9, 0.999, 1e-6)
_VARIANTS = {  # mode, P, lr, (b1, b2, eps), step, clip, scale, moments, stats, chain
    "adam_first": ("adamw", 1, 2e-3, _D, 1, 0.0, 1.0, "zero", True, 1),
    "adam_betas_clip": ("adamw", 3, 2e-3, (0.8, 0.99, 1e-8), 2, 1e-3, 0.25, "nonzero", True, 1),
    "adam_eps_lr0": ("adamw", 1, 0.0, (0.9, 0.999, 1e-3), 1000, 1e-3, 1.0, "nonzero", True, 1),
    "adam_eps_late": ("adamw", 3, 2e-3, (0.9, 0.999, 1e-3), 1000, 0.0, 0.25, "nonzero", False, 1),
    "adam_chain": ("adamw", 3, 2e-3, _D, 1, 1e-3, 1.0, "zero", True, 3),
    "pgd_clip_nan": ("pgd", 3, 2e-3, _D, 1, 1e-3, 0.25, "nan", True, 1),
    "pgd_plain": ("pgd", 1, 2e-3, _D, 1, 0.0, 1.0, "none", False, 1),
}
K4_CASES = {}
for _i, (_s, _shape) in enumerate(SHAPES.items()):
    for _j, (_v, (_mode, _P, _lr, (_b1, _b2, _eps), _step, _clip, _scale, _mom, _st, _ch)) in enumerate(_VARIANTS.items()):
        K4_CASES[f"{_s}-{_v}"] = K4Case(_shape, _P, _mode, _lr, _b1, _b2, _eps, _step, _clip, _scale, _mom, _st, _ch, 100 * _i + _j)


def _draw(rs, n, lo, hi):
    """randn * 10^U(lo, hi) with |randn| kept above 0.25 (the input condition: nothing underflows)."""
    z = rs.standard_normal(n)
    z = np.where(np.abs(z) < 0.25, np.copysign(0.25, z), z)
    return z * 10.0 ** rs.uniform(lo, hi, n)


def gradient(rs, n, P):
    """[P, n] fp32. The last group spans 1e-7 .. 1e-1; with three groups, group 0 spans 1e-10 .. 1e-8 (its L1 norm stays under the 1e-3 clip
    at every n here: coef = 1) and group 1 is 30 times the span of the last: the norms differ by decades. Every 97th element is exactly 0
    (alternately -0 and +0); element 1 of a group is the top of its span."""
    spans = [(-10, -8, 1.0), (-7, -1, 30.0), (-7, -1, 1.0)][3 - P:]
    g = np.stack([_draw(rs, n, lo, hi) * f for lo, hi, f in spans])
    g[:, 1] = np.copysign([10.0 ** hi * f for _lo, hi, f in spans], g[:, 1])  # element 1 at the top of its span: the clip bites at n = 3 too
    g = g.astype(np.float32)
    g[:, ::97] = 0.0
    g[:, ::194] = -0.0
    return g


def patch_values(rs, n, P):
    """[P, n] fp32 in [0, 1]: the first min(100, n // 3) elements of a group at 0, the next as many at 1 (the random gradient signs push
    about half of them outwards)."""
    p = rs.uniform(0.0, 1.0, (P, n)).astype(np.float32)
    k = min(100, n // 3)
    p[:, :k] = 0.0
    p[:, k : 2 * k] = 1.0
    return p


def moments(rs, n, P):
    m = _draw(rs, P * n, -7, -2).reshape(P, n).astype(np.float32)
    v = (m.astype(np.float64) ** 2 * rs.uniform(0.5, 30.0, (P, n))).astype(np.float32)
    return m, v


@functools.lru_cache(maxsize=None)
def k4_inputs(name):
    """dict(case, p, g, m, v): read-only fp32 arrays [P, n]; m / v are zeros, drawn, NaN-filled (PGD: must come back untouched) or None."""
    c = K4_CASES[name]
    n = int(np.prod(c.shape))
    rs = np.random.RandomState(c.seed)
    d = dict(case=c, n=n, p=patch_values(rs, n, c.P), g=gradient(rs, n, c.P))
    if c.moments == "nonzero":
        d["m"], d["v"] = moments(rs, n, c.P)
    elif c.moments == "zero":
        d["m"], d["v"] = np.zeros((c.P, n), np.float32), np.zeros((c.P, n), np.float32)
    elif c.moments == "nan":
        d["m"], d["v"] = np.full((c.P, n), np.nan, np.float32), np.full((c.P, n), np.nan, np.float32)
    else:
        d["m"] = d["v"] = None
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def case_step_ref(name, p, m, v, k=0, **kw):
    """k4_ref of step k of a case from the given state (the case's own inputs for k = 0)."""
    d = k4_inputs(name)
    c = d["case"]
    return k4_ref(p, d["g"], m, v, c.mode, c.lr, c.b1, c.b2, c.eps, c.step + k, c.clip, c.scale, c.P, **kw)


@functools.lru_cache(maxsize=None)
def k4_case_ref(name):
    """The reference of a case's first step (shared; leave it unchanged)."""
    d = k4_inputs(name)
    return case_step_ref(name, d["p"], d["m"], d["v"])


# ---------------------------------------------------------------------------------------------------------------------------------
# Epilogue cases: (n, nparts, P). n = 1581 (and 3, 62) takes partial_reduce_block's scalar path, 7500 the float4 path with a last block of
# 12 elements, 64 exactly one block; nparts 1 / 5 leave most of the 16 slices empty, 16 / 17 sit on the slice stride, 512 is the most the
# grid argument allows.
# ---------------------------------------------------------------------------------------------------------------------------------
EPI_N = (3, 62, 64, 1581, 7500)
EPI_NPARTS = (1, 5, 16, 17, 64, 512)
EPI_CASES = [(n, q, 1) for n in EPI_N for q in EPI_NPARTS] + [(3, 1, 3), (62, 5, 3), (64, 16, 3), (1581, 17, 3), (7500, 64, 3), (3, 512, 3)]
EPI_WIDE = (1581, 17, 3)  # also run off the grid: randn * 10^U(-6, 2)
EPI_UPDATE = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-6, step=2)  # the fused K4 of the *_update forms (no clip, scale 1: the entry points' own)


@functools.lru_cache(maxsize=None)
def epi_inputs(n, nparts, P, wide=False):
    """dict(partials [P*nparts, n], scalars [P, 8], p, m, v [P, n]), read-only fp32. Grid partials: randn * 10^U(-5, 1.8) clipped to +-64 and
    rounded to a multiple of 2^-20 (seven decades of magnitudes, so the one fp32 rounding of a sum is a real one)."""
    rs = np.random.RandomState(7 * n + 13 * nparts + P + (1000 if wide else 0))
    rows = P * nparts
    if wide:
        x = rs.standard_normal((rows, n)) * 10.0 ** rs.uniform(-6, 2, (rows, n))
    else:
        x = np.clip(rs.standard_normal((rows, n)) * 10.0 ** rs.uniform(-5, 1.8, (rows, n)), -64.0, 64.0)
        x = np.round(x * 2.0 ** 20) / 2.0 ** 20
    d = dict(partials=x.astype(np.float32), scalars=rs.standard_normal((P, 8)).astype(np.float32), p=patch_values(rs, n, P))
    d["m"], d["v"] = moments(rs, n, P)
    for a in d.values():
        a.setflags(write=False)
    return d
