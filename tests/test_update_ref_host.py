"""The fp64 K4 / epilogue-sum reference (tests/update_ref.py) against independent fp32 implementations, and its bounds against injected faults.
No GPU: what test_gpu_update_ref.py compares the kernels with is checked here on its own, for every case, no element excluded.

The independent implementations take the hyper-parameters as the library's C interface narrows them (fp32 values held in Python floats):
update_ref's docstring says why, and test_double_betas_differ_by_the_narrowing_of_one_minus_beta states what the un-narrowed doubles cost."""
import math

import numpy as np
import pytest
import torch

import update_ref as R
from oracle import c_oracle, ref_port
from patch_grad_ref import fma32

CASES = sorted(R.K4_CASES)
F = np.float32


def _n32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------------------------
# input conditions of the case table
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_case_inputs_meet_the_reference_conditions(name):
    """No clip coefficient within its error of 1, nothing non-zero below 2^-100, fl(g scale coef) == 0 only where g == 0, the stated patch
    / gradient edges present."""
    d, ref = R.k4_inputs(name), R.k4_case_ref(name)
    c, meta = d["case"], ref["meta"]
    assert not meta["near"].any() and meta["coef_margin"].min() > 100, meta["coef_margin"]
    assert meta["min_nonzero"] > R.TINY and meta["sign_kept"], meta["min_nonzero"]
    k = min(100, d["n"] // 3)
    assert np.all(d["p"][:, :k] == 0) and np.all(d["p"][:, k : 2 * k] == 1) and d["p"].min() >= 0 and d["p"].max() <= 1
    assert np.all(d["g"][:, ::97] == 0) and np.count_nonzero(d["g"]) == d["g"].size - c.P * len(range(0, d["n"], 97))
    if c.P == 3 and c.clip > 0:  # one group unclipped, the others far below 1
        assert ref["coef"].value[0] == 1.0 and ref["coef"].bound[0] == 0.0 and np.all(ref["coef"].value[1:] < 0.5), ref["coef"].value
    if c.mode == "adamw" and c.lr > 0:  # outward pushes at both ends of [0, 1] exist (n = 3 has one element at each end)
        up = -np.sign(ref["m"].value)
        assert d["n"] < 300 or (np.any((d["p"] == 0) & (up < 0)) and np.any((d["p"] == 1) & (up > 0)))


def test_case_table_covers_every_axis_per_form():
    for form in set(R.FORM.values()):
        cs = [c for n, c in R.K4_CASES.items() if R.FORM[n.split("-")[0]] == form]
        assert {c.P for c in cs} == {1, 3} and {c.mode for c in cs} == {"adamw", "pgd"} and {c.step for c in cs} >= {1, 2, 1000}
        assert {(c.b1, c.b2, c.eps) for c in cs} >= {(0.9, 0.999, 1e-6), (0.8, 0.99, 1e-8), (0.9, 0.999, 1e-3)}
        assert {c.lr for c in cs} == {2e-3, 0.0} and {c.scale for c in cs} == {1.0, 0.25} and {c.moments for c in cs} >= {"zero", "nonzero", "nan"}
        assert any(not c.stats for c in cs) and any(c.chain == 3 for c in cs) and any(c.clip > 0 and c.scale == 0.25 for c in cs)
    assert sorted(int(np.prod(s)) for s in R.SHAPES.values()) == [3, 1581, 8192, 8427, 32768, 33075]


# ---------------------------------------------------------------------------------------------------------------------------------
# independent fp32 implementations inside the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _torch_route(d, g):
    """One group through torch: the scale, clip_grad_norm_ (L1), then ref_port.HFAdamW + clamp or ref_port.pgd_step. -> p, m, v, norm."""
    c = d["case"]
    prm = torch.nn.Parameter(torch.from_numpy(d["p"][g].copy()))
    prm.grad = torch.from_numpy(d["g"][g].copy()) * _n32(c.scale)
    norm = None
    if c.clip > 0:
        norm = float(torch.nn.utils.clip_grad_norm_([prm], _n32(c.clip), norm_type=1))
    if c.mode == "pgd":
        return ref_port.pgd_step(prm.data, prm.grad, _n32(c.lr)).numpy(), None, None, norm
    opt = ref_port.HFAdamW([prm], lr=_n32(c.lr), betas=(_n32(c.b1), _n32(c.b2)), eps=_n32(c.eps))
    st = opt.state[prm]
    st["step"], st["exp_avg"], st["exp_avg_sq"] = c.step - 1, torch.from_numpy(d["m"][g].copy()), torch.from_numpy(d["v"][g].copy())
    opt.step()
    return prm.data.clamp(0, 1).numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), norm


@pytest.mark.parametrize("name", CASES)
def test_torch_optimiser_route_inside_the_bound(name):
    """ref_port.HFAdamW + clamp, torch's clip_grad_norm_(norm_type=1) and ref_port.pgd_step. clip_grad_norm_ adds its norm in fp32: the
    coefficient's bound carries its own summation term (n - 1) u (recursive summation's; torch's blocked sum is inside it)."""
    d = R.k4_inputs(name)
    c = d["case"]
    adam = c.mode == "adamw"
    ref = R.case_step_ref(name, d["p"], d["m"], d["v"], coef_extra_rel=(d["n"] - 1) * R.U if c.clip > 0 else 0.0)
    assert not ref["meta"]["near"].any()
    got = [_torch_route(d, g) for g in range(c.P)]
    r = {"patch": R.compare(ref["patch"], np.stack([x[0] for x in got]), f"{name} patch")}
    if adam:
        r["m"] = R.compare(ref["m"], np.stack([x[1] for x in got]), f"{name} m")
        r["v"] = R.compare(ref["v"], np.stack([x[2] for x in got]), f"{name} v")
    if c.clip > 0:  # the norm it returns is sum |g scale|
        S = ref["stats"].value[:, 0]
        assert np.all(np.abs(np.array([x[3] for x in got]) - S) <= R.SAFETY * d["n"] * R.U * S)
    print(name, {k: float(f"{v:.3g}") for k, v in r.items()})


@pytest.mark.parametrize("name", CASES)
def test_c_oracle_inside_the_bound(name):
    """oracle/vaa_oracle.c's patch_update, group by group: plain fp32 C, no FMA, p - step_size (m / den): every element inside the bound."""
    d, ref = R.k4_inputs(name), R.k4_case_ref(name)
    c = d["case"]
    adam = c.mode == "adamw"
    p = d["p"].copy()
    m, v = (d["m"].copy(), d["v"].copy()) if adam else (np.zeros_like(p), np.zeros_like(p))
    l1 = [c_oracle.patch_update(p[g], d["g"][g].copy(), m[g], v[g], 0 if adam else 1, c.lr, c.step, c.b1, c.b2, c.eps, c.clip, c.scale) for g in range(c.P)]
    r = {"patch": R.compare(ref["patch"], p, f"{name} patch"), "sum|g|": R.compare(R.Ref(ref["stats"].value[:, 0], ref["stats"].bound[:, 0]), l1, f"{name} sum|g|")}
    if adam:
        r["m"], r["v"] = R.compare(ref["m"], m, f"{name} m"), R.compare(ref["v"], v, f"{name} v")
    print(name, {k: float(f"{v:.3g}") for k, v in r.items()})


def test_double_betas_differ_by_the_narrowing_of_one_minus_beta():
    """transformers' AdamW keeps the betas as Python doubles: torch narrows 1 - b2 = 0.001 itself, the library forms 1 - fl32(0.999). With zero
    moments v' = (1 - b2) g^2, so HFAdamW with the doubles leaves the v bound by exactly that factor — and by nothing else."""
    d = R.k4_inputs("r8_n1581-adam_first")
    ref = R.k4_case_ref("r8_n1581-adam_first")
    prm = torch.nn.Parameter(torch.from_numpy(d["p"][0].copy()))
    prm.grad = torch.from_numpy(d["g"][0].copy())
    opt = ref_port.HFAdamW([prm], lr=2e-3)
    opt.step()
    v = opt.state[prm]["exp_avg_sq"].numpy().astype(np.float64)
    want = float(F(1.0 - 0.999)) / (1.0 - float(F(0.999)))
    assert abs(want - 1) == pytest.approx(1.29e-5, rel=0.01)
    assert R.outside(ref["v"], v) > 0.9
    nz = ref["v"].value[0] > 0
    assert np.all(np.abs(v[nz] / ref["v"].value[0][nz] / want - 1) <= 4 * R.U)


# ---------------------------------------------------------------------------------------------------------------------------------
# injected faults: a numpy fp32 emulation of patch_update_body / update_one, each fault outside the bound
# ---------------------------------------------------------------------------------------------------------------------------------
def emu_k4(d, fault=None):
    """fp32, operation by operation as the kernel (module docstring of update_ref). -> dict(patch, m, v, stats)."""
    c = d["case"]
    P, n = c.P, d["n"]
    lr, b1, b2, eps, clip, scale = (F(x) for x in (c.lr, c.b1, c.b2, c.eps, c.clip, c.scale))
    if fault == "beta2_fixed":
        b2 = F(0.999)
    if fault == "beta1_fixed":
        b1 = F(0.9)
    if fault == "eps_fixed":
        eps = F(1e-6)
    omb1, omb2 = F(1.0 - float(b1)), F(1.0 - float(b2))
    bc1, bc2 = 1.0 - float(b1) ** c.step, 1.0 - float(b2) ** c.step
    ss = F(float(lr) * math.sqrt(bc2) / bc1)
    g, p = d["g"], d["p"]
    g0 = g * scale
    ta, ts = np.abs(g0.astype(np.float64)).sum(axis=1), g0.astype(np.float64).sum(axis=1)
    coef = np.ones(P, F)
    if clip > 0:
        tc = np.abs(g.astype(np.float64)).sum(axis=1) if fault == "coef_unscaled" else ta
        coef = np.minimum(clip / (tc.astype(F) + F(1e-6)), F(1.0)).astype(F)
    if fault == "coef_other_group":
        coef = np.roll(coef, 1)
    G = g0 * coef[:, None]
    s0 = np.abs(G.astype(np.float64)).sum(axis=1) if fault == "stats_after_clip" else ta
    stats = np.stack([s0.astype(F), (ts / (P * n if fault == "mean_over_Pn" else n)).astype(F)], axis=1)
    out = dict(stats=stats, m=None, v=None)
    if c.mode == "adamw":
        m = fma32(G, omb1, d["m"] * b1)
        v = d["v"] * b2 + (omb2 * G) * G
        if fault == "eps_in_sqrt":
            pn = p + ((-ss) * m) / np.sqrt(v + eps)
        elif fault == "eps_after_bias_correction":  # torch.optim.AdamW: sqrt(v) / sqrt(bc2) + eps, lr / bc1
            pn = p + ((-F(float(lr) / bc1)) * m) / (np.sqrt(v) / F(math.sqrt(bc2)) + eps)
        elif fault == "no_bias_correction":
            pn = p + ((-lr) * m) / (np.sqrt(v) + eps)
        else:
            pn = p + ((-ss) * m) / (np.sqrt(v) + eps)
        out["m"], out["v"] = m, v
    else:
        pn = p - lr * np.sign(G)
    out["patch"] = pn if fault == "no_clamp" else np.minimum(F(1.0), np.maximum(F(0.0), pn))
    assert all(a is None or a.dtype == F for a in out.values())
    return out


@pytest.mark.parametrize("name", CASES)
def test_emulation_inside_the_bound(name):
    """The emulation without a fault is what the kernel is meant to compute: inside every bound, at every element of every case."""
    d, ref = R.k4_inputs(name), R.k4_case_ref(name)
    got = emu_k4(d)
    r = {k: R.compare(ref[k], got[k], f"{name} {k}") for k in ("patch", "m", "v", "stats") if ref[k] is not None}
    print(name, {k: float(f"{v:.3g}") for k, v in r.items()})


# fault -> (output it shows in, cases that must catch it, least fraction of that output's elements outside the bound in the FIRST case; every
# listed case must catch it in at least one element)
FAULTS = {
    "eps_in_sqrt": ("patch", ["r8_n8192-adam_first", "stream_n33075-adam_betas_clip"], 0.6),
    "eps_after_bias_correction": ("patch", ["r8_n8192-adam_first", "r32_n8427-adam_betas_clip"], 0.6),
    "no_bias_correction": ("patch", ["r8_n8192-adam_first", "r32_n32768-adam_betas_clip"], 0.6),
    "beta2_fixed": ("v", ["r8_n1581-adam_betas_clip"], 0.6),
    "beta1_fixed": ("m", ["r8_n1581-adam_betas_clip"], 0.6),
    "eps_fixed": ("patch", ["r8_n1581-adam_betas_clip", "r8_n1581-adam_eps_late"], 0.3),
    "coef_unscaled": ("m", ["r8_n1581-adam_betas_clip", "r32_n8427-adam_betas_clip"], 0.3),
    "coef_other_group": ("m", ["r8_n1581-adam_betas_clip", "r8_n1581-adam_chain"], 0.3),
    "no_clamp": ("patch", ["r8_n1581-adam_first", "r8_n1581-pgd_plain"], 0.0),
    "stats_after_clip": ("stats", ["r8_n1581-adam_betas_clip", "r8_n1581-pgd_clip_nan"], 0.0),
    "mean_over_Pn": ("stats", ["r8_n1581-adam_betas_clip", "stream_n33075-pgd_clip_nan"], 0.0),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_injected_fault_breaks_the_bound(fault):
    out, names, least = FAULTS[fault]
    for i, name in enumerate(names):
        ref = R.k4_case_ref(name)
        frac = R.outside(ref[out], emu_k4(R.k4_inputs(name), fault)[out])
        print(f"{fault} on {name}: {100 * frac:.1f} % of {out} outside the bound")
        assert frac > (least if i == 0 else 0.0), (fault, name, frac)


# ---------------------------------------------------------------------------------------------------------------------------------
# the epilogue's sum
# ---------------------------------------------------------------------------------------------------------------------------------
def emu_sum(partials, P, fault=None, k=0):
    """partial_reduce_block's order: 16 interleaved slices (p = s, s + 16, ...) in fp64, then slice 0..15, then one fp32 rounding."""
    a = partials.astype(np.float64).reshape(P, -1, partials.shape[1])
    nparts, n = a.shape[1], a.shape[2]
    if fault == "skip_tile":
        a = np.delete(a, k, axis=1)
        nparts -= 1
    t = np.zeros((P, n))
    for s in range(16):
        acc = np.zeros((P, n))
        for q in range(s, nparts, 16):
            acc = acc + a[:, q]
        t = t + acc
    out = t.astype(F)
    if fault == "drop_tail" and n % 4:
        out[:, n - n % 4 :] = 0
    return out


def test_epilogue_case_table_covers_every_axis():
    ns, qs, Ps = zip(*R.EPI_CASES)
    assert set(ns) == set(R.EPI_N) and set(qs) == set(R.EPI_NPARTS) and set(Ps) == {1, 3}
    assert (1581, 17, 3) in R.EPI_CASES and (7500, 512, 1) in R.EPI_CASES and R.EPI_WIDE in R.EPI_CASES
    assert 1581 % 4 != 0 and 7500 % 4 == 0 and 7500 % 64 == 12 and max(qs) <= 512


@pytest.mark.parametrize("n,nparts,P", R.EPI_CASES)
def test_grid_partials_sum_exactly_in_any_order(n, nparts, P):
    """On the grid the fp64 sum is exact: ascending, descending and the kernel's two-level order agree with math.fsum bit for bit, so
    np.float32(value) is THE correctly rounded result."""
    d = R.epi_inputs(n, nparts, P)
    x = d["partials"]
    assert np.abs(x).max() <= 64 and np.all(x.astype(np.float64) * 2.0 ** 20 == np.round(x.astype(np.float64) * 2.0 ** 20)) and nparts <= 512
    ref = R.epilogue_sum_ref(x, P)
    a = x.astype(np.float64).reshape(P, nparts, n)
    fwd, bwd = np.zeros((P, n)), np.zeros((P, n))
    for q in range(nparts):
        fwd, bwd = fwd + a[:, q], bwd + a[:, nparts - 1 - q]
    assert np.array_equal(fwd, ref.value) and np.array_equal(bwd, ref.value)
    cols = np.random.RandomState(n + nparts).choice(P * n, min(P * n, 64), replace=False)  # math.fsum on a sample of the columns
    for e in cols:
        g, i = divmod(int(e), n)
        assert math.fsum(a[g, :, i].tolist()) == ref.value[g, i]
    assert np.array_equal(emu_sum(x, P), ref.value.astype(F))


def test_wide_partials_inside_the_bound():
    n, nparts, P = R.EPI_WIDE
    x = R.epi_inputs(n, nparts, P, wide=True)["partials"]
    ref = R.epilogue_sum_ref(x, P, wide=True)
    assert R.compare(ref, emu_sum(x, P), "wide") <= 1.0
    exact = np.array([[math.fsum(x[g * nparts : (g + 1) * nparts, i].astype(np.float64).tolist()) for i in range(0, n, 37)] for g in range(P)])
    assert R.compare(R.Ref(ref.value[:, ::37], ref.bound[:, ::37]), exact.astype(F), "wide fsum") <= 1.0


@pytest.mark.parametrize("k", [0, 15, 16, -1])
def test_skipped_tile_is_seen(k):
    """One partial tile left out of the sum (the first, the last of the first stride, the first of the second, the last): on the grid the
    result differs from np.float32(sum) wherever that tile is non-zero after rounding — in most elements."""
    for n, nparts, P in [(1581, 17, 3), (7500, 512, 1), (64, 17, 1)]:
        x = R.epi_inputs(n, nparts, P)["partials"]
        want = R.epilogue_sum_ref(x, P).value.astype(F)
        assert np.mean(emu_sum(x, P, "skip_tile", k % nparts) != want) > 0.5


def test_dropped_tail_is_seen():
    for n, nparts, P in [(1581, 17, 3), (62, 5, 3), (3, 1, 1)]:
        x = R.epi_inputs(n, nparts, P)["partials"]
        want = R.epilogue_sum_ref(x, P).value.astype(F)
        got = emu_sum(x, P, "drop_tail")
        assert np.array_equal(got[:, : n - n % 4], want[:, : n - n % 4]) and np.any(got[:, n - n % 4 :] != want[:, n - n % 4 :])
