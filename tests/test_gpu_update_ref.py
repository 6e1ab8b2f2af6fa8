"""GPU tests of K4 (vaa_patch_update[_seg]) and of the step epilogue's pass-through forms (the gradient sum, the message tail, K4 fused into
the launch) against tests/update_ref.py: the fp64 reference with a bound per output element (its docstring derives the terms).

Every case of update_ref.K4_CASES is one step from stated inputs (`chain` cases: three, each fed with the kernel's own read-back state);
patch, m, v and stats go through update_ref.compare element by element, none excluded. Every buffer is a view inside a NaN-filled allocation
with 32 guard elements on either side, which must be intact afterwards. The epilogue's msg on the grid of update_ref.epi_inputs must EQUAL
np.float32(fp64 sum); its fused K4 is checked against k4_ref fed with the kernel's own msg.
Combinations that do not exist (not generated, nothing is skipped): step_epilogue x P = 3 (vaa_step_epilogue[_update] has one group).
The epilogue's fold (rowmap given) is test_gpu_loss_ref.py's; multi-step trajectories and the bit-for-bit equality of the forms are
test_gpu_kernels.py's / test_gpu_sweep.py's.

Worst error / bound per (form, output), measured on an MI355X (pytest -s prints them; the host test's fp32 emulation of update_one gives the
same figures, and the first-order bound is attained to a half by construction of SAFETY = 2):
    K4 4 workgroups (R = 8)     patch 0.498   m 0.475   v 0.469   stats 0.454
    K4 16 workgroups (R = 32)   patch 0.500   m 0.480   v 0.479   stats 0.368
    K4 streaming (R = 0)        patch 0.499   m 0.484   v 0.481   stats 0.390
    epilogue, _seg, _seg_tail   msg on the grid: equal to np.float32(fp64 sum) at every element; off the grid (_seg, _seg_tail) 0.991 of
                                u |value| + nparts 2^-52 sum |partial|, i.e. of half an ulp
      with update=              patch 0.495   m 0.409   v 0.469   stat_part 0 (equal to the fp64 block sums)
                                last_stats 0.288 (epilogue), 0.441 (_seg), 0.264 (_seg_tail)
"""
import numpy as np
import pytest
import torch

import update_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 32

WORST = {}  # (form, output) -> worst error / bound seen in this session (printed by the tests: pytest -s)


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _guarded(a, dtype=torch.float32):
    """np array -> (contiguous view of its shape holding it, the NaN-filled allocation of a.size + 64 elements around the view)."""
    a = np.array(a, order="C")  # a copy: the case table's arrays are read-only
    alloc = torch.full((a.size + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    view = alloc[GUARD : GUARD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a).to(dtype))
    return view, alloc


def _guards_intact(alloc, what):
    g = torch.cat([alloc[:GUARD], alloc[-GUARD:]]).cpu().numpy()
    want = np.full(1, np.nan, g.dtype).view(np.uint32 if g.dtype == np.float32 else np.uint64)[0]
    assert np.all(g.view(want.dtype) == want), f"{what}: guard elements around the buffer were written"


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint32)


def _np(t, P):
    return t.detach().cpu().numpy().reshape(P, -1)


def _track(form, out, ref, got, tag):
    r = R.compare(ref, got, f"{form} {tag} {out}")
    WORST[(form, out)] = max(WORST.get((form, out), 0.0), r)


def _report(prefix):
    print("worst error / bound so far:", {f"{k[0]} {k[1]}": float(f"{v:.3g}") for k, v in sorted(WORST.items()) if k[0].startswith(prefix)})


def _sync(ops):
    torch.cuda.synchronize()
    ops.async_error_check()


# ---------------------------------------------------------------------------------------------------------------------------------
# K4
# ---------------------------------------------------------------------------------------------------------------------------------
def _k4_call(ops, c, P, p, g, m, v, step, clip=None):
    mode = ops.OPT_ADAMW_HF if c.mode == "adamw" else ops.OPT_PGD_SIGN
    clip = c.clip if clip is None else clip
    if P == 1:
        return ops.patch_update(p, g, m, v, mode, c.lr, step, c.b1, c.b2, c.eps, clip, c.scale, c.stats)
    return ops.patch_update_seg(p, g, m, v, P, mode, c.lr, step, c.b1, c.b2, c.eps, clip, c.scale, c.stats)


@pytest.mark.parametrize("name", sorted(R.K4_CASES))
def test_k4_every_form_vs_fp64_reference(ops, name):
    """vaa_patch_update (P = 1) / vaa_patch_update_seg (P = 3): patch, m, v, stats inside their bounds at every element; the patch in [0, 1];
    lr = 0 and PGD's zero-gradient elements leave the patch bit for bit; PGD leaves NaN-filled m / v untouched; the group whose clip
    coefficient is 1 is bit for bit the unclipped call on that group; the guard elements are intact."""
    d = R.k4_inputs(name)
    c, P, n = d["case"], d["case"].P, d["n"]
    form = R.FORM[name.split("-")[0]]
    adam = c.mode == "adamw"
    shape = ((P,) if P > 1 else ()) + tuple(c.shape)
    p, pa = _guarded(d["p"].reshape(shape))
    g, ga = _guarded(d["g"].reshape(shape))
    m, ma = _guarded(d["m"].reshape(shape)) if d["m"] is not None else (None, None)
    v, va = _guarded(d["v"].reshape(shape)) if d["v"] is not None else (None, None)
    p0, m0, v0 = d["p"], d["m"], d["v"]
    for k in range(c.chain):
        ref = R.k4_case_ref(name) if k == 0 else R.case_step_ref(name, p0, m0, v0, k)
        stats = _k4_call(ops, c, P, p, g, m, v, c.step + k)
        _sync(ops)
        tag = f"{name} step {c.step + k}"
        p1 = _np(p, P)
        _track(form, "patch", ref["patch"], p1, tag)
        assert p1.min() >= 0.0 and p1.max() <= 1.0
        if adam:
            m1, v1 = _np(m, P), _np(v, P)
            _track(form, "m", ref["m"], m1, tag)
            _track(form, "v", ref["v"], v1, tag)
            if c.lr == 0:
                assert np.array_equal(_bits(p1), _bits(p0)), "lr = 0 moved the patch"
                assert not np.array_equal(m1, m0) and not np.array_equal(v1, v0)
        else:
            z = d["g"] == 0
            assert np.array_equal(_bits(p1[z]), _bits(p0[z])), "PGD moved an element whose gradient is +-0"
            if m is not None:
                assert np.array_equal(_bits(m), _bits(m0)) and np.array_equal(_bits(v), _bits(v0)), "PGD touched m / v"
            m1 = v1 = None
        if c.stats:
            _track(form, "stats", ref["stats"], stats.cpu().numpy().reshape(P, 2), tag)
        else:
            assert stats is None
        assert np.array_equal(_bits(g), _bits(d["g"])), "the gradient was written"
        for al, what in ((pa, "patch"), (ga, "grad"), (ma, "m"), (va, "v")):
            if al is not None:
                _guards_intact(al, f"{tag} {what}")
        if k == 0 and P == 3 and c.clip > 0:  # group 0: coef = 1 -> bit for bit the call without the clip on that group alone
            assert ref["coef"].value[0] == 1.0
            q, _ = _guarded(d["p"][0].reshape(c.shape))
            gq, _ = _guarded(d["g"][0].reshape(c.shape))
            mq, vq = (_guarded(a[0].reshape(c.shape))[0] for a in (d["m"], d["v"])) if d["m"] is not None else (None, None)
            sq = _k4_call(ops, c, 1, q, gq, mq, vq, c.step, clip=0.0)
            _sync(ops)
            assert np.array_equal(_bits(q), _bits(p1[0])), "coef = 1 group differs from the unclipped call"
            if adam:
                assert np.array_equal(_bits(mq), _bits(m1[0])) and np.array_equal(_bits(vq), _bits(v1[0]))
            if c.stats:
                assert np.array_equal(_bits(sq), _bits(stats.reshape(P, 2)[0]))
        p0, m0, v0 = p1, m1, v1
    _report("K4")


# ---------------------------------------------------------------------------------------------------------------------------------
# step epilogue, pass-through forms
# ---------------------------------------------------------------------------------------------------------------------------------
def _epi_call(ops, form, partials, msg, scalars, P, update):
    if form == "epilogue":
        ops.step_epilogue(partials, msg, scalars, update=update)
    elif form == "epilogue_seg":
        ops.step_epilogue_seg(partials, msg, scalars, P, update=update)
    else:
        ops.step_epilogue_seg_tail(partials, msg, scalars, P, update=update)


def _epi_tail(form, scalars, P):
    if form == "epilogue_seg":
        return np.zeros((P, 4), np.float32)
    return scalars.reshape(P, 8)[:, [1, 2, 7, 0]]


def _check_msg(form, d, sref, wide, msg, P, n, tag):
    got = msg.cpu().numpy()
    if wide:
        _track(form, "msg", sref, got[: P * n], tag)
    else:
        assert np.array_equal(got[: P * n].reshape(P, n), sref.value.astype(np.float32)), f"{form} {tag}: msg is not the correctly rounded sum"
        WORST.setdefault((form, "msg"), 0.0)
    assert np.array_equal(_bits(got[P * n :]), _bits(_epi_tail(form, d["scalars"], P))), f"{form} {tag}: message tail"
    return got[: P * n].reshape(P, n)


def _run_epilogue(ops, form, n, nparts, P, wide, mode):
    d = R.epi_inputs(n, nparts, P, wide)
    sref = R.epilogue_sum_ref(d["partials"], P, wide)
    tag = f"n={n} nparts={nparts} P={P}{' wide' if wide else ''} {mode or 'plain'}"
    partials, parta = _guarded(d["partials"])
    scal_np = d["scalars"][0] if form == "epilogue" else d["scalars"]
    scalars, scala = _guarded(scal_np)
    msg, msga = _guarded(np.full(P * (n + 4), np.nan, np.float32))
    bufs = [(parta, "partials"), (scala, "scalars"), (msga, "msg")]
    update = None
    if mode is not None:
        adam = mode == "adamw"
        p, pa = _guarded(d["p"])
        m, ma = _guarded(d["m"]) if adam else _guarded(np.full((P, n), np.nan, np.float32))
        v, va = _guarded(d["v"]) if adam else _guarded(np.full((P, n), np.nan, np.float32))
        nred = (n + 63) // 64
        sp, spa = _guarded(np.full((P * nred, 2), np.nan), torch.float64)
        h = R.EPI_UPDATE
        update = dict(patch=p, m=m, v=v, mode=ops.OPT_ADAMW_HF if adam else ops.OPT_PGD_SIGN, lr=h["lr"], step=h["step"], beta1=h["b1"], beta2=h["b2"],
                      eps=h["eps"], stat_part=sp)
        bufs += [(pa, "patch"), (ma, "m"), (va, "v"), (spa, "stat_part")]
    _epi_call(ops, form, partials, msg, scalars, P, update)
    _sync(ops)
    gmsg = _check_msg(form, d, sref, wide, msg, P, n, tag)
    assert np.array_equal(_bits(partials), _bits(d["partials"])) and np.array_equal(_bits(scalars), _bits(scal_np))
    if mode is not None:
        uform = form + " update"
        ref = R.k4_ref(d["p"], gmsg, d["m"] if adam else None, d["v"] if adam else None, mode, h["lr"], h["b1"], h["b2"], h["eps"], h["step"], 0.0, 1.0, P)
        assert ref["meta"]["min_nonzero"] > R.TINY
        p1 = _np(p, P)
        _track(uform, "patch", ref["patch"], p1, tag)
        assert p1.min() >= 0.0 and p1.max() <= 1.0
        if adam:
            _track(uform, "m", ref["m"], _np(m, P), tag)
            _track(uform, "v", ref["v"], _np(v, P), tag)
        else:
            assert np.isnan(_np(m, P)).all() and np.isnan(_np(v, P)).all(), "PGD touched m / v"
        # stat_part: every block's {sum |g|, sum g} over its 64 elements of the kernel's own msg
        pad = np.zeros((P, nred * 64))
        pad[:, :n] = gmsg
        blocks = pad.reshape(P * nred, 64)
        want = np.stack([np.abs(blocks).sum(axis=1), blocks.sum(axis=1)], axis=1)
        tol = 64 * 2.0 ** -52 * want[:, :1]
        sp_np = sp.cpu().numpy()
        assert np.all(np.abs(sp_np - want) <= tol), f"{uform} {tag}: stat_part"
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(sp_np == want, 0.0, np.abs(sp_np - want) / tol).max()
        WORST[(uform, "stat_part")] = max(WORST.get((uform, "stat_part"), 0.0), float(r))
    for al, what in bufs:
        _guards_intact(al, f"{form} {tag} {what}")


@pytest.mark.parametrize("n,nparts,P", R.EPI_CASES)
def test_epilogue_sum_tail_and_fused_k4_vs_fp64_reference(ops, n, nparts, P):
    """vaa_step_epilogue (P = 1), vaa_step_epilogue_seg (zero tail) and vaa_step_epilogue_seg_tail, each plain and with the AdamW and the PGD
    update fused: msg equals the correctly rounded fp64 sum, the tail is exact, patch / m / v are inside k4_ref's bounds for the kernel's
    own msg, every stat_part row is the fp64 sum of its block."""
    forms = (["epilogue"] if P == 1 else []) + ["epilogue_seg", "epilogue_seg_tail"]
    for wide in (False, True) if (n, nparts, P) == R.EPI_WIDE else (False,):
        for form in forms:
            for mode in (None, "adamw", "pgd"):
                _run_epilogue(ops, form, n, nparts, P, wide, mode)
    _report("epilogue")


@pytest.mark.parametrize("form,n,nparts,P", [("epilogue", 7500, 512, 1), ("epilogue", 3, 1, 1), ("epilogue_seg", 1581, 17, 3), ("epilogue_seg_tail", 62, 5, 3)])
def test_fused_step_last_stats_vs_fp64_reference(ops, form, n, nparts, P):
    """PatchOptimizer.last_stats after a fused step (the block sums of stat_part folded on the host) inside k4_ref's stats bound."""
    from roboticattack_amd.optim import PatchOptimizer

    d = R.epi_inputs(n, nparts, P)
    patch = torch.from_numpy(d["p"].copy()).to(DEV)
    opt = PatchOptimizer(patch, lr=2e-3, groups=P)
    partials = torch.from_numpy(d["partials"].copy()).to(DEV)
    scal_np = d["scalars"][0] if form == "epilogue" else d["scalars"]
    msg = torch.full((P * (n + 4),), float("nan"), device=DEV)
    _epi_call(ops, form, partials, msg, torch.from_numpy(scal_np.copy()).to(DEV), P, opt.fused_update_args())
    _sync(ops)
    gmsg = msg[: P * n].cpu().numpy().reshape(P, n)
    ref = R.k4_ref(d["p"], gmsg, np.zeros((P, n), np.float32), np.zeros((P, n), np.float32), "adamw", 2e-3, 0.9, 0.999, 1e-6, 1, 0.0, 1.0, P)
    _track(form + " update", "last_stats", ref["stats"], opt.last_stats.cpu().numpy().reshape(P, 2), f"n={n} nparts={nparts} P={P}")
    _track(form + " update", "patch", ref["patch"], _np(patch, P), f"n={n} nparts={nparts} P={P} optimiser")
    _report("epilogue")
