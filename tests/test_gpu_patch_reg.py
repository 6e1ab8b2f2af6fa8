"""GPU tests of the patch regulariser (K6: total variation + non-printability score): the kernel through ops against the fp64 restatement of
include/vaa.h's definition (tests/patch_reg_ref.py: values by tensor ops, gradient by autograd), its bitwise promises (accumulate form, values-only
form, repeatability), the NaN rule, and the four attack loops with the weights on and off.

Bounds are derived, not guessed (patch_reg_ref.tolerances): eight times the error of the fp32 restatement against the fp64 one on the same inputs,
with floors that follow from the number of fp32 roundings; the kernel is never compared with itself. Near a tie of two palette colours the argmin
may legitimately differ: a texel's gradient may point to any colour within 2e-6 (fp64) of its minimum; no texel is left out."""
import types

import numpy as np
import pytest
import torch

import patch_reg_ref as ref
from roboticattack_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(c):
    return c["patch"].to(DEV), c["palette"].to(DEV)


def _values(part, n3):
    from roboticattack_amd import ops

    tv, nps = ops.patch_reg_values(part, n3)
    assert tv.dtype == torch.float64 and tv.is_cuda and nps.dtype == torch.float64 and nps.is_cuda
    return float(tv), float(nps)


@pytest.mark.parametrize("name", ref.CASES)
def test_values_and_gradient_vs_fp64(name):
    from roboticattack_amd import _lib, ops

    c = ref.case(name)
    t_tv, t_nps, t_g = ref.tolerances(name)
    patch, pal = _dev(c)
    g, part = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS)
    assert tuple(part.shape) == (_lib.lib().vaa_patch_reg_parts(int(patch.shape[1]), int(patch.shape[2])), 2)
    tv, nps = _values(part, patch.numel())
    err, gmax = ref.grad_error(g.cpu(), c["patch"], c["palette"], ref.W_TV, ref.W_NPS, c["grad64"])
    print(f"{name}: |tv - fp64| = {abs(tv - c['tv64']):.3e} (e_ref {c['e_tv']:.3e}, tol {t_tv:.3e}); |nps - fp64| = {abs(nps - c['nps64']):.3e} "
          f"(e_ref {c['e_nps']:.3e}, tol {t_nps:.3e}); gradient {err / gmax:.3e} of max|ref| (e_ref {c['e_grad_rel']:.3e}, tol {t_g:.3e})")
    assert abs(tv - c["tv64"]) <= t_tv and abs(nps - c["nps64"]) <= t_nps
    assert err <= t_g * gmax


@pytest.mark.parametrize("name", ["50x50-grid27", "17x23-rand64", "17x23-rand64-q8", "1x1-k1"])
def test_bitwise_promises(name):
    """The accumulate form is g + r with ONE rounded add of the write form's r; the values-only form and the accumulate form write the write
    form's `part` bits; a second identical call gives identical bits."""
    from roboticattack_amd import ops

    patch, pal = _dev(ref.case(name))
    r, part = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS)
    r2, part2 = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS)
    assert torch.equal(r.view(torch.int32), r2.view(torch.int32)) and torch.equal(part.view(torch.int64), part2.view(torch.int64))
    g = torch.randn(patch.shape, generator=torch.Generator().manual_seed(9)).to(DEV) * float(r.abs().max())
    acc = g.clone()
    out, part_acc = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS, grad=acc, accumulate=True)
    assert out is acc and torch.equal(acc.view(torch.int32), (g + r).view(torch.int32)) and not torch.equal(acc, g)
    assert torch.equal(part_acc.view(torch.int64), part.view(torch.int64))
    none, part_v = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS, want_grad=False)
    assert none is None and torch.equal(part_v.view(torch.int64), part.view(torch.int64))
    given = torch.full_like(patch, 7.0)  # a given buffer without `accumulate` is overwritten
    ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS, grad=given)
    assert torch.equal(given.view(torch.int32), r.view(torch.int32))


@pytest.mark.parametrize("name", ["50x50-grid27", "17x23-rand64-q8", "7x1-k1"])
def test_single_terms(name):
    """w_tv = 0: the NPS-only gradient; w_nps = 0 with no palette at all: the TV-only gradient (an NPS value of 0)."""
    from roboticattack_amd import ops

    c = ref.case(name)
    _, _, t_g = ref.tolerances(name)
    patch, pal = _dev(c)
    g, part = ops.patch_reg_grad(patch, pal, 0.0, ref.W_NPS)
    err, gmax = ref.grad_error(g.cpu(), c["patch"], c["palette"], 0.0, ref.W_NPS)
    assert gmax > 0 and err <= t_g * gmax
    assert abs(_values(part, patch.numel())[1] - c["nps64"]) <= ref.tolerances(name)[1]
    g, part = ops.patch_reg_grad(patch, None, ref.W_TV, 0.0)
    err, gmax = ref.grad_error(g.cpu(), c["patch"], None, ref.W_TV, 0.0)
    assert gmax > 0 and err <= t_g * gmax
    tv, nps = _values(part, patch.numel())
    assert abs(tv - c["tv64"]) <= ref.tolerances(name)[0] and nps == 0.0


def test_zero_differences_have_zero_sign():
    """A patch quantised to multiples of 1/8 has many exactly-zero differences: sgn(0) = 0, so the TV gradient is an exact multiple of c_tv there
    (a constant patch: exactly zero everywhere)."""
    from roboticattack_amd import ops

    flat = torch.full((3, 17, 23), 0.375, device=DEV)
    g, part = ops.patch_reg_grad(flat, None, ref.W_TV, 0.0)
    assert bool((g == 0).all()) and _values(part, flat.numel()) == (0.0, 0.0)
    c = ref.case("50x50-grid27-q8")
    g, _ = ops.patch_reg_grad(c["patch"].to(DEV), None, 1.0, 0.0)
    want = ref.grad(c["patch"], None, 1.0, 0.0) * c["patch"].numel()  # small integers in fp64
    got = g.cpu().double() / float(np.float32(1.0 / c["patch"].numel()))
    assert torch.equal(got.round(), want) and float((got - want).abs().max()) < 1e-6 and 0.02 < float((want == 0).double().mean())


def test_nan_texel():
    """A NaN texel: NaN at its three gradient elements and in the NPS sum; every element whose texel is neither it nor one of its four neighbours
    stays finite."""
    from roboticattack_amd import ops

    c = ref.case("17x23-grid27")
    patch, pal = _dev(c)
    patch = patch.clone()
    i, j = 5, 7
    patch[1, i, j] = float("nan")
    g, part = ops.patch_reg_grad(patch, pal, ref.W_TV, ref.W_NPS)
    assert bool(torch.isnan(g[:, i, j]).all())
    assert np.isnan(_values(part, patch.numel())[1])
    near = torch.zeros(patch.shape[1:], dtype=torch.bool, device=DEV)
    for a, b in ((i, j), (i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
        near[a, b] = True
    assert bool(torch.isfinite(g[:, ~near]).all())


# ------------------------------------------------------------------------------------------------------
# the attack loops (surrogate model, bs 3, a 3x17x23 patch)
# ------------------------------------------------------------------------------------------------------
class _Fresh:
    def __init__(self, seeds, b):
        self.seeds, self.b = seeds, b

    def __len__(self):
        return len(self.seeds)

    def __iter__(self):
        for s in self.seeds:
            yield synthetic.synth_batch(s, self.b, "smooth")


BS, PATCH = 3, [3, 17, 23]


def _seed():
    import random

    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


def _run_loop(which, tmp_path, monkeypatch, n_it, inner, reg=None, unfused=False, resize_patch=False, colorjitter=False):
    """n_it outer x inner inner steps, seed 42, one validation batch (at outer iteration 0). `reg`: None = the run never mentions the flags, else the
    weights (tv_weight, nps_weight). `unfused`: VAA_FUSED_EPILOGUE=0. Returns (attacker, final patch on the host, the record of every
    add_patch_reg call: (patch before the step, patch.grad before, patch.grad after, scale), the number of accumulate calls of ops.patch_reg_grad)."""
    import sweep_harness
    from roboticattack_amd import ops
    from roboticattack_amd.attack import engine
    from roboticattack_amd.surrogate import SurrogateHeadVLA, SurrogateVLA

    tmp_path.mkdir(parents=True, exist_ok=True)
    sweep_harness.env(monkeypatch)
    if unfused:
        monkeypatch.setenv("VAA_FUSED_EPILOGUE", "0")
    record, calls = [], [0]
    orig_add, orig_grad = engine.AttackBase.add_patch_reg, ops.patch_reg_grad

    def add(self, patch, scale=1.0):
        pre = None if patch.grad is None else patch.grad.detach().clone()
        p0 = patch.detach().clone()
        orig_add(self, patch, scale)
        record.append((p0, pre, None if patch.grad is None else patch.grad.detach().clone(), scale))

    def spy(*a, **k):
        calls[0] += bool(k.get("accumulate", False))
        return orig_grad(*a, **k)

    monkeypatch.setattr(engine.AttackBase, "add_patch_reg", add)
    monkeypatch.setattr(ops, "patch_reg_grad", spy)
    args = types.SimpleNamespace(wandb_project="false")
    loaders = _Fresh([7000 + k for k in range(n_it)], BS), _Fresh([7100], BS)
    _seed()
    if which == "ddp":
        from roboticattack_amd.attack.uada_ddp import OpenVLAAttacker

        kw = {} if reg is None else dict(tv_weight=reg[0], nps_weight=reg[1])
        att = OpenVLAAttacker(vla_path="x", dataset_name="synthetic", save_dir=str(tmp_path), patch_size=PATCH, lr=0.02, bs=BS, warmup=1, num_iter=n_it,
                              maskidx=[0], innerLoop=inner, geometry=True, use_wandb=False, MSE_weights=5, device=torch.device(DEV), resize_patch=resize_patch,
                              colorjitter=colorjitter, model_factory=lambda path, dev: SurrogateHeadVLA(seed=2).to(dev), dataset_factory=lambda *a: loaders, **kw)
        att.val_batches = 1
        patch = att.attack(0, 1)
    else:
        mod = __import__("roboticattack_amd.attack." + which, fromlist=["OpenVLAAttacker"])
        vla = (SurrogateHeadVLA(seed=2) if which == "upa" else SurrogateVLA(seed=2)).to(DEV)  # UPA through K2', UADA / TMA through K2
        att = mod.OpenVLAAttacker(vla, None, str(tmp_path), optimizer="adamW", resize_patch=resize_patch)
        att.val_batches = 1
        if reg is not None:
            att.set_patch_reg(*reg)
        kw = dict(num_iter=n_it, patch_size=PATCH, accumulate_steps=1, maskidx=[0, 1, 2], warmup=1, geometry=True, innerLoop=inner, args=args,
                  colorjitter=colorjitter)
        kw.update({"alpha": 0.02} if which == "tma" else {"lr": 0.02})
        if which == "upa":
            kw["reverse_direction"] = True
        patch = att.patchattack_unconstrained(*loaders, **kw)
    torch.cuda.synchronize()
    ops.async_error_check()
    monkeypatch.setattr(engine.AttackBase, "add_patch_reg", orig_add)
    monkeypatch.setattr(ops, "patch_reg_grad", orig_grad)
    return att, patch.detach().cpu().clone(), record, calls[0]


@pytest.mark.parametrize("which", ["tma", "uada", "upa", "ddp"])
def test_loop_gradient_is_the_twins_plus_r(which, tmp_path, monkeypatch):
    """One backward with the weights on: patch.grad = the weights-off twin's patch.grad (same seeds, VAA_FUSED_EPILOGUE=0) + the write form's r,
    bitwise; ops.patch_reg_grad is called exactly once per backward; the logs carry the two values."""
    from roboticattack_amd import ops

    att, patch_on, rec_on, n_calls = _run_loop(which, tmp_path / "on", monkeypatch, 1, 2, reg=(ref.W_TV, ref.W_NPS))
    _, _, rec_off, n_off = _run_loop(which, tmp_path / "twin", monkeypatch, 1, 2, reg=(0.0, 0.0), unfused=True)
    assert n_calls == 2 and len(rec_on) == 2 and n_off == 0 and len(rec_off) == 2
    (p0, pre, post, scale), (q0, twin, twin_after, _) = rec_on[0], rec_off[0]
    assert torch.equal(p0, q0) and torch.equal(twin.view(torch.int32), twin_after.view(torch.int32))  # the same first step; off: nothing added
    assert torch.equal(pre.view(torch.int32), twin.view(torch.int32))
    r, _ = ops.patch_reg_grad(p0, torch.from_numpy(att._reg_palette_host).to(DEV), ref.W_TV * scale, ref.W_NPS * scale)
    assert float(r.abs().max()) > 0 and torch.equal(post.view(torch.int32), (twin + r).view(torch.int32))
    assert bool(torch.isfinite(patch_on).all()) and float(patch_on.min()) >= 0.0 and float(patch_on.max()) <= 1.0
    # the logs: the last inner step's values (of the patch that step saw) and the saved patch's values, against the fp64 restatement
    tv, nps = ref.values(rec_on[-1][0].cpu(), torch.from_numpy(att._reg_palette_host))
    assert abs(att.last_train_log["TRAIN_patch_tv"] - tv) <= 1e-6 and abs(att.last_train_log["TRAIN_patch_nps"] - nps) <= 1e-6
    tv, nps = ref.values(patch_on, torch.from_numpy(att._reg_palette_host))  # validation ran behind outer iteration 0's inner steps
    assert abs(att.last_val_log["VAL_patch_tv"] - tv) <= 1e-6 and abs(att.last_val_log["VAL_patch_nps"] - nps) <= 1e-6


@pytest.mark.parametrize("which", ["tma", "uada", "upa", "ddp"])
def test_loop_with_both_weights_zero_is_the_plain_run(which, tmp_path, monkeypatch):
    """Both weights 0: the fused paths stay selected, nothing is launched, and two outer iterations end on the bits of a run that never mentions
    the flags."""
    from roboticattack_amd.optim import PatchOptimizer

    att, zero, _, n_calls = _run_loop(which, tmp_path / "zero", monkeypatch, 2, 2, reg=(0.0, 0.0))
    assert n_calls == 0 and att._reg_part is None and "TRAIN_patch_tv" not in att.last_train_log and "VAL_patch_tv" not in att.last_val_log
    assert att.fused_update_sink(PatchOptimizer(torch.zeros(3, 8, 8, device=DEV), 1e-3, "adamW")) == {}
    if which in ("upa", "ddp"):  # the models that expose their patch-embed weights and hidden rows
        assert att.fused_ddp_available()
    _, plain, _, _ = _run_loop(which, tmp_path / "plain", monkeypatch, 2, 2)
    assert torch.equal(zero.view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("which,kw", [("uada", dict(colorjitter=True)), ("upa", dict(resize_patch=True))])
def test_loop_composes_with_colorjitter_and_resize_patch(which, kw, tmp_path, monkeypatch):
    """The regulariser acts on the base patch's gradient behind the jitter / resize adjoint: the runs complete (assert_finite_state passes inside
    the loop) and every step added the term."""
    _, patch, rec, n_calls = _run_loop(which, tmp_path, monkeypatch, 1, 2, reg=(ref.W_TV, ref.W_NPS), **kw)
    assert n_calls == 2 and all(not torch.equal(pre, post) for _, pre, post, _ in rec)
    assert bool(torch.isfinite(patch).all()) and float(patch.min()) >= 0.0 and float(patch.max()) <= 1.0
