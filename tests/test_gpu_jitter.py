"""GPU tests of the colour jitter (K0c): the two kernels through the C-ABI / ops against the fp64 restatement of include/vaa.h's definition
(tests/jitter_ref.py), their composition with the per-image-patch forms of K1 / K2 / K2', and the attack loops with the flag on.

Tolerances are measured, not guessed (jitter_ref.tolerances): tol_f = max(8 * e_ref_fwd, 3e-6) and tol_g = max(8 * e_ref_grad_rel, 1e-5), where
e_ref is the error of the fp32 restatement against the fp64 one on the same inputs; the kernel is never compared with itself."""
import types

import numpy as np
import pytest
import torch

import jitter_ref
from roboticattack_amd import synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]


def _pdesc(B, ph, pw):
    from roboticattack_amd import ops

    pdesc_np, total = ops.make_pdesc([(ph, pw)] * B)
    return pdesc_np, torch.from_numpy(pdesc_np).to(DEV), total


def _unpack(packed, pdesc_np, ph, pw):
    """packed f32 [total] -> [B,3,ph,pw] (a copy), read at the descriptor's offsets."""
    return torch.stack([packed[o : o + 3 * ph * pw].view(3, ph, pw) for o in pdesc_np[:, 2].tolist()])


def _pack(x, pdesc_np, total):
    """[B,3,ph,pw] -> packed f32 [total] in the descriptor's layout (zeros between the patches)."""
    packed = torch.zeros(total, dtype=torch.float32, device=x.device)
    for b, o in enumerate(pdesc_np[:, 2].tolist()):
        packed[o : o + x[b].numel()] = x[b].reshape(-1)
    return packed


def _kernel_fwd(patch, factors):
    from roboticattack_amd import ops

    ph, pw = int(patch.shape[1]), int(patch.shape[2])
    pdesc_np, pdesc, total = _pdesc(int(factors.shape[0]), ph, pw)
    return _unpack(ops.patch_jitter_fwd(patch, factors, pdesc, total), pdesc_np, ph, pw)


def _kernel_bwd(gout, patch, factors):
    from roboticattack_amd import ops

    pdesc_np, pdesc, total = _pdesc(int(factors.shape[0]), int(patch.shape[1]), int(patch.shape[2]))
    return ops.patch_jitter_bwd(_pack(gout, pdesc_np, total), patch, factors, pdesc)


def _dev(c):
    return c["patch"].to(DEV), c["factors"].to(DEV), c["gout"].to(DEV)


@pytest.mark.parametrize("name", list(jitter_ref.CASES))
def test_forward_vs_fp64(name):
    c = jitter_ref.case(name)
    tol_f, _ = jitter_ref.tolerances(name)
    patch, factors, _ = _dev(c)
    err = float((_kernel_fwd(patch, factors).cpu().double() - c["fwd64"]).abs().max())
    print(f"{name}: forward max|kernel - fp64| = {err:.3e} (e_ref {c['e_fwd']:.3e}, tol_f {tol_f:.3e})")
    assert err <= tol_f


@pytest.mark.parametrize("name", list(jitter_ref.CASES))
def test_identity_factors_return_the_base_patch_bit_for_bit(name):
    c = jitter_ref.case(name)
    patch = c["patch"].to(DEV)
    B = int(c["factors"].shape[0])
    out = _kernel_fwd(patch, torch.ones((B, 3), dtype=torch.float32, device=DEV))
    for b in range(B):
        assert torch.equal(out[b].view(torch.int32), patch.view(torch.int32))


@pytest.mark.parametrize("name", list(jitter_ref.CASES))
def test_adjoint_vs_fp64_autograd(name):
    """Upstream gradient standard normal; compared over the texels none of whose fp64 pre-clamp values lies within 1e-5 of 0 or 1 (at most 1 % may
    be left out). Every case holds an image with kappa = 0.5: an adjoint without the whole-patch mean term of the contrast stage misses there by
    6e-4 (50x50), 1.5e-2 (7x5) and 1.1e-3 (100x100) of max|ref| — 62 to 1489 times tol_g (confirmed on the restatement with the mean detached:
    tests/test_jitter_host.py::test_restatement_fp32_against_fp64_baseline)."""
    c = jitter_ref.case(name)
    _, tol_g = jitter_ref.tolerances(name)
    patch, factors, gout = _dev(c)
    keep = c["keep"]
    assert 1.0 - float(keep.float().mean()) <= 0.01
    assert any(float(k) == 0.5 for k in c["factors"][:, 1])
    g = _kernel_bwd(gout, patch, factors).cpu().double()
    ref = c["grad64"]
    err, gmax = float((g - ref)[:, keep].abs().max()), float(ref[:, keep].abs().max())
    print(f"{name}: adjoint max|kernel - fp64| = {err / gmax:.3e} of max|ref| (e_ref {c['e_grad_rel']:.3e}, tol_g {tol_g:.3e})")
    assert err <= tol_g * gmax


def test_saturated_texels_have_exact_gates():
    """About 20 % exact 0.0 and 20 % exact 1.0 texels, kappa = sigma = 1, beta in {0.8, 1.25}: the gradient is beta*G where beta*p <= 1 — at
    p = 0 too, the gate's bounds are inclusive — and exactly 0 where beta*p > 1. Nothing is left out of the comparison."""
    c = jitter_ref.case("saturated")
    _, tol_g = jitter_ref.tolerances("saturated")
    patch, factors, gout = _dev(c)
    ref = c["grad64"]
    gmax = float(ref.abs().max())
    g = _kernel_bwd(gout, patch, factors).cpu().double()
    err = float((g - ref).abs().max())
    print(f"saturated: adjoint max|kernel - fp64| = {err / gmax:.3e} of max|ref| (tol_g {tol_g:.3e})")
    assert err <= tol_g * gmax
    p = c["patch"]
    for b in range(2):  # per image (B = 1: the kernel writes the gradient itself): the closed form, zeros exact
        beta = float(c["factors"][b, 0])
        gb = _kernel_bwd(gout[b : b + 1], patch, factors[b : b + 1]).cpu()
        passes = (np.float32(beta) * p) <= 1
        assert bool((gb[~passes] == 0).all())
        want = beta * c["gout"][b].double()
        assert float((gb.double() - want)[passes].abs().max()) <= tol_g * float(want.abs().max())
        assert bool(passes[p == 0].all()) and bool((gb[p == 0] != 0).any())


def test_forward_and_adjoint_are_repeatable():
    g = torch.Generator().manual_seed(5)
    B = 8
    patch = (torch.rand((3, 50, 50), generator=g) * 0.9 + 0.05).to(DEV)
    factors = (torch.rand((B, 3), generator=g) * 0.8 + 0.6).to(DEV)
    gout = torch.randn((B, 3, 50, 50), generator=g).to(DEV)
    f0, g0 = _kernel_fwd(patch, factors), _kernel_bwd(gout, patch, factors)
    f1, g1 = _kernel_fwd(patch, factors), _kernel_bwd(gout, patch, factors)
    assert torch.equal(f0.view(torch.int32), f1.view(torch.int32)) and torch.equal(g0.view(torch.int32), g1.view(torch.int32))
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0


def test_descriptor_of_another_size_is_refused():
    """A pdesc entry whose size is not (ph, pw): that image is left unwritten and the library's failure word reports it."""
    from roboticattack_amd import _lib, ops

    patch = jitter_ref.case("7x5")["patch"].to(DEV)
    pdesc_np, _, total = _pdesc(2, 7, 5)
    pdesc_np = pdesc_np.copy()
    pdesc_np[1, 0] = 6
    packed = ops.patch_jitter_fwd(patch, torch.ones((2, 3), dtype=torch.float32, device=DEV), torch.from_numpy(pdesc_np).to(DEV), total)
    torch.cuda.synchronize()
    with pytest.raises(_lib.VaaError, match="pdesc entry"):
        ops.async_error_check()
    ops.async_error_check()  # the poll cleared the word
    out = _unpack(packed, pdesc_np, 7, 5)
    assert torch.equal(out[0], patch) and bool((out[1] == 0).all())


# ------------------------------------------------------------------------------------------------------
# composition with K1 / K2 / K2'
# ------------------------------------------------------------------------------------------------------
def _transform_call(t, patch, frames, colorjitter, monkeypatch, record):
    """apply_random_patch_batch(colorjitter=..., geometry=True) with K1's outputs and the per-image K2 / K2' outputs recorded."""
    from roboticattack_amd import ops

    k1, k2, k2e = ops._k1, ops.patch_grad_gather_multi, ops.patch_embed_grad_gather_multi_tiles

    def rec(key, f):
        def g(*a, **k):
            r = f(*a, **k)
            record[key] = r
            return r

        return g

    monkeypatch.setattr(ops, "_k1", rec("k1", k1))
    monkeypatch.setattr(ops, "patch_grad_gather_multi", rec("k2", k2))
    monkeypatch.setattr(ops, "patch_embed_grad_gather_multi_tiles", rec("k2", k2e))
    _seed()
    return t.apply_random_patch_batch(frames, patch, MEAN, STD, True, colorjitter=colorjitter)


def _seed():
    import random

    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


@pytest.mark.parametrize("route", ["planar", "embed"])
def test_composition_with_the_per_image_patch_kernels(route, monkeypatch):
    """Image b of the jittered call = the single-patch K1 (planar / tile-major) on frame b with the kernel's own y3_b as the patch, bit for bit;
    patch.grad = the jitter adjoint of the per-image K2 / K2' output, bit for bit; with factors (1, 1, 1) it is the shared-patch K2 / K2' gradient
    within 2e-6 * max|g| (DESIGN.md section 2's K2 bound for B <= 8: the per-image partials are added in another fixed order)."""
    from roboticattack_amd import ops
    from roboticattack_amd.surrogate import SurrogateHeadVLA
    from roboticattack_amd.transform import RandomPatchTransform

    B = 3
    frames = torch.from_numpy(synthetic.synth_images(11, B, "smooth")).to(DEV)
    patch = jitter_ref.case("50x50")["patch"].to(DEV).requires_grad_(True)
    t = RandomPatchTransform(DEV)
    if route == "embed":
        t.embed_with = SurrogateHeadVLA(seed=1).to(DEV)
    gen = torch.Generator().manual_seed(3)
    record = {}
    out = _transform_call(t, patch, frames, True, monkeypatch, record)
    k1_out = record["k1"]  # (the single-patch calls below go through the recorded K1 body too)
    xy_n, th_n = t.last_params
    xy, theta = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    factors = torch.from_numpy(t.last_jitter).to(DEV)
    assert float((factors - 1).abs().max()) > 0.01
    y3 = _kernel_fwd(patch.detach(), factors)
    for b in range(B):
        sl = slice(b, b + 1)
        if route == "planar":
            single, _ = ops.patch_apply_fwd(frames[sl], y3[b].contiguous(), xy[sl].contiguous(), theta[sl].contiguous(), True)
            assert torch.equal(out[sl].view(torch.int16), single.view(torch.int16))
        else:
            assert isinstance(out, ops.PatchEmbeds)
            s0, s1, _, _ = ops.patch_apply_fwd_tiles(frames[sl], y3[b].contiguous(), xy[sl].contiguous(), theta[sl].contiguous(), True)
            assert torch.equal(k1_out[0][sl].view(torch.int16), s0.view(torch.int16)) and torch.equal(k1_out[1][sl].view(torch.int16), s1.view(torch.int16))

    def backward(o):
        if route == "planar":
            gout = (torch.randn(o.shape, generator=gen) * 1e-3).to(torch.bfloat16).to(DEV)
            o.backward(gout)
            return (gout,)
        gs = tuple((torch.randn(e.shape, generator=gen) * 0.1).to(torch.bfloat16).to(DEV) for e in o)
        torch.autograd.backward(list(o), list(gs))
        return gs

    backward(out)
    pdesc = _pdesc(B, 50, 50)[1]
    assert torch.equal(patch.grad, ops.patch_jitter_bwd(record["k2"], patch.detach(), factors, pdesc))
    assert float(patch.grad.abs().max()) > 0

    # factors forced to (1, 1, 1): the shared-patch gradient
    patch.grad = None
    record.clear()
    out1 = _transform_call(t, patch, frames, (0.0, 0.0, 0.0), monkeypatch, record)
    assert np.array_equal(t.last_jitter, np.ones((B, 3), np.float32))
    gs = backward(out1)
    if route == "planar":
        _, keep = ops.patch_apply_fwd(frames, patch.detach(), xy, theta, True)
        shared = ops.patch_grad_gather(gs[0], patch.detach(), xy, theta, keep, True)
    else:
        _, _, wp0, _, _, wp1 = t.embed_with.patch_embed_params()
        _, _, keep_t, flags = ops.patch_apply_fwd_tiles(frames, patch.detach(), xy, theta, True)
        shared = ops.patch_embed_grad_gather_tiles(gs[0], gs[1], wp0, wp1, patch.detach(), xy, theta, keep_t, flags, True)
    err, gmax = float((patch.grad - shared).abs().max()), float(shared.abs().max())
    print(f"{route}: identity-jitter gradient vs shared-patch gradient: {err / gmax:.3e} of max|g|")
    assert gmax > 0 and err <= 2e-6 * gmax


# ------------------------------------------------------------------------------------------------------
# the attack loops
# ------------------------------------------------------------------------------------------------------
class _Fresh:
    def __init__(self, seeds, b):
        self.seeds, self.b = seeds, b

    def __len__(self):
        return len(self.seeds)

    def __iter__(self):
        for s in self.seeds:
            yield synthetic.synth_batch(s, self.b, "smooth")


N_IT, INNER, BS = 2, 2, 3


def _run_loop(which, tmp_path, monkeypatch, **jit):
    """2 outer x 2 inner steps, bs 3, seed 42, one validation batch (at outer iteration 0). Returns (the final patch on the host, kernel names of
    the training steps, kernel names of the validation pass)."""
    from roboticattack_amd import ops
    from roboticattack_amd.surrogate import SurrogateHeadVLA, SurrogateVLA

    train, val_names = [], []
    tmp_path.mkdir(parents=True, exist_ok=True)

    def traced(validate):  # the dispatch record is split around the validation pass
        def f(*a, **k):
            train.extend(n for n, _ in ops.prof_collect())
            ops.prof_start(4096)
            r = validate(*a, **k)
            val_names.extend(n for n, _ in ops.prof_collect())
            ops.prof_start(4096)
            return r

        return f

    args = types.SimpleNamespace(wandb_project="false")
    loaders = _Fresh([7000, 7001], BS), _Fresh([7100], BS)
    _seed()
    if which == "ddp":
        import sweep_harness
        from roboticattack_amd.attack.uada_ddp import OpenVLAAttacker

        sweep_harness.env(monkeypatch)
        att = OpenVLAAttacker(vla_path="x", dataset_name="synthetic", save_dir=str(tmp_path), patch_size=[3, 50, 50], lr=0.02, bs=BS, warmup=1,
                              num_iter=N_IT, maskidx=[0], innerLoop=INNER, geometry=True, use_wandb=False, MSE_weights=5, device=torch.device(DEV),
                              model_factory=lambda path, dev: SurrogateHeadVLA(seed=2).to(dev), dataset_factory=lambda *a: loaders, **jit)
        att.val_batches = 1
        att.validate = traced(att.validate)
        ops.prof_start(4096)
        patch = att.attack(0, 1)
    else:
        mod = __import__("roboticattack_amd.attack." + which, fromlist=["OpenVLAAttacker"])
        vla = (SurrogateHeadVLA(seed=2) if which == "upa" else SurrogateVLA(seed=2)).to(DEV)  # UPA through K2', UADA / TMA through K2
        att = mod.OpenVLAAttacker(vla, None, str(tmp_path), optimizer="adamW")
        att.val_batches = 1
        att.validate = traced(att.validate)
        kw = dict(num_iter=N_IT, patch_size=[3, 50, 50], accumulate_steps=1, maskidx=[0, 1, 2], warmup=1, geometry=True, innerLoop=INNER, args=args, **jit)
        kw.update({"alpha": 0.02} if which == "tma" else {"lr": 0.02})
        if which == "upa":
            kw["reverse_direction"] = True
        ops.prof_start(4096)
        patch = att.patchattack_unconstrained(*loaders, **kw)
    train.extend(n for n, _ in ops.prof_collect())
    torch.cuda.synchronize()
    ops.async_error_check()
    return patch.detach().cpu().clone(), train, val_names


@pytest.mark.parametrize("which", ["uada", "upa", "tma", "ddp"])
def test_attack_loops_with_colorjitter(which, tmp_path, monkeypatch):
    """UADA, UPA and TMA single-process and the data-parallel attacker at world size 1: colorjitter=True runs, the patch is finite and in [0,1],
    bitwise repeatable, and differs from the colorjitter=False run; the jitter forward and adjoint ran on every training step and not in the
    validation pass; colorjitter=False is bitwise the run without the argument (and launches neither kernel)."""
    on, train, val = _run_loop(which, tmp_path / "on", monkeypatch, colorjitter=True)
    assert bool(torch.isfinite(on).all()) and float(on.min()) >= 0.0 and float(on.max()) <= 1.0
    fwd, bwd = (sum(k in n for n in train) for k in ("patch_jitter_fwd_kernel", "patch_jitter_bwd_kernel"))
    assert fwd == N_IT * INNER and bwd == N_IT * INNER, sorted(set(train))
    assert val and not any("patch_jitter" in n for n in val), sorted(set(val))
    again, _, _ = _run_loop(which, tmp_path / "again", monkeypatch, colorjitter=True)
    assert torch.equal(on.view(torch.int32), again.view(torch.int32))
    off, train_off, _ = _run_loop(which, tmp_path / "off", monkeypatch, colorjitter=False)
    assert not torch.equal(on, off) and not any("patch_jitter" in n for n in train_off)
    plain, _, _ = _run_loop(which, tmp_path / "plain", monkeypatch)
    assert torch.equal(off.view(torch.int32), plain.view(torch.int32))
