"""K11 on the GPU (vaa_defocus_blur_fwd / _bwd, ops.DefocusBlur, RandomPatchTransform.set_defocus_blur) against tests/blur_ref.py: the forward
byte for byte against the fp32 restatement, the adjoint within a derived per-element bound of the fp64 transpose, batch independence, repeat
determinism, the composition K1 -> K11 -> K9 -> K10 with its adjoints, and one outer iteration of UADA and TMA with the blur on. B = 4."""
import types

import numpy as np
import pytest
import torch

import blur_ref as BR
from roboticattack_amd import synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _dev(bits):
    return torch.from_numpy(np.array(bits).view(np.int16)).to(DEV).view(torch.bfloat16)  # (a copy: the shared inputs are read-only)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def run(ops):
    """The shared inputs through both kernels, once: (taps, forward bits, adjoint bits)."""
    xb, gb = BR.inputs()
    taps = ops.blur_taps(BR.SIGMAS)
    assert np.array_equal(taps, BR.reference()["taps"])
    fwd, bwd = _bits(ops.defocus_blur_fwd(_dev(xb), taps)), _bits(ops.defocus_blur_bwd(_dev(gb), taps))
    torch.cuda.synchronize()
    ops.async_error_check()
    return taps, fwd, bwd


def test_forward_is_the_fp32_restatement_byte_for_byte(run):
    _, fwd, _ = run
    want = BR.reference()["fwd_bits"]
    diff = fwd != want
    for b in range(4):
        n = int(diff[b].sum())
        first = tuple(int(v) for v in np.argwhere(diff[b])[0]) if n else None
        print(f"image {b} (sigma {BR.SIGMAS[b]}): {n} of {want[b].size} elements differ, first at (plane, y, x) = {first}")
    assert not diff.any(), f"{int(diff.sum())} of {want.size} elements differ, first at (image, plane, y, x) = {tuple(int(v) for v in np.argwhere(diff)[0])}"


def test_sigma_zero_is_a_bit_copy_both_ways(run):
    xb, gb = BR.inputs()
    taps, fwd, bwd = run
    assert BR.SIGMAS[0] == 0.0 and tuple(taps[0]) == (1, 0, 0, 0, 0, 0, 0, 0)
    assert np.array_equal(fwd[0], xb[0]) and np.array_equal(bwd[0], gb[0])


def test_adjoint_within_its_bound_of_the_fp64_transpose(run):
    """Every element: |kernel - A^T g A| <= half a bf16 ulp + 2 ((n_r + 1) + (n_j + 1)) u sum |w| |w| |g| (blur_ref's module docstring derives it);
    the all-zero plane has bound 0 and must be +0 bits everywhere."""
    _, _, bwd = run
    ref = BR.reference()
    got = BR.bits_f32(bwd).astype(np.float64)
    for b in range(4):
        w, _ = BR.worst_ratio(got[b], ref["gx"][b], ref["gx_bound"][b])
        print(f"image {b} (sigma {BR.SIGMAS[b]}): worst adjoint error / bound = {w:.4g}")
    worst, e = BR.worst_ratio(got, ref["gx"], ref["gx_bound"])
    assert worst <= 1.0, (f"element {np.unravel_index(e, got.shape)}: got {got.ravel()[e]!r}, reference {ref['gx'].ravel()[e]!r}, "
                          f"bound {ref['gx_bound'].ravel()[e]!r}")
    assert (bwd[BR.ZERO_PLANE] == 0).all()  # +0 bits, not -0


def test_an_images_bits_do_not_depend_on_the_batch(ops, run):
    xb, gb = BR.inputs()
    taps, fwd, bwd = run
    for k in (1, 3):
        one = taps[k : k + 1]
        assert np.array_equal(_bits(ops.defocus_blur_fwd(_dev(xb[k : k + 1]), one))[0], fwd[k])
        assert np.array_equal(_bits(ops.defocus_blur_bwd(_dev(gb[k : k + 1]), one))[0], bwd[k])


def test_a_second_call_gives_the_same_bits(ops, run):
    xb, gb = BR.inputs()
    taps, fwd, bwd = run
    assert np.array_equal(_bits(ops.defocus_blur_fwd(_dev(xb), taps)), fwd)
    assert np.array_equal(_bits(ops.defocus_blur_bwd(_dev(gb), taps)), bwd)
    torch.cuda.synchronize()
    ops.async_error_check()


def test_autograd_function_is_forward_and_adjoint(ops, run):
    xb, gb = BR.inputs()
    taps, fwd, bwd = run
    x = _dev(xb).requires_grad_(True)
    y = ops.DefocusBlur.apply(x, taps)
    y.backward(_dev(gb))
    assert np.array_equal(_bits(y.detach()), fwd) and np.array_equal(_bits(x.grad), bwd)


def test_overlapping_buffers_are_refused(ops):
    """The entry point's overlap rule with real device addresses: out inside x's range returns VAA_E_INVALID before any launch."""
    from roboticattack_amd import _lib

    buf = torch.zeros(2 * 6 * 224 * 224 + 8, dtype=torch.bfloat16, device=DEV)
    taps = ops.blur_taps([1.0])
    tdev = torch.from_numpy(taps).to(DEV)
    L = _lib.lib()
    for off in (0, 8, 6 * 224 * 224 - 8):
        rc = L.vaa_defocus_blur_fwd(buf.data_ptr(), taps.ctypes.data, tdev.data_ptr(), 1, buf.data_ptr() + 2 * off, None)
        assert rc == -1 and b"must not overlap" in L.vaa_last_error(), off
    rc = L.vaa_defocus_blur_fwd(buf.data_ptr(), taps.ctypes.data, tdev.data_ptr(), 1, buf.data_ptr() + 2 * 6 * 224 * 224, None)
    assert rc == 0  # adjacent is not overlapping
    torch.cuda.synchronize()
    ops.async_error_check()


# ---- composition K1 -> K11 -> K9 -> K10 ----
def _seed():
    import random

    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


def test_composition_with_crop_and_scene_jitter(ops):
    """RandomPatchTransform with blur, train_crop="random" and scene jitter equals K1 -> defocus_blur_fwd -> crop_resize_fwd -> scene_jitter_fwd
    composed by hand from last_blur / last_crop / last_scene, bit for bit, and patch.grad equals K2 of the hand-composed adjoints."""
    from roboticattack_amd.transform import RandomPatchTransform

    B, ph, pw = 4, 22, 22
    frames = torch.from_numpy(synthetic.synth_images(11, B, "smooth")).to(DEV)
    gen = torch.Generator().manual_seed(5)
    patch = (0.25 + 0.5 * torch.rand(3, ph, pw, generator=gen)).to(DEV).requires_grad_(True)
    t = RandomPatchTransform(DEV, train_crop="random")
    t.set_scene_jitter(True)
    t.set_defocus_blur(1.5)
    _seed()
    out = t.apply_random_patch_batch(frames, patch, MEAN, STD, True)
    gout = (torch.randn(out.shape, generator=gen) * 1e-2).to(torch.bfloat16).to(DEV)
    out.backward(gout)
    torch.cuda.synchronize()
    xy_n, th_n = t.last_params
    sig, boxes, factors = t.last_blur, t.last_crop, t.last_scene
    assert sig.dtype == np.float32 and sig.shape == (B,) and (sig > 0).all() and (sig <= 1.5).all() and len(set(sig.tolist())) == B
    taps = ops.blur_taps(sig)
    xy, theta = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    plain, keep = ops.patch_apply_fwd(frames, patch.detach(), xy, theta, True)
    blurred = ops.defocus_blur_fwd(plain, taps)
    cropped = ops.crop_resize_fwd(blurred, boxes)
    lit = ops.scene_jitter_fwd(cropped, factors)
    assert torch.equal(out.view(torch.int16), lit.view(torch.int16))
    assert not torch.equal(blurred.view(torch.int16), plain.view(torch.int16))
    g = ops.scene_jitter_bwd(gout, cropped, factors)
    g = ops.crop_resize_bwd(g, boxes)
    g = ops.defocus_blur_bwd(g, taps)
    want = ops.patch_grad_gather(g, patch.detach(), xy, theta, keep, True)
    assert torch.equal(patch.grad.view(torch.int32), want.view(torch.int32)) and float(patch.grad.abs().max()) > 0
    torch.cuda.synchronize()
    ops.async_error_check()


# ---- the loops ----
class _Fresh:
    def __init__(self, seeds, b):
        self.seeds, self.b = seeds, b

    def __len__(self):
        return len(self.seeds)

    def __iter__(self):
        for s in self.seeds:
            yield synthetic.synth_batch(s, self.b, "smooth")


def _run_loop(ops, which, tmp_path, **blur):
    """One outer iteration (one inner step, one validation batch) of UADA / TMA on the surrogate, bs 2, seed 42. warmup=0: the cosine schedule
    starts at the full learning rate (with a warm-up the first step's rate is 0 and no run could move the patch)."""
    from roboticattack_amd.surrogate import SurrogateVLA

    tmp_path.mkdir(parents=True, exist_ok=True)
    mod = __import__("roboticattack_amd.attack." + which, fromlist=["OpenVLAAttacker"])
    att = mod.OpenVLAAttacker(SurrogateVLA(seed=2).to(DEV), None, str(tmp_path), optimizer="adamW")
    att.val_batches = 1
    kw = dict(num_iter=1, patch_size=[3, 22, 22], accumulate_steps=1, maskidx=[0, 1, 2], warmup=0, geometry=True, innerLoop=1,
              args=types.SimpleNamespace(wandb_project="false"), **blur)
    kw.update({"alpha": 0.02} if which == "tma" else {"lr": 0.02})
    _seed()
    ops.prof_start(1024)
    patch = att.patchattack_unconstrained(_Fresh([7000], 2), _Fresh([7100], 2), **kw)
    names = [n for n, _ in ops.prof_collect()]
    torch.cuda.synchronize()
    ops.async_error_check()
    return patch.detach().cpu().clone(), names, att


@pytest.mark.parametrize("which", ["uada", "tma"])
def test_one_outer_iteration_with_blur(ops, which, tmp_path):
    on, names, att = _run_loop(ops, which, tmp_path / "on", defocus_blur=0.8)
    assert bool(torch.isfinite(on).all()) and float(on.min()) >= 0.0 and float(on.max()) <= 1.0
    last = att.randomPatchTransform.last_blur
    assert last.shape == (2,) and last.dtype == np.float32 and (last >= 0).all() and (last <= np.float32(0.8)).all()
    # the training step blurs and carries the gradient back; the validation pass sees the sharp frame
    assert sum("defocus_blur_fwd_kernel" in n for n in names) == 1 and sum("defocus_blur_bwd_kernel" in n for n in names) == 1, sorted(set(names))
    off, names_off, att_off = _run_loop(ops, which, tmp_path / "off", defocus_blur=False)
    plain, _, _ = _run_loop(ops, which, tmp_path / "plain")
    assert torch.equal(off, plain) and not any("defocus_blur" in n for n in names_off) and att_off.randomPatchTransform.last_blur is None
    assert not torch.equal(on, plain)
