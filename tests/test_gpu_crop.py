"""K9 on the GPU (vaa_crop_resize_fwd / _bwd, ops.CropResize, RandomPatchTransform(train_crop=...)) against tests/crop_ref.py: the forward byte
for byte against the fp32 restatement, the adjoint within a derived per-element bound of the fp64 transpose, the composition with K1 / K2, the
agreement with the evaluation's image path (K5 -> K7), and one outer iteration of UADA and TMA with the crop on."""
import types

import numpy as np
import pytest
import torch

import crop_ref as CR
import jitter_ref
import patch_grad_ref as R
from roboticattack_amd import synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, MEAN6, STD0, STD1, STD6

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def runs(ops):
    """Both batches of boxes through both kernels, once: {name: (boxes, forward bits, adjoint bits)}."""
    xb, gb = CR.inputs()
    x, g = _dev(xb), _dev(gb)
    out = {}
    for name, boxes in (("a", CR.boxes_a()), ("b", CR.boxes_b())):
        out[name] = (boxes, _bits(ops.crop_resize_fwd(x, boxes)), _bits(ops.crop_resize_bwd(g, boxes)))
    torch.cuda.synchronize()
    ops.async_error_check()
    return out


@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_is_the_fp32_restatement_byte_for_byte(runs, name):
    boxes, fwd, _ = runs[name]
    want = CR.fwd32(CR.inputs()[0], boxes)[0]
    assert np.array_equal(fwd, want), f"{int((fwd != want).sum())} of {want.size} elements differ"


def test_identity_box_is_a_copy_both_ways(runs):
    xb, gb = CR.inputs()
    boxes, fwd, bwd = runs["b"]
    assert tuple(boxes[0]) == (0, 0, 1, 1)
    assert np.array_equal(fwd[0], xb[0]) and np.array_equal(bwd[0], gb[0])


@pytest.mark.parametrize("name", ["a", "b"])
def test_adjoint_within_its_bound_of_the_fp64_transpose(runs, name):
    """Every element: |kernel - Wy^T g Wx| <= half a bf16 ulp + 16 u sum|w g| (crop_ref's module docstring derives the 16); elements no output
    touches have bound 0 and must be exactly +0."""
    boxes, _, bwd = runs[name]
    val, bound, _ = CR.bwd64(CR.bits_f32(CR.inputs()[1]).astype(np.float64), boxes)
    got = CR.bits_f32(bwd).astype(np.float64)
    worst, e = CR.worst_ratio(got, val, bound)
    print(f"boxes {name}: worst adjoint error / bound = {worst:.3g}")
    assert worst <= 1.0, f"element {np.unravel_index(e, val.shape)}: got {got.ravel()[e]!r}, reference {val.ravel()[e]!r}, bound {bound.ravel()[e]!r}"
    un = np.broadcast_to(CR.untouched(boxes)[:, None], bwd.shape)
    assert (bwd[un] == 0).all()  # +0 bits, not -0
    if name == "a":
        assert un.any()


def test_an_images_bits_do_not_depend_on_the_batch(ops, runs):
    xb, gb = CR.inputs()
    for name in ("a", "b"):
        boxes, fwd, bwd = runs[name]
        for k in (0, 2):
            one = boxes[k : k + 1]
            assert np.array_equal(_bits(ops.crop_resize_fwd(_dev(xb[k : k + 1]), one))[0], fwd[k])
            assert np.array_equal(_bits(ops.crop_resize_bwd(_dev(gb[k : k + 1]), one))[0], bwd[k])


def test_autograd_function_is_forward_and_adjoint(ops, runs):
    xb, gb = CR.inputs()
    boxes, fwd, bwd = runs["a"]
    x = _dev(xb).requires_grad_(True)
    y = ops.CropResize.apply(x, boxes)
    y.backward(_dev(gb))
    assert np.array_equal(_bits(y.detach()), fwd) and np.array_equal(_bits(x.grad), bwd)


# ---- composition with K1 / K2 ----
def _seed():
    import random

    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


@pytest.mark.parametrize("colorjitter", [False, True])
def test_composition_patch_gradient_vs_fp64(ops, colorjitter):
    """apply_random_patch_batch(geometry=True, train_crop="center") on 2 frames and a 3x22x22 patch: patch.grad against crop_ref.compose_ref —
    patch_grad_ref's K2 reference fed with the fp64 transpose of K9's taps, its per-texel bound widened by K9's per-element bound (derived
    there). With colorjitter the per-image K2 reference is carried through the fp64 jitter adjoint: bound = sum_b |J_b|^T bound_b (J_b the
    jitter's Jacobian; the patch lies in [0.25, 0.75], so no clamp engages and the jitter is linear) + 1e-5 max|value|, the jitter
    adjoint's own tolerance floor (jitter_ref.tolerances)."""
    from roboticattack_amd.transform import RandomPatchTransform

    B, ph, pw = 2, 22, 22
    frames = torch.from_numpy(synthetic.synth_images(11, B, "smooth")).to(DEV)
    gen = torch.Generator().manual_seed(5)
    patch = (0.25 + 0.5 * torch.rand(3, ph, pw, generator=gen)).to(DEV).requires_grad_(True)
    t = RandomPatchTransform(DEV, train_crop="center")
    _seed()
    out = t.apply_random_patch_batch(frames, patch, MEAN, STD, True, colorjitter=colorjitter)
    gout = (torch.randn(out.shape, generator=gen) * 1e-2).to(torch.bfloat16).to(DEV)
    out.backward(gout)
    torch.cuda.synchronize()
    xy_n, th_n = t.last_params
    boxes = t.last_crop
    assert np.array_equal(boxes, np.tile(CR.center_box(0.9), (B, 1)))
    xy, theta = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    if not colorjitter:
        plain, keep = ops.patch_apply_fwd(frames, patch.detach(), xy, theta, True)
        assert torch.equal(out.view(torch.int16), ops.crop_resize_fwd(plain, boxes).view(torch.int16))
        keep01 = np.unpackbits(keep.cpu().numpy(), axis=-1, bitorder="little")
        ref = CR.compose_ref(_bits(gout), boxes, keep01, xy_n, th_n.reshape(B, 2, 3), True, ph, pw)
        worst = R.compare(ref, patch.grad, "K9 -> K2")
    else:
        factors = torch.from_numpy(t.last_jitter).to(DEV)
        pdesc_np, total = ops.make_pdesc([(ph, pw)] * B)
        pdesc = torch.from_numpy(pdesc_np).to(DEV)
        packed = ops.patch_jitter_fwd(patch.detach(), factors, pdesc, total)
        plain, keep = ops.patch_apply_fwd_multi(frames, packed, pdesc, (ph, pw), xy, theta, True)
        assert torch.equal(out.view(torch.int16), ops.crop_resize_fwd(plain, boxes).view(torch.int16))
        keep01 = np.unpackbits(keep.cpu().numpy(), axis=-1, bitorder="little")
        per = CR.compose_ref(_bits(gout), boxes, keep01, xy_n, th_n.reshape(B, 2, 3), True, ph, pw, pdesc=pdesc_np)
        n = 3 * ph * pw
        p64, f64 = patch.detach().cpu().double(), factors.cpu().double()
        val, bound = np.zeros(n), np.zeros(n)
        for b in range(B):
            off = int(pdesc_np[b][2])
            J = torch.autograd.functional.jacobian(lambda p: jitter_ref.jitter_fwd(p, f64[b : b + 1])[0], p64, vectorize=True).reshape(n, n).numpy()
            val += J.T @ per.value[off : off + n]
            bound += np.abs(J).T @ per.bound[off : off + n]
        bound += 1e-5 * np.abs(val).max()
        worst, e = CR.worst_ratio(patch.grad.detach().double().cpu().numpy().ravel(), val, bound)
        assert worst <= 1.0, f"texel {e}: error / bound = {worst:.3g}"
    print(f"colorjitter={colorjitter}: worst patch-gradient error / bound = {worst:.3g}")
    assert float(patch.grad.abs().max()) > 0


# ---- agreement with the evaluation ----
def test_training_pixels_agree_with_the_evaluations(ops):
    """Frame bytes and patch texels that are exact multiples of 1/255, no geometry, a fixed position: CropResize(K1) with the centre box lies
    within crop_ref.eval_bound (derived there) of eval_pixel_values(simulation_patch_batch(...), center_crop=True) on EVERY element, while K1's
    uncropped output exceeds that bound on at least 6 * 22 elements (one border row of the 22x22 patch in every plane: the crop magnifies by
    1.054 about the centre, which moves a patch at (20, 30) by about 5 pixels)."""
    from roboticattack_amd.transform import RandomPatchTransform

    B, ph, pw, pos = 2, 22, 22, (20, 30)
    frames_np = synthetic.synth_images(4, B, "smooth")
    frames = torch.from_numpy(frames_np).to(DEV)
    # texels k/255 that K5's uint8 quantisation (fp32 * 255, truncated) returns as k: the two paths then paste the same value
    k = np.arange(256)
    exact = k[((k.astype(np.float32) / np.float32(255.0)) * np.float32(255.0)).astype(np.int32) == k]
    rs = np.random.RandomState(3)
    patch = torch.from_numpy((rs.choice(exact, (3, ph, pw)).astype(np.float32) / np.float32(255.0))).to(DEV)
    t = RandomPatchTransform(DEV)
    pasted = t.simulation_patch_batch(frames, patch, [False] * B, [0.0] * B, [0.0] * B, [0.0] * B, [pos] * B)
    want = t.eval_pixel_values(pasted, MEAN, STD, center_crop=True).float().cpu().numpy().astype(np.float64)
    xy = torch.tensor([pos] * B, dtype=torch.int32, device=DEV)
    plain, _ = ops.patch_apply_fwd(frames, patch, xy, None, False, ops.MASK_NE_M100)
    got = ops.CropResize.apply(plain, np.tile(CR.center_box(0.9), (B, 1))).float().cpu().numpy().astype(np.float64)
    bound = CR.eval_bound(MEAN6, STD6)[None, :, None, None]
    err = np.abs(got - want)
    print("worst |training - evaluation| / bound per channel:", (err / bound).max(axis=(0, 2, 3)).round(3))
    assert (err <= bound).all(), f"{int((err > bound).sum())} elements outside the bound, worst {float((err / bound).max()):.3g} x"
    off = np.abs(plain.float().cpu().numpy().astype(np.float64) - want) > bound
    print("uncropped output outside the bound on", int(off.sum()), "elements")
    assert int(off.sum()) >= 6 * 22


# ---- the loops ----
class _Fresh:
    def __init__(self, seeds, b):
        self.seeds, self.b = seeds, b

    def __len__(self):
        return len(self.seeds)

    def __iter__(self):
        for s in self.seeds:
            yield synthetic.synth_batch(s, self.b, "smooth")


def _run_loop(ops, which, tmp_path, **crop):
    """One outer iteration (one inner step, one validation batch) of UADA / TMA on the surrogate, bs 2, seed 42."""
    from roboticattack_amd.surrogate import SurrogateVLA

    tmp_path.mkdir(parents=True, exist_ok=True)
    mod = __import__("roboticattack_amd.attack." + which, fromlist=["OpenVLAAttacker"])
    att = mod.OpenVLAAttacker(SurrogateVLA(seed=2).to(DEV), None, str(tmp_path), optimizer="adamW")
    att.val_batches = 1
    boxes = []
    orig = att.randomPatchTransform._crop_boxes
    att.randomPatchTransform._crop_boxes = lambda *a: boxes.append(orig(*a).copy()) or boxes[-1]
    kw = dict(num_iter=1, patch_size=[3, 22, 22], accumulate_steps=1, maskidx=[0, 1, 2], warmup=1, geometry=True, innerLoop=1,
              args=types.SimpleNamespace(wandb_project="false"), **crop)
    kw.update({"alpha": 0.02} if which == "tma" else {"lr": 0.02})
    _seed()
    ops.prof_start(1024)
    patch = att.patchattack_unconstrained(_Fresh([7000], 2), _Fresh([7100], 2), **kw)
    names = [n for n, _ in ops.prof_collect()]
    torch.cuda.synchronize()
    ops.async_error_check()
    return patch.detach().cpu().clone(), names, boxes, att


@pytest.mark.parametrize("which", ["uada", "tma"])
def test_one_outer_iteration_with_random_crop(ops, which, tmp_path):
    on, names, boxes, att = _run_loop(ops, which, tmp_path / "on", train_crop="random")
    assert bool(torch.isfinite(on).all()) and float(on.min()) >= 0.0 and float(on.max()) <= 1.0
    last = att.randomPatchTransform.last_crop
    assert last.shape == (2, 4) and last.dtype == np.float32
    centre = np.tile(CR.center_box(0.9), (2, 1))
    assert len(boxes) == 2 and not np.array_equal(boxes[0], centre) and np.array_equal(boxes[1], centre)  # the step draws, the validation pass does not
    assert sum("crop_resize_fwd_kernel" in n for n in names) == 2 and sum("crop_resize_bwd_kernel" in n for n in names) == 1, sorted(set(names))
    off, names_off, boxes_off, _ = _run_loop(ops, which, tmp_path / "off", train_crop=None)
    plain, _, _, _ = _run_loop(ops, which, tmp_path / "plain")
    assert torch.equal(off.view(torch.int32), plain.view(torch.int32)) and not boxes_off and not any("crop_resize" in n for n in names_off)
