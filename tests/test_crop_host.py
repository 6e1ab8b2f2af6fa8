"""CPU-only checks of the crop-aware training path (K9): the references of tests/crop_ref.py against K7's restatement and against each other,
the bounds' self-test, the host layer (flags, RNG consumption, refusals) and the entry points' argument errors. No kernel is launched."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import crop_ref as CR
import eval_ref
from conftest import ROOT
from roboticattack_amd import _lib, ops, synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
from roboticattack_amd.transform import RandomPatchTransform, center_crop_box
from sweep_harness import attacker, fused

MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]
B, PH, PW = 4, 50, 40
f32 = np.float32


# ---- references ----
def test_centre_box_is_k7s_geometry():
    """The centre box at 0.9: the same source coordinate, t, b, lx = ly per output index as K7's restatement (eval_ref.crop_u8_f32 forms them
    inline: restated here line by line), the clamp never fires, and on frames of exact bytes / 255 the fp32 bilinear with crop_ref's taps is
    eval_ref's pre-quantisation value bit for bit."""
    box = CR.center_box(0.9)
    assert np.array_equal(box, center_crop_box(0.9)) and box[0] == box[1] and box[2] == box[3]
    s = np.minimum(np.maximum(np.sqrt(f32(0.9)), f32(0.0)), f32(1.0))
    y1 = (f32(1.0) - s) / f32(2.0)
    y2 = y1 + s
    scale = ((y2 - y1) * f32(223)) / f32(223)
    in_c = y1 * f32(223) + np.arange(224, dtype=f32) * scale  # eval_ref.crop_u8_f32
    t, b, l, c = CR.taps32(box[0], box[2])
    assert np.array_equal(c, in_c) and in_c.min() >= 0 and in_c.max() <= 223
    assert np.array_equal(t, np.floor(in_c)) and np.array_equal(b, np.ceil(in_c)) and np.array_equal(l, in_c - np.floor(in_c))
    frames = eval_ref.frames("noise", 2)
    want = eval_ref._resample(frames, in_c, f32)  # [B,224,224,3], clipped to [0, 1] (a convex combination of values in [0, 1] already is)
    f = frames.astype(f32) * (f32(1.0) / f32(255.0))
    tl, tr, bl, br = f[:, t][:, :, t], f[:, t][:, :, b], f[:, b][:, :, t], f[:, b][:, :, b]
    lx, ly = l[None, None, :, None], l[None, :, None, None]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    got = top + (bot - top) * ly
    assert got.dtype == f32 and np.array_equal(got, want)


def test_fp64_adjoint_is_the_transpose():
    rs = np.random.RandomState(1)
    for boxes in (CR.boxes_a(), CR.boxes_b()):
        x, g = rs.standard_normal((3, 6, 224, 224)), rs.standard_normal((3, 6, 224, 224))
        lhs = float((CR.fwd64(x, boxes) * g).sum())
        rhs = float((x * CR.bwd64(g, boxes)[0]).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_identity_box_returns_its_input():
    xb, gb = CR.inputs()
    ident = np.tile(np.array([0, 0, 1, 1], f32), (3, 1))
    assert np.array_equal(CR.fwd32(xb, ident)[0], xb)
    assert np.array_equal(CR.fwd64(CR.bits_f32(xb).astype(np.float64), ident), CR.bits_f32(xb).astype(np.float64))
    val, bound, _ = CR.bwd64(CR.bits_f32(gb).astype(np.float64), ident)
    assert np.array_equal(val, CR.bits_f32(gb).astype(np.float64))


def test_fp32_restatement_against_fp64():
    """The restatement's values before the bf16 rounding lie within 6 u sum|w x| of the fp64 forward (fl(tr - tl), the product and the add per
    blend, three blends deep along one path: 6 roundings of quantities bounded by sum|w x| <= 2 max|x| each)."""
    xb, _ = CR.inputs()
    for boxes in (CR.boxes_a(), CR.boxes_b()):
        x = CR.bits_f32(xb).astype(np.float64)
        err = np.abs(CR.fwd32(xb, boxes)[1].astype(np.float64) - CR.fwd64(x, boxes))
        assert float(err.max()) <= 6 * CR.U * 2 * 2.6


def test_untouched_elements_are_exactly_zero_in_the_reference():
    _, gb = CR.inputs()
    g = CR.bits_f32(gb).astype(np.float64)
    for boxes in (CR.boxes_a(), CR.boxes_b()):
        val, bound, A = CR.bwd64(g, boxes)
        un = CR.untouched(boxes)
        m = np.broadcast_to(un[:, None], val.shape)
        assert (val[m] == 0).all() and (bound[m] == 0).all() and (A[m] == 0).all()
    un = CR.untouched(CR.boxes_a())
    assert un[0].any() and un[1].any() and un[2].any() and not CR.untouched(CR.boxes_b())[0].any()
    assert un[1][223, 223] and un[2][0, 0] and un[0][0, 0] and un[0][223, 223]


@pytest.mark.parametrize("fault", ["tap", "swap"])
def test_perturbation_breaks_every_bound(fault):
    """One tap moved by one index (output row 100's bottom tap), or ly traded for 1 - ly: the forward's restatement changes bits, the adjoint
    leaves its per-element bound, the composed patch gradient leaves its per-texel bound, and the training-against-evaluation bound of
    test_gpu_crop.py (crop_ref.eval_bound) is exceeded."""
    xb, gb = CR.inputs()
    boxes = CR.boxes_a()
    good_bits, good = CR.fwd32(xb, boxes)
    bad_bits, bad = CR.fwd32(xb, boxes, fault)
    assert not np.array_equal(good_bits, bad_bits)
    g = CR.bits_f32(gb).astype(np.float64)
    val, bound, _ = CR.bwd64(g, boxes)
    assert CR.worst_ratio(CR.bwd64(g, boxes, fault)[0], val, bound)[0] > 1.0
    # composition: an un-warped 22x22 paste (keep = the patch's footprint) under the centre box
    import patch_grad_ref as R

    xy = np.array([[90, 92], [10, 180]], np.int32)
    keep = np.zeros((2, 3, 224, 224), np.uint8)
    for k, (x, y) in enumerate(xy):
        keep[k, :, y : y + 22, x : x + 22] = 1
    cb = np.tile(CR.center_box(0.9), (2, 1))
    ref = CR.compose_ref(gb[:2], cb, keep.reshape(2, 3, -1), xy, None, False, 22, 22)
    bad_ref = CR.compose_ref(gb[:2], cb, keep.reshape(2, 3, -1), xy, None, False, 22, 22, fault=fault)
    with pytest.raises(AssertionError):
        R.compare(ref, bad_ref.value, fault)
    # agreement with the evaluation: the fault moves pixel values by more than EVAL_BOUND allows anywhere
    from roboticattack_amd.constants import MEAN6, STD6

    assert (np.abs(bad.astype(np.float64) - good.astype(np.float64))[0] > CR.eval_bound(MEAN6, STD6)[:, None, None]).any()


# ---- host layer ----
def _wrapper(fname):
    spec = importlib.util.spec_from_file_location("crop_" + fname[:-3], os.path.join(ROOT, "VLAAttacker", fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("fname", ["UADA_wrapper.py", "UADA_wrapper_ddp.py", "UPA_wrapper.py", "TMA_wrapper.py"])
def test_cli_flags(fname):
    from roboticattack_amd import cli

    w = _wrapper(fname)
    a = w.arg_parser([])
    assert a.train_crop == "none" and a.train_crop_scale == 0.9 and cli.train_crop_args(a) == {"train_crop": None, "train_crop_scale": 0.9}
    a = w.arg_parser(["--train_crop", "center"])
    assert cli.train_crop_args(a) == {"train_crop": "center", "train_crop_scale": 0.9}
    a = w.arg_parser(["--train_crop", "random", "--train_crop_scale", "0.81"])
    assert cli.train_crop_args(a) == {"train_crop": "random", "train_crop_scale": 0.81}
    with pytest.raises(SystemExit):
        w.arg_parser(["--train_crop", "corner"])


def _seed():
    random.seed(42)
    np.random.seed(42)


def _state():
    return random.getstate(), np.random.get_state()


def _same(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def _stub(monkeypatch, calls):
    def paste(name):
        def apply(patch, img, *rest):
            calls.append((name, rest))
            return torch.zeros((img.shape[0], 6, 224, 224), dtype=torch.bfloat16)

        return staticmethod(apply)

    for name in ("PatchApply", "PatchApplyJittered", "PatchApplyResized", "PatchApplyEmbed"):
        monkeypatch.setattr(getattr(ops, name), "apply", paste(name), raising=False)

    def crop(x, boxes):
        calls.append(("CropResize", np.array(boxes, copy=True)))
        return x

    monkeypatch.setattr(ops.CropResize, "apply", staticmethod(crop), raising=False)


def _frames():
    return torch.from_numpy(synthetic.synth_images(3, B, "smooth"))


@pytest.mark.parametrize("geometry", [True, False])
def test_crop_off_consumes_todays_rng_stream(monkeypatch, geometry):
    """train_crop=None (the default, and set explicitly): the draws of draw_params and nothing else; no CropResize."""
    for t in (RandomPatchTransform("cpu"), RandomPatchTransform("cpu", train_crop=None)):
        calls = []
        _stub(monkeypatch, calls)
        patch = torch.rand(3, PH, PW, requires_grad=True)
        _seed()
        t.apply_random_patch_batch(_frames(), patch, MEAN, STD, geometry)
        after = _state()
        _seed()
        t.draw_params(B, PH, PW, geometry)
        assert _same(after, _state()) and [c[0] for c in calls] == ["PatchApply"] and t.last_crop is None and t.train_crop is None


@pytest.mark.parametrize("colorjitter", [False, True])
def test_random_crop_draws_two_per_image_behind_every_other_draw(monkeypatch, colorjitter):
    calls = []
    _stub(monkeypatch, calls)
    t = RandomPatchTransform("cpu", train_crop="random", train_crop_scale=0.9)
    patch = torch.rand(3, PH, PW, requires_grad=True)
    _seed()
    t.apply_random_patch_batch(_frames(), patch, MEAN, STD, True, colorjitter=colorjitter)
    after = _state()
    _seed()
    t.draw_params(B, PH, PW, True)
    if colorjitter:
        [random.uniform(0.8, 1.2) for _ in range(3 * B)]
    s = float(CR.center_box(0.9)[2] - CR.center_box(0.9)[0])
    want = np.array([[random.uniform(0, 1 - s), random.uniform(0, 1 - s)] for _ in range(B)], f32)  # image-major: y1, then x1
    assert _same(after, _state())
    assert [c[0] for c in calls] == ["PatchApplyJittered" if colorjitter else "PatchApply", "CropResize"]
    boxes = calls[-1][1]
    assert boxes.dtype == f32 and boxes.shape == (B, 4) and np.array_equal(boxes, t.last_crop) and np.array_equal(boxes[:, :2], want)
    side = boxes[:, 2:] - boxes[:, :2]
    assert (boxes >= 0).all() and (boxes <= 1).all() and (side >= f32(0.5)).all() and np.abs(side - s).max() < 1e-6


def test_centre_crop_and_validation_calls_make_no_draw(monkeypatch):
    """"center": no RNG call beyond the placement; a call that is not differentiable (the loops' validation passes) uses the centre box in both modes."""
    for mode, grad in (("center", True), ("random", False), ("center", False)):
        calls = []
        _stub(monkeypatch, calls)
        t = RandomPatchTransform("cpu", train_crop=mode)
        patch = torch.rand(3, PH, PW, requires_grad=grad)
        _seed()
        t.random_paste_patch(_frames(), patch, MEAN, STD)
        after = _state()
        _seed()
        t.draw_params(B, PH, PW, False)
        assert _same(after, _state())
        assert np.array_equal(calls[-1][1], np.tile(CR.center_box(0.9), (B, 1)))
    calls = []
    _stub(monkeypatch, calls)
    t = RandomPatchTransform("cpu", train_crop="random")
    with torch.no_grad():
        t.paste_patch_fix(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD)
    assert np.array_equal(calls[-1][1], np.tile(CR.center_box(0.9), (B, 1)))


def test_side_half_boxes_pass_the_library_check():
    """train_crop_scale = 0.25 (side 0.5): every drawn box keeps an fp32 side >= 0.5 inside [0, 1] — what vaa_crop_resize_* accepts."""
    t = RandomPatchTransform("cpu", train_crop="random", train_crop_scale=0.25)
    _seed()
    boxes = t._crop_boxes(256, torch.zeros(1, requires_grad=True))
    side = boxes[:, 2:] - boxes[:, :2]
    assert side.dtype == f32 and (side >= f32(0.5)).all() and (boxes >= 0).all() and (boxes <= 1).all()


def test_crop_with_the_embed_path_and_resize_goes_planar(monkeypatch):
    """With a model that exposes its patch-embed weights the crop still takes the planar K1 -> K9 path (K2' cannot take the cropped gradient);
    resize_patch=True composes unchanged."""
    calls = []
    _stub(monkeypatch, calls)
    t = RandomPatchTransform("cpu", train_crop="center")
    t.embed_with = object()  # never asked for its weights
    t.apply_random_patch_batch(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD, True)
    assert [c[0] for c in calls] == ["PatchApply", "CropResize"]
    calls.clear()
    t = RandomPatchTransform("cpu", resize_patch=True, train_crop="center")
    t.apply_random_patch_batch(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD, True)
    assert [c[0] for c in calls] == ["PatchApplyResized", "CropResize"]


def test_refusals(monkeypatch, tmp_path):
    frames, patch = _frames(), torch.rand(3, PH, PW)
    with pytest.raises(ValueError, match="train_crop must be"):
        RandomPatchTransform("cpu", train_crop="corner")
    for bad in (0.2, 1.5, float("nan")):
        with pytest.raises(ValueError, match="train_crop_scale"):
            RandomPatchTransform("cpu", train_crop="center", train_crop_scale=bad)
    with pytest.raises(ValueError, match="grad_sink is not available with train_crop"):
        RandomPatchTransform("cpu", train_crop="center").apply_random_patch_batch(frames, patch, MEAN, STD, True, grad_sink={})
    fused(monkeypatch)
    with pytest.raises(ValueError, match="maskidx_sweep: train_crop is not supported"):
        attacker(monkeypatch, tmp_path, train_crop="center", maskidx_sweep=[[0], [0, 1, 2]])
    assert attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0, 1, 2]]).randomPatchTransform.train_crop is None


def test_a_cropping_transform_stays_off_the_fused_single_patch_paths(monkeypatch, tmp_path):
    from roboticattack_amd.optim import PatchOptimizer

    monkeypatch.delenv("VAA_FUSED_EPILOGUE", raising=False)
    monkeypatch.delenv("VAA_FUSED_EMBED_GRAD", raising=False)
    opt = PatchOptimizer(torch.zeros(3, 8, 8), 1e-3, "adamW")
    att = attacker(monkeypatch, tmp_path)
    assert att.fused_ddp_available() and att.fused_update_sink(opt) == {}
    for mode in ("center", "random"):
        att = attacker(monkeypatch, tmp_path, train_crop=mode, train_crop_scale=0.81)
        t = att.randomPatchTransform
        assert (t.train_crop, t.train_crop_scale) == (mode, 0.81)
        assert not att.fused_ddp_available() and att.fused_update_sink(opt) is None


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(1, 6, 224, 224, dtype=torch.bfloat16)
    box = np.array([[0, 0, 1, 1]], f32)
    for f in (ops.crop_resize_fwd, ops.crop_resize_bwd, ops.CropResize.apply):
        with pytest.raises(_lib.VaaError, match="no CPU fallback"):
            f(x, box)


# ---- entry points ----
def test_entry_point_argument_errors_without_gpu():
    """vaa_crop_resize_fwd / _bwd refuse, before any launch: a NULL pointer, a misaligned base, a bad box; B == 0 returns VAA_OK. Host buffers
    stand in for the device pointers (nothing dereferences them: every call here returns before a launch)."""
    L = _lib.lib()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15
    p = lambda off=0: ctypes.c_void_p(base + off)
    good = (ctypes.c_float * 8)(0, 0, 1, 1, 0.25, 0.25, 0.75, 0.75)
    box = lambda *v: (ctypes.c_float * 4)(*v)
    for f in (L.vaa_crop_resize_fwd, L.vaa_crop_resize_bwd):
        assert f(None, None, None, 0, None, None) == 0  # empty batch: nothing validated, nothing launched
        assert f(p(), good, p(1024), -1, p(2048), None) == -1 and b"bad batch size" in L.vaa_last_error()
        for args in ((None, good, p(1024), p(2048)), (p(), None, p(1024), p(2048)), (p(), good, None, p(2048)), (p(), good, p(1024), None)):
            assert f(args[0], args[1], args[2], 2, args[3], None) == -1 and b"null pointer" in L.vaa_last_error()
        for args in ((p(2), p(1024), p(2048)), (p(), p(1028), p(2048)), (p(), p(1024), p(2056))):
            assert f(args[0], good, args[1], 2, args[2], None) == -1 and b"16-byte aligned" in L.vaa_last_error()
        nan, inf = float("nan"), float("inf")
        for bad in ((0, 0, 0.4, 1), (0, 0, 1, 0.49), (-0.1, 0, 0.9, 1), (0, 0.1, 1, 1.1), (0.6, 0, 0.5, 1), (0.5, 0, 0.5, 1), (nan, 0, 1, 1), (0, 0, inf, 1),
                    (0, nan, 1, 1), (0.3, 0, 0.79, 1)):
            assert f(p(), box(*bad), p(1024), 1, p(2048), None) == -1 and b"side of at least 0.5" in L.vaa_last_error(), bad
