"""CPU-only checks of the scene-lighting jitter (K10): the references of tests/scene_ref.py against each other and against torch autograd, the
bounds' self-test and the near-gate share on the GPU tests' own inputs, the host layer (factors, flags, RNG consumption, refusals) and the entry
points' argument errors. No kernel is launched."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

import scene_ref as SR
from conftest import ROOT
from roboticattack_amd import _lib, ops, synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
from roboticattack_amd.transform import SCENE_JITTER_STRENGTH, RandomPatchTransform, scene_strength
from sweep_harness import attacker, fused

MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]
B, PH, PW = 4, 50, 40
f32 = np.float32


# ---- references ----
def _small(seed=0, b=3, h=6, w=5):
    """A small problem with every clamp engaged somewhere: x float64 [b,6,h,w], g, factors (the references take any plane size)."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-2.6, 2.6, (b, 6, h, w))
    g = rs.randn(b, 6, h, w)
    F = SR.factors(rs.uniform(-0.3, 0.3, b), rs.uniform(0.5, 1.6, b), rs.uniform(0.4, 1.7, b), rs.uniform(-0.5, 0.5, b))
    return x, g, F


def test_numpy_adjoint_equals_torch_autograd():
    x, g, F = _small()
    xt = torch.tensor(x, requires_grad=True)
    out = SR.fwd_torch(xt, F)
    out.backward(torch.tensor(g))
    gx, _, near_gate, _ = SR.bwd64(g, x, F, round_s=False)
    # fwd_torch does not round the mean to fp32: the outputs differ by < 1e-6, the gradients agree to fp64 (the gates are the same away from them)
    assert np.abs(out.detach().numpy() - SR.fwd64(x, F)).max() < 1e-6
    assert not near_gate.any()
    assert np.abs(gx - xt.grad.numpy()).max() <= 1e-12 * np.abs(gx).max()
    st = SR.stages64(x, F)
    for k in ("pre1", "pre2", "pre3", "pre4"):  # every clamp is engaged on both sides somewhere, so every gate is exercised
        assert (st[k] < 0).any() and (st[k] > 1).any(), k


def test_adjoint_identity_in_fp64():
    """<J v, w> = <v, J^T w> with J v by central differences of the (piecewise linear) forward."""
    x, g, F = _small(1)
    rs = np.random.RandomState(7)
    v = rs.randn(*x.shape)
    h = 1e-7
    fwd = lambda z: SR.fwd_torch(torch.tensor(z), F).numpy()  # the unrounded mean: exactly piecewise linear
    Jv = (fwd(x + h * v) - fwd(x - h * v)) / (2 * h)
    xt = torch.tensor(x, requires_grad=True)
    SR.fwd_torch(xt, F).backward(torch.tensor(g))
    lhs, rhs = float((Jv * g).sum()), float((v * SR.bwd64(g, x, F, round_s=False)[0]).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_scene_factors():
    F = ops.scene_factors([0.1, 0.0], [1.2, 1.0], [0.8, 1.0], [0.0, 0.0])
    assert F.dtype == f32 and F.shape == (2, 12)
    assert np.array_equal(F[:, 3:], np.tile(np.eye(3, dtype=f32).reshape(9), (2, 1)))  # h = 0: exactly the identity
    assert np.array_equal(F[1], np.array([0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1], f32))
    h = np.linspace(-0.5, 0.5, 41)
    F = ops.scene_factors(np.zeros(41), np.ones(41), np.ones(41), h)
    assert np.array_equal(F, SR.factors(np.zeros(41), np.ones(41), np.ones(41), h))  # the reference's own construction
    R = F[:, 3:].reshape(41, 3, 3).astype(np.float64)
    assert np.abs(R.sum(axis=2) - 1.0).max() <= 3 * 2.0 ** -24 * np.abs(R).sum(axis=2).max()  # every row sums to 1 within fp32 rounding
    half = SR.hue_matrix(0.5)
    assert np.allclose(half @ half, np.eye(3), atol=1e-12)  # two half turns


# ---- bounds ----
def test_near_gate_share_of_the_gpu_inputs():
    """On the GPU tests' own inputs the reference classifies at most 0.5 % of every case's elements as near-gate (a condition on the inputs: the
    adjoint is compared on at least 99.5 % of every image), and the forward's pre-clamp error stays far below the gate margin."""
    ref = SR.reference()
    share = ref["near_gate"].reshape(len(SR.CASES), -1).mean(axis=1)
    print({c: float(s) for c, s in zip(SR.CASES, share)}, "pre-clamp error bound", ref["pre_err"])
    assert (share <= 0.005).all(), dict(zip(SR.CASES, share))
    assert ref["pre_err"] < 0.4 * SR.GATE_MARGIN
    # the cases are what they claim: delta = +-1 shuts every first gate; the other images keep most of theirs open
    shut = ref["shut1"].reshape(len(SR.CASES), -1).mean(axis=1)
    assert shut[7] == 1.0 and shut[8] == 1.0 and (shut[[0, 1, 3, 4, 5, 6, 9]] < 0.5).all()
    assert (ref["gx"][7:9] == 0).all() and (ref["gx_bound"][7:9] == 0).all()
    assert np.isfinite(ref["fwd_bound"]).all() and np.isfinite(ref["gx_bound"]).all()


@pytest.mark.parametrize("fault", ["gray_mean", "hue_t", "mul_brightness"])
def test_perturbation_breaks_the_forward_bound(fault):
    """A reference with one deliberately wrong stage (rounded to bf16 as a kernel would) violates the forward bound on the generic image; the
    right one (rounded alike) holds it."""
    xb, _, F = SR.inputs()
    x, F1 = SR.bits_f32(xb[:1]).astype(np.float64), F[:1]
    ref = SR.reference()
    want, bound = ref["fwd"][:1], ref["fwd_bound"][:1]
    rnd = lambda v: SR.bits_f32(SR.f32_to_bf16_bits(v.astype(f32))).astype(np.float64)
    assert SR.worst_ratio(rnd(SR.fwd64(x, F1)), want, bound)[0] <= 1.0
    worst, _ = SR.worst_ratio(rnd(SR.fwd64(x, F1, wrong=fault)), want, bound)
    assert worst > 1.0, fault


def test_perturbation_breaks_the_adjoint_bound():
    """Adjoints with one wrong stage — the whole-image mean term dropped; the hue matrix not transposed — violate the adjoint bound outside the
    near-gate set; the right one (rounded to bf16) holds it."""
    xb, gb, F = SR.inputs()
    x, g, F1 = SR.bits_f32(xb[:1]).astype(np.float64), SR.bits_f32(gb[:1]).astype(np.float64), F[:1]
    ref = SR.reference()
    want, bound, skip = ref["gx"][:1], ref["gx_bound"][:1], ref["near_gate"][:1]
    rnd = lambda v: SR.bits_f32(SR.f32_to_bf16_bits(v.astype(f32))).astype(np.float64)
    assert SR.worst_ratio(rnd(want), want, bound, skip)[0] <= 1.0
    st = SR.stages64(x, F1)
    delta, kappa, sigma, omk, oms, R = st["F"]
    mean, std = st["norm"]
    w = SR.W32.reshape(1, 1, 3, 1)
    for wrong in ("no_mean_term", "hue_not_transposed"):
        G4 = np.where(SR.gate(st["pre4"]), g.reshape(st["v"].shape) / std, 0.0)
        G3 = np.einsum("bdc,btcn->btdn" if wrong == "hue_not_transposed" else "bcd,btcn->btdn", R, G4)
        G3 = np.where(SR.gate(st["pre3"]), G3, 0.0)
        G2 = np.where(SR.gate(st["pre2"]), sigma[0] * G3 + oms[0] * w * G3.sum(axis=2, keepdims=True), 0.0)
        s = 0.0 if wrong == "no_mean_term" else G2.mean(axis=3, keepdims=True)
        gx = np.where(SR.gate(st["pre1"]), (kappa[0] * G2 + omk[0] * s) * std, 0.0).reshape(x.shape)
        worst, _ = SR.worst_ratio(rnd(gx), want, bound, skip)
        assert worst > 1.0, wrong


# ---- flags ----
def _wrapper(fname):
    spec = importlib.util.spec_from_file_location("scene_" + fname[:-3], os.path.join(ROOT, "VLAAttacker", fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("fname", ["UADA_wrapper.py", "UADA_wrapper_ddp.py", "UPA_wrapper.py", "TMA_wrapper.py"])
def test_cli_flags(fname):
    from roboticattack_amd import cli

    w = _wrapper(fname)
    a = w.arg_parser([])
    assert a.scene_jitter is False and a.scene_jitter_strength == (0.2, 0.2, 0.2, 0.05) and cli.scene_jitter_arg(a) == {"scene_jitter": False}
    a = w.arg_parser(["--scene_jitter", "true"])
    assert cli.scene_jitter_arg(a) == {"scene_jitter": (0.2, 0.2, 0.2, 0.05)}
    a = w.arg_parser(["--scene_jitter", "true", "--scene_jitter_strength", "0.1,0.3,0.25,0.02"])
    assert cli.scene_jitter_arg(a) == {"scene_jitter": (0.1, 0.3, 0.25, 0.02)}
    for bad in ("0.1,0.2,0.3", "0.1,0.2,0.3,0.6", "-0.1,0.2,0.3,0.05", "a,b,c,d"):
        with pytest.raises(SystemExit):
            w.arg_parser(["--scene_jitter_strength", bad])


def test_strengths():
    assert scene_strength(None) is None and scene_strength(False) is None and scene_strength(True) == SCENE_JITTER_STRENGTH == (0.2, 0.2, 0.2, 0.05)
    assert scene_strength([0.1, 0.2, 0.3, 0.04]) == (0.1, 0.2, 0.3, 0.04)
    for bad in ((0.1, 0.2, 0.3), (0.1, 0.2, 0.3, 0.6), (-0.1, 0.2, 0.3, 0.05), (1.5, 0.2, 0.3, 0.05), (0.1, 0.2, float("nan"), 0.05)):
        with pytest.raises(ValueError, match="scene_jitter must be"):
            scene_strength(bad)
        with pytest.raises(ValueError, match="scene_jitter must be"):
            RandomPatchTransform("cpu").set_scene_jitter(bad)


# ---- draws ----
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

    def scene(x, factors, mean6, std6):
        calls.append(("SceneJitter", np.array(factors, copy=True), tuple(mean6), tuple(std6)))
        return x

    monkeypatch.setattr(ops.CropResize, "apply", staticmethod(crop), raising=False)
    monkeypatch.setattr(ops.SceneJitter, "apply", staticmethod(scene), raising=False)


def _frames():
    return torch.from_numpy(synthetic.synth_images(3, B, "smooth"))


@pytest.mark.parametrize("geometry", [True, False])
def test_scene_jitter_off_consumes_todays_rng_stream(monkeypatch, geometry):
    """Off (the default, and set explicitly to None / False): the draws of draw_params and nothing else; no SceneJitter."""
    ts = [RandomPatchTransform("cpu"), RandomPatchTransform("cpu"), RandomPatchTransform("cpu")]
    ts[1].set_scene_jitter(None)
    ts[2].set_scene_jitter(False)
    for t in ts:
        calls = []
        _stub(monkeypatch, calls)
        patch = torch.rand(3, PH, PW, requires_grad=True)
        _seed()
        t.apply_random_patch_batch(_frames(), patch, MEAN, STD, geometry)
        after = _state()
        _seed()
        t.draw_params(B, PH, PW, geometry)
        assert _same(after, _state()) and [c[0] for c in calls] == ["PatchApply"] and t.last_scene is None and t.scene_jitter is None


@pytest.mark.parametrize("colorjitter,crop", [(False, None), (True, "random"), (False, "center")])
def test_scene_draws_four_per_image_behind_every_other_draw(monkeypatch, colorjitter, crop):
    calls = []
    _stub(monkeypatch, calls)
    t = RandomPatchTransform("cpu", train_crop=crop)
    s = (0.1, 0.3, 0.25, 0.02)
    t.set_scene_jitter(s)
    patch = torch.rand(3, PH, PW, requires_grad=True)
    _seed()
    t.apply_random_patch_batch(_frames(), patch, MEAN, STD, True, colorjitter=colorjitter)
    after = _state()
    _seed()
    t.draw_params(B, PH, PW, True)
    if colorjitter:
        [random.uniform(0.8, 1.2) for _ in range(3 * B)]
    if crop == "random":
        side = float(center_side())
        [random.uniform(0, 1 - side) for _ in range(2 * B)]
    d = np.array([[random.uniform(-s[0], s[0]), random.uniform(1 - s[1], 1 + s[1]), random.uniform(1 - s[2], 1 + s[2]), random.uniform(-s[3], s[3])]
                  for _ in range(B)])  # image-major: delta, kappa, sigma, h
    assert _same(after, _state())
    want = ["PatchApplyJittered" if colorjitter else "PatchApply"] + (["CropResize"] if crop else []) + ["SceneJitter"]
    assert [c[0] for c in calls] == want  # K10 is the last stage, behind K9
    F = calls[-1][1]
    assert F.dtype == f32 and F.shape == (B, 12) and np.array_equal(F, t.last_scene)
    assert np.array_equal(F, ops.scene_factors(d[:, 0], d[:, 1], d[:, 2], d[:, 3]))
    assert calls[-1][2] == tuple(MEAN0 + MEAN1) and calls[-1][3] == tuple(STD0 + STD1)


def center_side():
    from roboticattack_amd.transform import center_crop_box

    box = center_crop_box(0.9)
    return box[2] - box[0]


def test_calls_that_are_not_differentiable_make_no_draw_and_no_launch(monkeypatch):
    """The loops' validation passes (a patch without requires_grad, or under no_grad): zero extra RNG calls, no SceneJitter."""
    for grad, nograd in ((False, False), (True, True)):
        calls = []
        _stub(monkeypatch, calls)
        t = RandomPatchTransform("cpu")
        t.set_scene_jitter(True)
        patch = torch.rand(3, PH, PW, requires_grad=grad)
        _seed()
        with torch.set_grad_enabled(not nograd):
            t.random_paste_patch(_frames(), patch, MEAN, STD)
        after = _state()
        _seed()
        t.draw_params(B, PH, PW, False)
        assert _same(after, _state()) and [c[0] for c in calls] == ["PatchApply"] and t.last_scene is None


def test_scene_jitter_composes_and_goes_planar(monkeypatch):
    """With a model that exposes its patch-embed weights the step still takes the planar K1 -> K10 path (K2' cannot take the gradient behind
    K10); resize_patch=True composes unchanged; the un-warped pastes jitter too."""
    calls = []
    _stub(monkeypatch, calls)
    t = RandomPatchTransform("cpu")
    t.set_scene_jitter(True)
    t.embed_with = object()  # never asked for its weights
    t.apply_random_patch_batch(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD, True)
    assert [c[0] for c in calls] == ["PatchApply", "SceneJitter"]
    calls.clear()
    t = RandomPatchTransform("cpu", resize_patch=True, train_crop="center")
    t.set_scene_jitter(True)
    t.apply_random_patch_batch(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD, True)
    assert [c[0] for c in calls] == ["PatchApplyResized", "CropResize", "SceneJitter"]
    calls.clear()
    t.resize_patch = False
    t.paste_patch_fix(_frames(), torch.rand(3, PH, PW, requires_grad=True), MEAN, STD)
    assert [c[0] for c in calls] == ["PatchApply", "CropResize", "SceneJitter"]


def test_refusals(monkeypatch, tmp_path):
    frames, patch = _frames(), torch.rand(3, PH, PW)
    t = RandomPatchTransform("cpu")
    t.set_scene_jitter(True)
    with pytest.raises(ValueError, match="grad_sink is not available with scene_jitter"):
        t.apply_random_patch_batch(frames, patch, MEAN, STD, True, grad_sink={})
    t.embed_with = object()
    with pytest.raises(ValueError, match="apply_sweep_batch is not available with scene_jitter"):
        t.apply_sweep_batch(frames, torch.rand(2, 3, PH, PW), MEAN, STD, True, {})
    fused(monkeypatch)
    with pytest.raises(ValueError, match="maskidx_sweep: scene_jitter is not supported"):
        attacker(monkeypatch, tmp_path, scene_jitter=True, maskidx_sweep=[[0], [0, 1, 2]])
    assert attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0, 1, 2]]).randomPatchTransform.scene_jitter is None
    with pytest.raises(ValueError, match="scene_jitter must be"):
        attacker(monkeypatch, tmp_path, scene_jitter=(0.2, 0.2, 0.2))


def test_a_scene_jittering_transform_stays_off_the_fused_single_patch_paths(monkeypatch, tmp_path):
    from roboticattack_amd.optim import PatchOptimizer

    monkeypatch.delenv("VAA_FUSED_EPILOGUE", raising=False)
    monkeypatch.delenv("VAA_FUSED_EMBED_GRAD", raising=False)
    opt = PatchOptimizer(torch.zeros(3, 8, 8), 1e-3, "adamW")
    att = attacker(monkeypatch, tmp_path)
    assert att.fused_ddp_available() and att.fused_update_sink(opt) == {}
    att = attacker(monkeypatch, tmp_path, scene_jitter=True)
    assert att.randomPatchTransform.scene_jitter == (0.2, 0.2, 0.2, 0.05)
    assert not att.fused_ddp_available() and att.fused_update_sink(opt) is None


def test_ops_refuse_cpu_tensors():
    x = torch.zeros(1, 6, 224, 224, dtype=torch.bfloat16)
    F = ops.scene_factors([0.0], [1.0], [1.0], [0.0])
    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.scene_jitter_fwd(x, F)
    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.scene_jitter_bwd(x, x, F)
    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.SceneJitter.apply(x, F)


# ---- entry points ----
def test_entry_point_argument_errors_without_gpu():
    """vaa_scene_jitter_fwd / _bwd refuse, before any launch: B < 0, a NULL pointer, a misaligned base, a bad factor, a bad std, a missing or
    small workspace; B == 0 returns VAA_OK. Host buffers stand in for the device pointers (nothing dereferences them: every call here returns
    before a launch)."""
    L = _lib.lib()
    assert L.vaa_scene_jitter_ws_bytes(0) == 0 and L.vaa_scene_jitter_ws_bytes(-1) == 0
    assert L.vaa_scene_jitter_ws_bytes(1) == 2 * 14 * 3 * 8 * 2 and L.vaa_scene_jitter_ws_bytes(64) == 64 * L.vaa_scene_jitter_ws_bytes(1)
    raw = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(raw) + 15) & ~15
    p = lambda off=0: ctypes.c_void_p(base + off)
    ident = (0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1)
    row = lambda *v: (ctypes.c_float * 24)(*(tuple(v) + ident))
    good = row(*ident)
    mean, std = _lib.f32x(MEAN0 + MEAN1), _lib.f32x(STD0 + STD1)
    need = L.vaa_scene_jitter_ws_bytes(2)

    def fwd(x=p(), fh=good, fd=p(1024), m=mean, s=std, n=2, out=p(2048), ws=p(4096), wsb=need):
        return L.vaa_scene_jitter_fwd(x, fh, fd, m, s, n, out, ws, wsb, None)

    def bwd(x=p(), fh=good, fd=p(1024), m=mean, s=std, n=2, out=p(2048), ws=p(4096), wsb=need, g=p(3072)):
        return L.vaa_scene_jitter_bwd(g, x, fh, fd, m, s, n, out, ws, wsb, None)

    nan, inf = float("nan"), float("inf")
    for f in (fwd, bwd):
        assert f(None, None, None, None, None, 0, None, None, 0) == 0  # empty batch: nothing validated, nothing launched
        assert f(n=-1) == -1 and b"bad batch size" in L.vaa_last_error()
        for kw in (dict(x=None), dict(fh=None), dict(fd=None), dict(m=None), dict(s=None), dict(out=None)):
            assert f(**kw) == -1 and b"null pointer" in L.vaa_last_error(), kw
        for kw in (dict(x=p(2)), dict(fd=p(1028)), dict(out=p(2056))):
            assert f(**kw) == -1 and b"16-byte aligned" in L.vaa_last_error(), kw
        for k, v in ((0, nan), (0, inf), (1, nan), (2, -inf), (3, nan), (11, inf)):
            bad = list(ident)
            bad[k] = v
            assert f(fh=row(*bad)) == -1 and b"is not finite" in L.vaa_last_error(), (k, v)
        for k in (1, 2):
            bad = list(ident)
            bad[k] = -0.01
            assert f(fh=row(*bad)) == -1 and b"need kappa >= 0 and sigma >= 0" in L.vaa_last_error()
        for v in (0.0, -0.5, nan, inf):
            bad_std = list(STD0 + STD1)
            bad_std[4] = v
            assert f(s=_lib.f32x(bad_std)) == -1 and b"std > 0" in L.vaa_last_error(), v
        bad_mean = list(MEAN0 + MEAN1)
        bad_mean[0] = nan
        assert f(m=_lib.f32x(bad_mean)) == -1 and b"std > 0" in L.vaa_last_error()
        assert f(ws=None) == -4 and f(wsb=need - 1) == -4 and f(ws=p(4100)) == -4 and b"workspace" in L.vaa_last_error()
    assert bwd(g=None) == -1 and b"null pointer" in L.vaa_last_error()
    assert bwd(g=p(3074)) == -1 and b"16-byte aligned" in L.vaa_last_error()
