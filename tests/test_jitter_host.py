"""CPU tests of the colour jitter's host side: RNG consumption with the flag off and on, the refusals, the routing off the fused single-patch
paths, the CLI flags, the argument errors of the three entry points, and the fp32-vs-fp64 baseline of the restatement (tests/jitter_ref.py)
the GPU tests' tolerances are derived from."""
import random

import numpy as np
import pytest
import torch

import jitter_ref
from roboticattack_amd import _lib, ops, synthetic
from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
from roboticattack_amd.transform import RandomPatchTransform
from sweep_harness import attacker, fused, wrapper

MEAN, STD = [torch.tensor(MEAN0), torch.tensor(MEAN1)], [torch.tensor(STD0), torch.tensor(STD1)]
B, PH, PW = 4, 50, 40


def _seed():
    random.seed(42)
    np.random.seed(42)


def _state():
    return random.getstate(), np.random.get_state()


def _same(a, b):
    return a[0] == b[0] and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def _stub(monkeypatch, name, calls):
    def apply(patch, img, *rest):
        calls.append((name, rest))
        return torch.zeros((img.shape[0], 6, 224, 224), dtype=torch.bfloat16)

    monkeypatch.setattr(getattr(ops, name), "apply", staticmethod(apply), raising=False)


def _frames():
    return torch.from_numpy(synthetic.synth_images(3, B, "smooth"))


@pytest.mark.parametrize("geometry", [True, False])
def test_jitter_off_consumes_todays_rng_stream(monkeypatch, geometry):
    """colorjitter=False: the call draws what draw_params draws — randint(x), randint(y), then with geometry numpy's rand [+ three uniforms] per
    image — and nothing else (the seed-42 stream golden and every trajectory golden depend on it)."""
    calls = []
    _stub(monkeypatch, "PatchApply", calls)
    t = RandomPatchTransform("cpu")
    patch = torch.rand(3, PH, PW)
    _seed()
    t.apply_random_patch_batch(_frames(), patch, MEAN, STD, geometry, colorjitter=False)
    after_call = _state()
    xy_call, th_call = t.last_params
    _seed()
    xy, th = t.draw_params(B, PH, PW, geometry)
    assert _same(after_call, _state()) and np.array_equal(xy, xy_call) and np.array_equal(th, th_call)
    # ... and the draw order itself, written out (appply_random_transform.py:120-128)
    _seed()
    for b in range(B):
        assert (random.randint(0, 224 - PW), random.randint(0, 224 - PH)) == tuple(xy[b])
        if geometry and not np.random.rand() < 0.2:
            [np.random.uniform(-1, 1) for _ in range(3)]
    assert _same(after_call, _state())
    assert [c[0] for c in calls] == ["PatchApply"] and t.last_jitter is None


@pytest.mark.parametrize("colorjitter,strength", [(True, (0.2, 0.2, 0.2)), ((0.1, 0.3, 0.0), (0.1, 0.3, 0.0))])
def test_jitter_on_draws_three_factors_per_image_behind_the_placement(monkeypatch, colorjitter, strength):
    """colorjitter on: the existing placement draws first, then 3*B calls random.uniform(1 - s_k, 1 + s_k), image-major in order brightness,
    contrast, saturation; kept as last_jitter [B,3] float32 and handed to the Function."""
    calls = []
    _stub(monkeypatch, "PatchApplyJittered", calls)
    t = RandomPatchTransform("cpu")
    patch = torch.rand(3, PH, PW)
    _seed()
    t.apply_random_patch_batch(_frames(), patch, MEAN, STD, True, colorjitter=colorjitter)
    after_call = _state()
    _seed()
    xy, th = t.draw_params(B, PH, PW, True)
    want = np.array([[random.uniform(1 - s, 1 + s) for s in strength] for _ in range(B)], np.float32)
    assert _same(after_call, _state())
    assert t.last_jitter.dtype == np.float32 and t.last_jitter.shape == (B, 3) and np.array_equal(t.last_jitter, want)
    for k, s in enumerate(strength):
        assert (want[:, k] >= np.float32(1 - s)).all() and (want[:, k] <= np.float32(1 + s)).all()
    assert np.array_equal(t.last_params[0], xy) and np.array_equal(t.last_params[1], th)
    assert [c[0] for c in calls] == ["PatchApplyJittered"] and np.array_equal(calls[0][1][0].numpy(), want)  # factors: the first argument behind the frames


def test_refusals(monkeypatch, tmp_path):
    frames, patch = _frames(), torch.rand(3, PH, PW)
    with pytest.raises(ValueError, match="colorjitter with resize_patch is not supported"):
        RandomPatchTransform("cpu", resize_patch=True).apply_random_patch_batch(frames, patch, MEAN, STD, True, colorjitter=True)
    with pytest.raises(ValueError, match="grad_sink is not available with colorjitter"):
        RandomPatchTransform("cpu").apply_random_patch_batch(frames, patch, MEAN, STD, True, colorjitter=True, grad_sink={})
    with pytest.raises(ValueError, match="three strengths"):
        RandomPatchTransform("cpu").apply_random_patch_batch(frames, patch, MEAN, STD, True, colorjitter=(0.2, 0.2))
    fused(monkeypatch)
    with pytest.raises(ValueError, match="maskidx_sweep: colorjitter is not supported"):
        attacker(monkeypatch, tmp_path, colorjitter=True, maskidx_sweep=[[0], [0, 1, 2]])
    assert attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0, 1, 2]]).randomPatchTransform.colorjitter is False


def test_a_jittering_transform_stays_off_the_fused_single_patch_paths(monkeypatch, tmp_path):
    from roboticattack_amd.optim import PatchOptimizer

    monkeypatch.delenv("VAA_FUSED_EPILOGUE", raising=False)
    monkeypatch.delenv("VAA_FUSED_EMBED_GRAD", raising=False)
    att = attacker(monkeypatch, tmp_path)
    opt = PatchOptimizer(torch.zeros(3, 8, 8), 1e-3, "adamW")
    assert att.fused_ddp_available() and att.fused_update_sink(opt) == {}
    jit = attacker(monkeypatch, tmp_path, colorjitter=True)
    assert jit.randomPatchTransform.colorjitter is True
    assert not jit.fused_ddp_available() and jit.fused_update_sink(opt) is None


def test_cli_flags():
    w = wrapper("uada_wrapper_ddp_jitter")
    from roboticattack_amd import cli

    a = w.arg_parser([])
    assert a.colorjitter is False and tuple(a.colorjitter_strength) == (0.2, 0.2, 0.2) and cli.colorjitter_arg(a) is False
    a = w.arg_parser(["--colorjitter", "true"])
    assert cli.colorjitter_arg(a) == (0.2, 0.2, 0.2)
    a = w.arg_parser(["--colorjitter", "true", "--colorjitter_strength", "0.1,0.3,0.05"])
    assert cli.colorjitter_arg(a) == (0.1, 0.3, 0.05)
    with pytest.raises(SystemExit):
        w.arg_parser(["--colorjitter_strength", "0.1,0.3"])


def test_entry_point_argument_errors_without_gpu():
    L = _lib.lib()
    assert L.vaa_version() >= 101
    assert L.vaa_patch_jitter_ws_bytes(0, 50, 50) == 0 and L.vaa_patch_jitter_ws_bytes(1, 50, 50) == 0  # a single image writes gpatch itself
    assert L.vaa_patch_jitter_ws_bytes(8, 50, 40) == 8 * 3 * 50 * 40 * 4  # one partial per image
    # empty batches return before anything is validated or launched
    assert L.vaa_patch_jitter_fwd(None, 50, 50, None, None, 0, None, None) == 0
    assert L.vaa_patch_jitter_bwd(None, None, 50, 50, None, None, 0, None, None, 0, None) == 0
    assert L.vaa_patch_jitter_fwd(None, 50, 50, None, None, 2, None, None) == -1 and b"null pointer" in L.vaa_last_error()
    assert L.vaa_patch_jitter_bwd(None, None, 50, 50, None, None, 2, None, None, 0, None) == -1 and b"null pointer" in L.vaa_last_error()


@pytest.mark.parametrize("name", list(jitter_ref.CASES) + ["saturated"])
def test_restatement_fp32_against_fp64_baseline(name):
    """The measured baseline e_ref (fp32 restatement against fp64, forward and gradient) of the GPU tests' inputs, and the facts about those
    inputs the GPU tests rely on: at most 1 % of the texels are left out of the gradient comparison, and kappa = 0.5 is present — there the
    adjoint WITHOUT the whole-patch mean term is wrong by orders of magnitude more than the tolerance."""
    c = jitter_ref.case(name)
    tol_f, tol_g = jitter_ref.tolerances(name)
    out = 1.0 - float(c["keep"].float().mean())
    print(f"{name}: e_ref_fwd={c['e_fwd']:.3e} e_ref_grad_rel={c['e_grad_rel']:.3e} tol_f={tol_f:.3e} tol_g={tol_g:.3e} left out={out:.4%}")
    assert c["e_fwd"] < 1e-6 and c["e_grad_rel"] < 1e-5  # fp32 rounding only: no gate differs between the fp32 and the fp64 restatement
    assert out <= 0.01
    assert float(c["patch"].min()) >= 0.0 and float(c["patch"].max()) <= 1.0
    if name == "saturated":
        p = c["patch"]
        assert 0.15 < float((p == 0).float().mean()) < 0.25 and 0.15 < float((p == 1).float().mean()) < 0.25
        # brightness alone: beta*G where beta*p <= 1 (p = 0 included: the gate's bounds are inclusive), exactly 0 where beta*p > 1
        want = sum(b * c["gout"][i].double() * ((b * p.double()) <= 1) for i, b in enumerate(c["factors"][:, 0].double()))
        assert torch.allclose(c["grad64"], want, rtol=0, atol=1e-12)
        return
    assert any(float(k) == 0.5 for k in c["factors"][:, 1])
    no_mean = jitter_ref.jitter_grad(c["patch"], c["factors"], c["gout"], detach_mean=True)
    miss = float((no_mean - c["grad64"])[:, c["keep"]].abs().max()) / float(c["grad64"][:, c["keep"]].abs().max())
    print(f"{name}: adjoint without the mean term misses by {miss:.3e} of max|ref| ({miss / tol_g:.0f} x tol_g)")
    assert miss > 10 * tol_g


class _Model:
    """Stands in for a model that exposes its patch-embed weights: six distinguishable objects."""
    emb = tuple(f"emb{k}" for k in range(6))

    def patch_embed_params(self):
        return self.emb


@pytest.mark.parametrize("embed", [False, True], ids=["planar", "embed"])
@pytest.mark.parametrize("site", ["plain", "plain_sink", "resized", "jittered", "paste"])
def test_every_paste_site_hands_its_function_the_same_arguments(monkeypatch, site, embed):
    """The one paste tail behind apply_random_patch_batch (plain, resize_patch, colorjitter) and _paste: each site's Function — the planar one,
    or with `embed_with` the *Embed one — receives, behind (patch, frames), exactly [sizes | factors,] xy, theta, geometry, mask mode, mean6,
    std6 [, the six patch-embed parameters] [, grad_sink]; _paste passes MASK_NE_M100 and geometry False, and only the plain site has a sink."""
    from roboticattack_amd.transform import _six

    name = {"plain": "PatchApply", "plain_sink": "PatchApply", "resized": "PatchApplyResized", "jittered": "PatchApplyJittered",
            "paste": "PatchApply"}[site] + ("Embed" if embed else "")
    calls = []
    for n in ("PatchApply", "PatchApplyResized", "PatchApplyJittered"):
        _stub(monkeypatch, n, calls)
        _stub(monkeypatch, n + "Embed", calls)
    t = RandomPatchTransform("cpu", resize_patch=(site == "resized"))
    t.embed_with = _Model() if embed else None
    patch = torch.rand(3, PH, PW, requires_grad=True)
    sink = {} if site == "plain_sink" else None
    _seed()
    if site == "paste":
        out = t.random_paste_patch(_frames(), patch, MEAN, STD)
    else:
        out = t.apply_random_patch_batch(_frames(), patch, MEAN, STD, True, colorjitter=(site == "jittered"), grad_sink=sink)
    assert isinstance(out, ops.PatchEmbeds) == embed
    assert [c[0] for c in calls] == [name]
    rest = list(calls[0][1])
    lead = {"resized": t.last_sizes, "jittered": t.last_jitter}.get(site)
    if lead is not None:
        got = rest.pop(0)
        assert np.array_equal(got.numpy() if isinstance(got, torch.Tensor) else got, lead)
    xy, theta = rest[:2]
    assert np.array_equal(xy.numpy(), t.last_params[0]) and np.array_equal(theta.numpy(), t.last_params[1])
    mean6, std6 = _six(MEAN, STD)
    want = [site != "paste", ops.MASK_NE_M100 if site == "paste" else ops.MASK_LT_M20, mean6, std6] + (list(_Model.emb) if embed else [])
    if site.startswith("plain"):
        want.append(sink)
    assert rest[2:] == want and rest[2] is want[0] and (sink is None or rest[-1] is sink)
