"""The COMPOSITION of the model-side kernels: the bf16 `OpenVLAShaped` on the GPU, in every dispatch form of LlamaLayer / VitBlock / the
towers, against the independent fp64 reference of openvla_ref.py (computed once per case on the CPU).

Yardstick: the same bf16 model on the same GPU with VAA_NO_FUSED_MODEL_OPS, VAA_NO_FUSED_ATTENTION and VAA_NO_TN_DGRAD set — the eager chain.
Bounds, per observable (labelled-row logits, full forward() logits on real tokens, pixel gradient, patch-embed gradients of sum(rows * C)):

    rel rms error (form)  <=  RMS_FACTOR x rel rms error (eager)        RMS_FACTOR = 2, the factor of test_gpu_attention_ref.py: two correct
                                                                       bf16 evaluations that differ in summation order and fusion differ
                                                                       by an O(1) factor in rms error
    1 - cos (form)        <=  RMS_FACTOR^2 x (1 - cos (eager))         gradients. The same slack: an error of relative size e, nearly orthogonal
                                                                       to the gradient (cos > 0.999 here), costs e^2 / 2 of cosine, so a
                                                                       factor 2 on e is a factor 4 on 1 - cos
    rel max error (form)  <=  MAX_FACTOR x rel max error (eager)       MAX_FACTOR = 3: the maximum of N error samples is an extreme-value
                                                                       statistic, noisier than their rms; measured worst ratio x its margin
                                                                       in DESIGN.md

Every form also asserts, by counting the autograd Functions (and the SDPA / side-stream calls) it went through, that it took the branch it is
named for: a form that silently fell back to the eager branch would meet every bound.
"""
import contextlib
import functools

import pytest
import torch

pytest.importorskip("transformers")

import openvla_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RMS_FACTOR = 2.0
MAX_FACTOR = 3.0
EAGER = dict(VAA_NO_FUSED_MODEL_OPS="1", VAA_NO_FUSED_ATTENTION="1", VAA_NO_TN_DGRAD="1")
SWITCHES = ("VAA_NO_FUSED_MODEL_OPS", "VAA_NO_FUSED_ATTENTION", "VAA_NO_TN_DGRAD", "VAA_FUSED_QKV", "VAA_SEQ_PACK", "VAA_TOWER_STREAMS", "VAA_SEQ_FLOOR",
            "VAA_MODEL_SCALE_ADD", "VAA_DIST_BACKEND")
FORMS = {  # name -> environment
    "default": {},
    "qkv_split": dict(VAA_FUSED_QKV="0"),
    "no_tn_dgrad": dict(VAA_NO_TN_DGRAD="1"),
    "no_fused_attention": dict(VAA_NO_FUSED_ATTENTION="1"),
    "seq_pack": dict(VAA_SEQ_PACK="1"),
    "one_stream": dict(VAA_TOWER_STREAMS="0"),
}
FNS = ("RopeFn", "SwiGLUFn", "ScaleAddFn", "ResidualRMSNormFn", "ResidualLayerNormFn", "FrozenLinearsFn", "AttentionFn", "RopeAttentionFn",
       "RopePackedAttentionFn", "PackedAttentionFn")


@contextlib.contextmanager
def _env(**kw):
    """The model's switches are read at call time: exactly `kw` of them set, the others unset."""
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in kw.items():
            mp.setenv(k, v)
        yield


@contextlib.contextmanager
def _count():
    """Calls of every model_ops Function, of SDPA and of the side stream, and whether an attention Function was given cu_seqlens."""
    from roboticattack_amd import model_ops

    n = dict.fromkeys(FNS + ("sdpa", "side_stream", "packed_calls"), 0)
    with pytest.MonkeyPatch.context() as mp:
        for name in FNS:
            cls = getattr(model_ops, name)

            def apply(*a, _orig=cls.apply, _name=name):
                n[_name] += 1
                if _name in ("RopeAttentionFn", "RopePackedAttentionFn") and any(isinstance(x, torch.Tensor) and x.dtype == torch.int32 for x in a):
                    n["packed_calls"] += 1
                return _orig(*a)

            mp.setattr(cls, "apply", apply)

        def sdpa(*a, _orig=torch.nn.functional.scaled_dot_product_attention, **kw):
            n["sdpa"] += 1
            return _orig(*a, **kw)

        def stream(*a, _orig=torch.cuda.stream, **kw):
            n["side_stream"] += 1
            return _orig(*a, **kw)

        mp.setattr(torch.nn.functional, "scaled_dot_product_attention", sdpa)
        mp.setattr(torch.cuda, "stream", stream)
        yield n


def _expected(cfg, form, packed):
    """The Function counts of one forward through the form that `form` names."""
    n, hd = cfg.llm_layers, cfg.llm_dim // cfg.llm_heads
    vit = cfg.dino.depth - 1 + cfg.siglip.depth - 1
    ls = (cfg.dino.depth - 1) * (2 if cfg.dino.layerscale else 0)
    e = dict.fromkeys(FNS + ("sdpa", "side_stream", "packed_calls"), 0)
    if form == "eager":  # (the three switches of the yardstick leave the towers on their two streams)
        e.update(sdpa=n + vit, side_stream=1)
        return e
    e.update(SwiGLUFn=n, ScaleAddFn=ls, ResidualRMSNormFn=2 * n, ResidualLayerNormFn=2 * vit, side_stream=0 if form == "one_stream" else 1)
    e["FrozenLinearsFn"] = 0 if form == "no_tn_dgrad" else 4 * n  # q/k/v (one call), o_proj + residual, gate/up, down_proj + residual
    if form == "no_fused_attention":
        e.update(RopeFn=2 * n, sdpa=n + vit)
        return e
    e["PackedAttentionFn"] = vit
    if hd not in (64, 128):
        e.update(RopeFn=2 * n, AttentionFn=n)
    elif form in ("qkv_split", "no_tn_dgrad"):
        e["RopeAttentionFn"] = n
    else:
        e["RopePackedAttentionFn"] = n
    e["packed_calls"] = n if packed else 0
    return e


def _embed_keys(meas):
    """The measures of the `patch_embeds=` path under names of their own (its rows are not forward_rows' rows on pixels)."""
    return {("embed_rows" if k == "rows" else k): v for k, v in meas.items()}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Per case, once: batch, fp64 reference observables (CPU), the bf16 model on the GPU and the eager chain's errors."""
    m = R.build_model(name)
    batch = R.make_batch(name)
    ref = R.build_reference(m)
    full = name == R.FULL_CASE
    obs = ref.observables(batch, full=full)
    obs_e = ref.observables(batch, embeds=True) if full else None
    model = m.to(torch.bfloat16).to(DEV)
    with _env(**EAGER):
        with _count() as n:
            got = R.model_observables(model, batch)
            calls = dict(n)
        eager = R.measure(got, obs)
        if full:
            eager["full"] = R.measure(R.model_observables(model, batch, full=True), obs)["full"]
            eager.update(_embed_keys(R.measure(R.model_observables(model, batch, embeds=True), obs_e)))
    c = dict(name=name, batch=batch, obs=obs, obs_e=obs_e, model=model, eager=eager, eager_calls=calls, full=full)
    for k, e in eager.items():
        print("OPENVLA_REF %s eager %s rms %.4e max %.4e cos %.8f" % (name, k, e["rms"], e["max"], e["cos"]))
    return c


@pytest.fixture(params=list(R.CASES))
def case(request):
    return _case(request.param)


def _assert_bounds(c, form, meas):
    bad = []
    for k, e in meas.items():
        y = c["eager"][k]
        print("OPENVLA_REF %s %s %s rms %.4e max %.4e cos %.8f ratio_rms %.3f ratio_max %.3f ratio_1mcos %.3f"
              % (c["name"], form, k, e["rms"], e["max"], e["cos"], e["rms"] / y["rms"], e["max"] / y["max"], (1 - e["cos"]) / (1 - y["cos"])))
        if not e["rms"] <= RMS_FACTOR * y["rms"]:
            bad.append("%s rel rms %.3e > %g x eager %.3e" % (k, e["rms"], RMS_FACTOR, y["rms"]))
        if not e["max"] <= MAX_FACTOR * y["max"]:
            bad.append("%s rel max %.3e > %g x eager %.3e" % (k, e["max"], MAX_FACTOR, y["max"]))
        if "grad" in k and not 1 - e["cos"] <= RMS_FACTOR ** 2 * (1 - y["cos"]):
            bad.append("%s cos %.8f < eager %.8f less the slack" % (k, e["cos"], y["cos"]))
    assert not bad, "%s %s: %s" % (c["name"], form, "; ".join(bad))


def test_eager_yardstick(case):
    """The yardstick took the eager branches only, and meets the yardstick condition on this GPU as well (rel rms < 0.1, cosine > 0.99)."""
    assert case["eager_calls"] == _expected(case["model"].cfg, "eager", False), case["eager_calls"]
    e = case["eager"]
    assert e["rows"]["rms"] < 0.1 and e["pixel_grad"]["rms"] < 0.1 and e["pixel_grad"]["cos"] > 0.99
    assert e["rows"]["rms"] > 1e-4  # bf16 error is visible: the ratios below divide by it


@pytest.mark.parametrize("form", list(FORMS))
def test_form_vs_fp64(case, form):
    """Labelled-row logits and pixel gradient of every dispatch form within the bounds, through the branch the form is named for."""
    model, batch = case["model"], case["batch"]
    hd = model.cfg.llm_dim // model.cfg.llm_heads
    with _env(**FORMS[form]), _count() as n:
        pack = None
        if form == "seq_pack":
            mask = batch["attention_mask"].to(DEV)
            pack = model.make_pack(mask)
            assert pack is not None and pack.total == int(mask.sum()) + mask.shape[0] * 256
            assert len(pack.lens) == mask.shape[0] + 1 and pack.total % 256 and (pack.total + pack.lens[-1]) % 256 == 0  # the fill sequence exists
        got = R.model_observables(model, batch, pack=pack)
        calls = dict(n)
    assert calls == _expected(model.cfg, form, pack is not None and hd in (64, 128)), calls
    _assert_bounds(case, form, R.measure(got, case["obs"]))


def test_patch_embeds_path_vs_fp64():
    """The `patch_embeds=` path (default form): rows and the gradient with respect to both patch-embed inputs."""
    c = _case(R.FULL_CASE)
    with _env(), _count() as n:
        got = R.model_observables(c["model"], c["batch"], embeds=True)
        calls = dict(n)
    assert calls == _expected(c["model"].cfg, "default", False), calls
    _assert_bounds(c, "patch_embeds", _embed_keys(R.measure(got, c["obs_e"])))


def test_full_forward_vs_fp64():
    """forward(): the full logits on every real token (default form; all positions go through the last layer)."""
    c = _case(R.FULL_CASE)
    with _env(), _count() as n:
        got = R.model_observables(c["model"], c["batch"], full=True)
        calls = dict(n)
    exp = _expected(c["model"].cfg, "default", False)
    assert calls == {k: 2 * v for k, v in exp.items()}, calls  # forward_rows + forward()
    _assert_bounds(c, "full_forward", dict(full=R.measure(got, c["obs"])["full"]))
