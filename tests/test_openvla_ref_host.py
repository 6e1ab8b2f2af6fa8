"""The DEFINITION of the OpenVLA model path, on the CPU: `OpenVLAShaped(cfg).double()` (the plain branches) against the independent fp64
reference of openvla_ref.py (Hugging Face Llama / DINOv2-with-registers / SigLIP classes built from configs, loaded with the same weights).

HOST_TOL: the worst relative error (rms or max) measured over every case and observable below is 6.8e-7 (pixel gradient, relative max, case
hd80; forward rows 1.7e-7): HF builds its rotary tables in fp32 even in a double model, and so does the model. The bound is 8 x that, the
margin of the jitter tests. It stays far below 1e-3: a tanh-for-erf GELU in the projector moves the rows by 0.8-1.2e-4 at these weights
(measured with that mutant), 14-21 x the bound.
"""
import copy
import functools

import pytest
import torch

pytest.importorskip("transformers")

import openvla_ref as R  # noqa: E402

HOST_TOL = 5.5e-6   # 8 x 6.8e-7 (module docstring)
EXACT = 1e-12       # the fp64 model against itself along another path: summation order only
FP32 = 2.0 ** -23   # forward() returns fp32 logits by contract: one rounding, 2^-24 relative per element


@functools.lru_cache(maxsize=None)
def _build(name):
    """Per case, once: the model (bf16-representable weights, fp32 storage), its .double(), the batch, the reference and its observables."""
    m = R.build_model(name)
    batch = R.make_batch(name)
    ref = R.build_reference(m)
    return dict(name=name, model=m, f64=copy.deepcopy(m).double(), batch=batch, ref=ref, obs=ref.observables(batch, full=True))


@pytest.fixture(params=list(R.CASES))
def case(request):
    return _build(request.param)


def _check(meas, tol, what):
    for obs, e in meas.items():
        print("%s %-11s rel rms %.3e  rel max %.3e" % (what, obs, e["rms"], e["max"]))
    for obs, e in meas.items():
        assert e["rms"] <= tol and e["max"] <= tol, (what, obs, e)


def test_case_table_is_what_the_branches_need():
    hd = {n: c[0].llm_dim // c[0].llm_heads for n, c in R.CASES.items()}
    assert hd == {"hd128": 128, "hd64_clspos": 64, "hd80": 80}
    c = R.CASES["hd128"][0]
    assert (c.dino.dim // c.dino.heads, c.siglip.dim // c.siglip.heads) == (64, 72)
    assert R.CASES["hd64_clspos"][0].dino.cls_pos and not R.CASES["hd128"][0].dino.cls_pos
    for cfg, lens, _ in R.CASES.values():
        assert len(set(lens)) == len(lens) and (cfg.seq_floor, cfg.seq_multiple) == (44, 4)  # padding exists; the 7B bucket
    assert min(R.CASES["hd128"][1]) < 44 and max(R.CASES["hd80"][1]) > 44  # below the floor / above it (the multiple decides)


def test_attention_logit_spread(case):
    """init_sensitive: the pre-softmax logits of every ViT block and Llama layer have a standard deviation between 1 and 2."""
    std = R.attention_logit_std(case["model"], case["batch"])
    print(case["name"], {k: round(v, 2) for k, v in std.items()})
    cfg = case["model"].cfg
    assert len(std) == cfg.dino.depth - 1 + cfg.siglip.depth - 1 + cfg.llm_layers
    assert all(1.0 <= v <= 2.0 for v in std.values()), std


def test_random_parts_are_not_trivial(case):
    for name, p in case["model"].named_parameters():
        assert float(p.std()) > 0.01, name  # no constant gains, zero biases, unit LayerScale or zero position / prefix tokens left


def test_fp64_model_matches_reference(case):
    """Forward rows, full logits on the real tokens and the pixel gradient of sum(rows * C)."""
    got = R.model_observables(case["f64"], case["batch"], full=True)
    _check(R.measure(got, case["obs"]), HOST_TOL, case["name"])


def test_rows_only_path_is_the_full_path(case):
    """forward_rows (last layer on the labelled rows only, prompts padded to the bucket) against the labelled rows of forward(): both within
    HOST_TOL of the reference, and of each other to forward()'s fp32 rounding of its logits."""
    a = R.model_observables(case["f64"], case["batch"])
    b = R.model_observables(case["f64"], case["batch"], rows_from_full=True)
    _check(R.measure(b, case["obs"]), HOST_TOL, case["name"] + " via forward()")
    _check(R.measure(a, dict(rows=b["rows"], grad=b["grad"])), FP32, case["name"] + " rows-only vs forward()")


def test_bucketed_padding_changes_nothing(case, monkeypatch):
    """The same rows with the seq_floor / seq_multiple bucket on and off."""
    m, batch = case["f64"], case["batch"]
    L = batch["input_ids"].shape[1]
    assert m.seq_bucket(L) > L
    on = R.model_observables(m, batch)
    monkeypatch.setenv("VAA_SEQ_FLOOR", "0")
    assert m.seq_bucket(L) == L
    off = R.model_observables(m, batch)
    _check(R.measure(off, case["obs"]), HOST_TOL, case["name"] + " bucket off")
    _check(R.measure(on, dict(rows=off["rows"], grad=off["grad"])), EXACT, case["name"] + " bucket on vs off")


def test_patch_embeds_path_matches_reference():
    """The `patch_embeds=` path: rows and the gradient with respect to the two patch-embed inputs."""
    case = _build(R.FULL_CASE)
    ref = case["ref"].observables(case["batch"], embeds=True)
    got = R.model_observables(case["f64"], case["batch"], embeds=True)
    _check(R.measure(got, ref), HOST_TOL, case["name"] + " patch_embeds")


def test_bf16_eager_is_a_usable_yardstick(case):
    """The yardstick condition of test_gpu_openvla_ref.py (not a tolerance on the kernels): the same model in bf16 eager stays within a
    relative rms error of 0.1 of the reference on rows and pixel gradient, gradient cosine above 0.99 — the weights are sensitive, not chaotic."""
    mb = copy.deepcopy(case["model"]).to(torch.bfloat16)
    meas = R.measure(R.model_observables(mb, case["batch"]), case["obs"])
    for obs, e in meas.items():
        print("%s bf16 eager %-11s rel rms %.3e  rel max %.3e  cos %.6f" % (case["name"], obs, e["rms"], e["max"], e["cos"]))
    assert meas["rows"]["rms"] < 0.1 and meas["pixel_grad"]["rms"] < 0.1 and meas["pixel_grad"]["cos"] > 0.99
    assert meas["rows"]["rms"] > 100 * HOST_TOL  # and bf16 is visible at all: the comparison is not vacuous
