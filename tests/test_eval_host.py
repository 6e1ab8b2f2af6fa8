"""CPU-only: the two references of the evaluation front end against each other, the exact cases of the contract, the metric arithmetic of
attack/evaluate.py and the argument rules of vaa_eval_preprocess."""
import ctypes

import numpy as np
import pytest
import torch

import eval_ref
from roboticattack_amd import _lib
from roboticattack_amd.action_tokenizer import ActionTokenizer
from roboticattack_amd.attack.evaluate import summarise

# (a) the share of bytes on which crop_u8_f32 and crop_u8_f64 differ (always by exactly one level), measured on the CPU for exactly the inputs
# of the test below (numpy 2.2.6): worst case 810 of 451,584 bytes = 1.794e-3 (checkerboard at crop_scale 0.5; noise at 0.5: 1.588e-3; every
# other case below 5.1e-4; 0 for crop_scale 1.0 and for constant frames). The cap is 4x the worst measured share.
WORST_MEASURED_SHARE = 810 / 451584
SHARE_CAP = 4 * WORST_MEASURED_SHARE


@pytest.mark.parametrize("kind", eval_ref.KINDS)
def test_fp32_restatement_against_fp64(kind):
    """The fp32 restatement never leaves the fp64 result by more than one level, and does so on at most SHARE_CAP = 7.17e-3 of the bytes
    (4x the worst measured share, 1.794e-3: truncation at exact level boundaries; the margin covers numpy-version rounding of sqrt only)."""
    fr = eval_ref.frames(kind)
    for scale in eval_ref.SCALES:
        d = np.abs(eval_ref.crop_u8_f32(fr, scale).astype(np.int32) - eval_ref.crop_u8_f64(fr, scale).astype(np.int32))
        share = float((d == 1).mean())
        print("%s crop_scale %.2f: max |difference| %d, share of one-level differences %.3e" % (kind, scale, d.max(), share))
        assert d.max() <= 1
        assert share <= SHARE_CAP


def test_full_frame_crop_is_the_identity_and_constants_stay_constant():
    """(b) crop_scale = 1.0 returns the input bytes exactly — all 256 levels in every channel; a constant frame stays constant at every scale."""
    levels = (np.arange(224 * 224 * 3, dtype=np.int64) % 256).astype(np.uint8).reshape(1, 224, 224, 3)
    assert set(np.unique(levels[..., 0])) == set(range(256))
    for fn in (eval_ref.crop_u8_f32, eval_ref.crop_u8_f64):
        assert np.array_equal(fn(levels, 1.0), levels)
        for kind in ("noise", "checker"):
            fr = eval_ref.frames(kind)
            assert np.array_equal(fn(fr, 1.0), fr)
            assert np.array_equal(fn(fr, 0), fr)  # 0 = no crop
    for level in range(256):
        const = np.full((1, 224, 224, 3), level, np.uint8)
        for scale in eval_ref.SCALES:
            assert np.array_equal(eval_ref.crop_u8_f32(const, scale), const), (level, scale)
    const = eval_ref.frames("constant")
    for scale in eval_ref.SCALES:
        assert np.array_equal(eval_ref.crop_u8_f64(const, scale), const)


def test_crop_takes_the_centre():
    """A frame that is black outside its central 112-pixel box: at 0.25 of the area the crop is that box, so away from the rim (where the
    half-pixel taps still blend in the black border) nothing black survives."""
    fr = np.zeros((1, 224, 224, 3), np.uint8)
    fr[:, 56:168, 56:168] = 200
    out = eval_ref.crop_u8_f32(fr, 0.25)
    assert (out[:, 2:-2, 2:-2] == 200).all() and out[0, 0, 0, 0] < 200


# ---------------------------------------------------------------- (c) summarise ----------------------------------------------------------------
def _tokens(rs, shape):
    return torch.from_numpy(rs.randint(31744, 32000, size=shape))


def test_summarise_identical_tokens_give_zero():
    clean = _tokens(np.random.RandomState(0), (4, 7))
    out = summarise(clean, clean[None].repeat(3, 1, 1))
    assert len(out["per_placement"]) == 3
    for r in out["per_placement"] + [out["overall"]]:
        assert torch.equal(r["token_flip_rate"], torch.zeros(7, dtype=torch.float64)) and torch.equal(r["nad"], torch.zeros(7, dtype=torch.float64))
        assert r["any_flip_rate"] == 0.0 and "l1_unnorm" not in r and "target_hit_rate" not in r


def test_summarise_one_changed_dof_in_one_of_four_frames():
    at = ActionTokenizer()
    clean = _tokens(np.random.RandomState(1), (4, 7))
    patched = clean[None].repeat(2, 1, 1).clone()
    patched[1, 2, 3] = 31744 if int(clean[2, 3]) != 31744 else 31800
    out = summarise(clean, patched)
    zero = torch.zeros(7, dtype=torch.float64)
    assert torch.equal(out["per_placement"][0]["token_flip_rate"], zero) and out["per_placement"][0]["any_flip_rate"] == 0.0
    r = out["per_placement"][1]
    want = zero.clone()
    want[3] = 0.25
    assert torch.equal(r["token_flip_rate"], want) and r["any_flip_rate"] == 0.25
    a_c, a_p = at.decode_token_ids_to_actions(np.array([int(clean[2, 3])])), at.decode_token_ids_to_actions(np.array([int(patched[1, 2, 3])]))
    nad = zero.clone()
    nad[3] = float(abs(a_p[0] - a_c[0])) / 4 / 2  # mean over the four frames, half the distance on [-1, 1]
    assert torch.allclose(r["nad"], nad, rtol=0, atol=1e-15) and float(r["nad"][3]) > 0
    o = out["overall"]  # 8 rows, one changed
    assert float(o["token_flip_rate"][3]) == 0.125 and o["any_flip_rate"] == 0.125 and float(o["token_flip_rate"].sum()) == 0.125


def test_summarise_target_hit_rate_uses_the_action_tokenizer():
    at = ActionTokenizer()
    target_action = np.array([0.5, -0.25, 0.0, 1.0, -1.0, 0.1, 0.9])
    maskidx = [1, 4]
    tok = at.action_to_token_ids(target_action)
    clean = _tokens(np.random.RandomState(2), (4, 7))
    clean[:, 1] = 31750  # away from the target tokens
    clean[:, 4] = 31751
    assert int(tok[1]) != 31750 and int(tok[4]) != 31751
    patched = clean[None].repeat(2, 1, 1).clone()
    patched[0, 0, 1] = int(tok[1])
    patched[0, 3, 1] = int(tok[1])
    patched[1, :, 4] = int(tok[4])
    patched[1, 1, 0] = int(tok[0])  # DoF 0 is not in maskidx: must not count
    for target in ((maskidx, target_action), (maskidx, target_action[maskidx])):  # a whole action vector, or one value per maskidx entry
        out = summarise(clean, patched, target=target)
        assert out["per_placement"][0]["target_hit_rate"].tolist() == [0.5, 0.0]
        assert out["per_placement"][1]["target_hit_rate"].tolist() == [0.0, 1.0]
        assert out["overall"]["target_hit_rate"].tolist() == [0.25, 0.5]
    assert summarise(clean, patched, target=([4], -1.0))["per_placement"][1]["target_hit_rate"].tolist() == [1.0]  # a scalar


def test_summarise_l1_unnorm_honours_the_mask():
    at = ActionTokenizer()
    clean = _tokens(np.random.RandomState(3), (4, 7))
    patched = _tokens(np.random.RandomState(4), (1, 4, 7))
    stats = dict(q01=np.linspace(-2, -1, 7).tolist(), q99=np.linspace(0.5, 3, 7).tolist(), mask=[True, True, False, True, True, True, False])
    r = summarise(clean, patched, unnorm_stats=stats)["per_placement"][0]
    d = np.abs(at.decode_token_ids_to_actions(patched[0].numpy()) - at.decode_token_ids_to_actions(clean.numpy())).mean(0)
    span = np.array(stats["q99"]) - np.array(stats["q01"])
    want = np.where(np.array(stats["mask"]), 0.5 * span * d, d)  # masked-out dimensions stay on the bin centres
    assert np.allclose(r["l1_unnorm"].numpy(), want, rtol=1e-12, atol=0)
    assert np.allclose(r["nad"].numpy(), d / 2, rtol=1e-12, atol=0)
    no_mask = summarise(clean, patched, unnorm_stats=dict(q01=stats["q01"], q99=stats["q99"]))["per_placement"][0]
    assert np.allclose(no_mask["l1_unnorm"].numpy(), 0.5 * span * d, rtol=1e-12, atol=0)


def test_summarise_refuses_mismatched_shapes():
    with pytest.raises(ValueError):
        summarise(torch.zeros(4, 7, dtype=torch.int64), torch.zeros(2, 3, 7, dtype=torch.int64))


# ---------------------------------------------------------------- (d) argument rules ----------------------------------------------------------------
def _call(B=1, crop_scale=0.9, null=None):
    """The entry point on host buffers: every case below returns before a launch."""
    L = _lib.lib()
    bufs = dict(img=ctypes.create_string_buffer(64), out=ctypes.create_string_buffer(64))
    args = dict(img=ctypes.cast(bufs["img"], ctypes.c_void_p), mean=_lib.f32x([0.5] * 6), std=_lib.f32x([0.25] * 6),
                out=ctypes.cast(bufs["out"], ctypes.c_void_p))
    if null:
        args[null] = None
    return L.vaa_eval_preprocess(args["img"], B, crop_scale, args["mean"], args["std"], args["out"], None)


def test_library_exports_the_entry_point():
    assert "vaa_eval_preprocess" in _lib.EXPORTS and hasattr(_lib.lib(), "vaa_eval_preprocess")


def test_argument_rules_without_gpu():
    L = _lib.lib()
    for name in ("img", "mean", "std", "out"):
        assert _call(null=name) == -1 and b"null pointer" in L.vaa_last_error()
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert _call(crop_scale=bad) == -1 and b"crop_scale" in L.vaa_last_error()
        assert _call(B=0, crop_scale=bad) == -1
    assert _call(B=-1) == -1
    assert _call(B=0) == 0 and _call(B=0, crop_scale=0.0) == 0 and _call(B=0, crop_scale=1.0) == 0
    assert L.vaa_eval_preprocess(None, 0, 0.9, None, None, None, None) == 0  # an empty batch reads no pointer
