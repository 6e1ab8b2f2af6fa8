"""CPU tests of the maskidx sweep's host side: CLI parsing, group tags, per-group label masking, the refusals, the C-ABI size rule of the
segmented row map and the RNG consumption of one sweep step (one draw per frame, shared by every group)."""
import random

import numpy as np
import pytest
import torch

from roboticattack_amd import _lib, synthetic
from roboticattack_amd.attack import sweep, uada_ddp
from sweep_harness import attacker, fused, wrapper


def test_cli_parses_the_sweep():
    w = wrapper("uada_wrapper_ddp_sweep")
    assert w.arg_parser(["--maskidx_sweep", "0;0,1,2"]).maskidx_sweep == [[0], [0, 1, 2]]
    assert w.arg_parser(["--maskidx_sweep", "0;0,1,2,3,4,5,6"]).maskidx_sweep == [[0], [0, 1, 2, 3, 4, 5, 6]]
    assert w.arg_parser([]).maskidx_sweep is None  # default: no sweep, today's loop
    assert uada_ddp.parse_maskidx_sweep("") is None and uada_ddp.parse_maskidx_sweep(None) is None


def test_group_tags():
    assert uada_ddp.sweep_tag([0]) == "maskidx0" and uada_ddp.sweep_tag([0, 1, 2]) == "maskidx0-1-2"
    assert uada_ddp.sweep_rows(8, [[0], [0, 1, 2]]) == 8 * 2 + 8 * 4


def test_labels_are_masked_per_group():
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(3, 4)
    sweep = [[0], [0, 1, 2], [0, 1, 2, 3, 4, 5, 6]]
    out = uada_ddp.mask_labels_sweep(labels, sweep)
    assert out.shape == (12, labels.shape[1])
    for g, m in enumerate(sweep):
        assert torch.equal(out[4 * g : 4 * g + 4], mask_labels(labels.clone(), m))
        assert int((out[4 * g : 4 * g + 4, 1:] != -100).sum()) == 4 * (len(m) + 1)
    assert torch.equal(labels, synthetic.synth_text_batch(3, 4)[1])  # the loader's labels are not touched


def test_refusals_name_their_limit(monkeypatch, tmp_path):
    fused(monkeypatch)
    ok = attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0, 1, 2]])
    assert ok.maskidx_sweep == [[0], [0, 1, 2]]
    assert attacker(monkeypatch, tmp_path).maskidx_sweep is None  # no sweep requested: the attacker is today's
    with pytest.raises(ValueError, match="UADA only"):
        attacker(monkeypatch, tmp_path, attack_type="UPA", maskidx_sweep=[[0]])
    with pytest.raises(ValueError, match="UADA only"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", maskidx_sweep=[[0]])
    with pytest.raises(ValueError, match="resize_patch"):
        attacker(monkeypatch, tmp_path, resize_patch=True, maskidx_sweep=[[0]])
    with pytest.raises(ValueError, match="fused path"):
        attacker(monkeypatch, tmp_path, model="plain", maskidx_sweep=[[0]])
    with pytest.raises(ValueError, match="limit of 128"):  # 2 x 20 x 8 = 320 labelled rows
        attacker(monkeypatch, tmp_path, bs=20, maskidx_sweep=[[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5]])
    with pytest.raises(ValueError, match="144 labelled rows"):  # 16 x 4 + 16 x 5
        attacker(monkeypatch, tmp_path, bs=16, maskidx_sweep=[[0, 1, 2], [0, 1, 2, 3]])
    attacker(monkeypatch, tmp_path, bs=16, maskidx_sweep=[[0], [0, 1, 2]])  # 32 + 64 = 96 rows: accepted
    with pytest.raises(ValueError, match="limit of 512"):  # 6 x 100 images
        attacker(monkeypatch, tmp_path, bs=100, maskidx_sweep=[[0], [1], [2], [3], [4], [5]])
    with pytest.raises(ValueError, match="distinct"):
        attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0]])
    with pytest.raises(ValueError, match="0..6"):
        attacker(monkeypatch, tmp_path, maskidx_sweep=[[7]])


def test_every_kind_states_its_own_facts_once(monkeypatch, tmp_path):
    """Per kind of sweep.KINDS: its parameter alone makes it the attacker's kind, its tags read back as its groups through its own CLI form, and
    its attack type, clip and selection metric are the standalone mode's (UPA.py:157; validate(): MSE distance for UADA, else the attack loss)."""
    fused(monkeypatch)
    given = dict(maskidx_sweep=[[0], (0, 1, 2)], target_sweep=[([0], 0), ((0, 1, 2), -0.5)], upa_sweep=[(0.8, 0.2), [1, 0], (-0.25, 2e-3)])
    facts = dict(maskidx_sweep=("UADA", 0.0, 2), target_sweep=("TMA", 0.0, 0), upa_sweep=("UPA", 1e-3, 0))
    # a tag in its kind's CLI form (the fixed prefixes come off, as test_upa_sweep_host.py reads a UPA tag back)
    cli = dict(maskidx_sweep=lambda t: t[len("maskidx"):].replace("-", ","),
               target_sweep=lambda t: t[len("maskidx"):].split("-target")[0].replace("-", ",") + ":" + t.split("-target")[1],
               upa_sweep=lambda t: t[len("alpha"):].replace("-belta", ":"))
    assert [k.param for k in sweep.KINDS] == list(given) and sweep.KINDS == (sweep.MASKIDX, sweep.TARGET, sweep.UPA)
    for kind in sweep.KINDS:
        att = attacker(monkeypatch, tmp_path, attack_type=kind.attack_type, **{kind.param: given[kind.param]})
        assert att.sweep_kind is kind and att.sweep_groups == getattr(att, kind.param) == kind.normalise(given[kind.param])
        assert [getattr(att, k.param) for k in sweep.KINDS if k is not kind] == [None, None] and not hasattr(att, "sweep_tags")
        for group in att.sweep_groups:
            assert kind.parse(cli[kind.param](kind.tag(group))) == [group], (kind.param, group)
        assert (kind.attack_type, kind.l1_clip, kind.select_metric) == facts[kind.param]
    plain = attacker(monkeypatch, tmp_path)
    assert plain.sweep_kind is None and plain.sweep_groups is None


def test_segmented_rowmap_sizes_without_gpu():
    L = _lib.lib()
    B, Lt, P = 12, 30, 3
    T = 4 + 4 * B * (Lt - 1)
    assert L.vaa_loss_rowmap_seg_bytes(B, Lt, P) == 4 * (T + 4 * P + P * (4 + 4 * (B // P) * (Lt - 1)))
    assert L.vaa_loss_rowmap_seg_bytes(B, Lt, 5) == 0  # not P equal groups
    assert L.vaa_loss_rowmap_build_seg(None, B, Lt, P, None, 0, None) == -1 and b"bad arguments" in L.vaa_last_error()
    assert L.vaa_step_epilogue_seg(None, 1, 7500, 3, None, 0, 0, 0, 32064, 1, _lib.f32x([5, .8, .2, 1]), None, 0, None, None, None, None, None) == -1
    assert L.vaa_patch_update_seg(None, None, None, None, 10, 2, 0, 1e-3, 0.9, 0.999, 1e-6, 1, 0.0, 1.0, None, None) == -1


def test_sweep_draws_consume_the_rng_like_one_standalone_call(monkeypatch):
    """apply_sweep_batch over P groups of Bp frames draws once per frame (exactly a standalone apply_random_patch_batch on the Bp frames) and hands
    every group the same placement and warp."""
    from roboticattack_amd import ops
    from roboticattack_amd.transform import RandomPatchTransform

    seen = {}

    def fake(patches, img, xy, theta, *a):
        seen["xy"], seen["theta"] = xy.numpy().copy(), theta.numpy().copy()
        return torch.zeros(1), torch.zeros(1)

    monkeypatch.setattr(ops.PatchApplySweepEmbed, "apply", staticmethod(fake))
    P, Bp = 3, 4

    class Emb:
        def patch_embed_params(self):
            return (None,) * 6

    t = RandomPatchTransform("cpu")
    t.embed_with = Emb()
    frames = torch.zeros((P * Bp, 224, 224, 3), dtype=torch.uint8)
    mean, std = [[0.5] * 3, [0.5] * 3], [[0.2] * 3, [0.2] * 3]
    random.seed(42)
    np.random.seed(42)
    t.apply_sweep_batch(frames, torch.zeros(P, 3, 50, 50), mean, std, True, {})
    after = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2])
    random.seed(42)
    np.random.seed(42)
    xy, theta = RandomPatchTransform("cpu").draw_params(Bp, 50, 50, True)
    assert random.getstate() == after[0] and np.array_equal(np.random.get_state()[1], after[1]) and np.random.get_state()[2] == after[2]
    assert np.array_equal(seen["xy"], np.tile(xy, (P, 1))) and np.array_equal(seen["theta"], np.tile(theta, (P, 1)))
