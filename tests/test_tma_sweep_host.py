"""CPU tests of the TMA target sweep's host side: CLI parsing, group tags, per-group target labels, every refusal, the untouched maskidx
sweep / no-sweep attacker, and the argument checks of the new C-ABI entry points (no kernel is launched)."""
import pytest
import torch

from roboticattack_amd import _lib, synthetic
from roboticattack_amd.attack import uada_ddp
from sweep_harness import attacker, fused, wrapper


def test_cli_parses_the_target_sweep():
    w = wrapper("uada_wrapper_ddp_target_sweep")
    a = w.arg_parser(["--attack", "TMA", "--target_sweep", "0:0;1:0;6:1"])
    assert a.target_sweep == [([0], 0.0), ([1], 0.0), ([6], 1.0)] and a.attack == "TMA"
    assert w.arg_parser(["--target_sweep", "0,1,2:0.25;0,1,2,3,4,5,6:-0.5"]).target_sweep == [([0, 1, 2], 0.25), ([0, 1, 2, 3, 4, 5, 6], -0.5)]
    assert w.arg_parser([]).target_sweep is None and w.arg_parser([]).maskidx_sweep is None  # default: no sweep, today's loop
    assert uada_ddp.parse_target_sweep("") is None and uada_ddp.parse_target_sweep(None) is None
    for bad in ("0", "0:", "0;1:0"):
        with pytest.raises(ValueError, match="maskidx\\[,maskidx...\\]:target"):
            uada_ddp.parse_target_sweep(bad)


def test_group_tags_are_equal_for_equal_groups_and_distinct_otherwise():
    tag = uada_ddp.target_sweep_tag
    assert tag([0], 0.25) == "maskidx0-target0.25" and tag([0, 1, 2], 0) == "maskidx0-1-2-target0"
    assert tag([0], 0) == tag([0], 0.0) == tag((0,), -0.0 + 0.0)
    groups = [([0], 0.0), ([0], 0.25), ([1], 0.0), ([0, 1], 0.0), ([0], -0.25), ([0], 1.0), ([0], 0.1), ([0], 0.125)]
    assert len({tag(m, t) for m, t in groups}) == len(groups)
    assert all(tag(m, t).startswith(uada_ddp.sweep_tag(m) + "-target") for m, t in groups)


def test_target_sweep_refusals_name_their_limit(monkeypatch, tmp_path):
    fused(monkeypatch)
    ok = attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([0], 0), ((0, 1, 2), 0.25)])
    assert ok.target_sweep == [([0], 0.0), ([0, 1, 2], 0.25)] and ok.maskidx_sweep is None
    with pytest.raises(ValueError, match="at least one group"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[])
    with pytest.raises(ValueError, match="at least one maskidx"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([], 0.0)])
    with pytest.raises(ValueError, match="distinct"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([0], 0.0), ([0], 0)])
    attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([0], 0.0), ([0], 0.5)])  # same maskidx, another target: two groups
    with pytest.raises(ValueError, match="0..6"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([7], 0.0)])
    with pytest.raises(ValueError, match="0..6"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([1, 1], 0.0)])
    for other in ("UADA", "UPA"):
        with pytest.raises(ValueError, match="TMA only"):
            attacker(monkeypatch, tmp_path, attack_type=other, target_sweep=[([0], 0.0)])
    with pytest.raises(ValueError, match="resize_patch"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", resize_patch=True, target_sweep=[([0], 0.0)])
    with pytest.raises(ValueError, match="fused path"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", model="plain", target_sweep=[([0], 0.0)])
    with pytest.raises(ValueError, match="limit of 512"):  # 6 x 100 images
        attacker(monkeypatch, tmp_path, attack_type="TMA", bs=100, target_sweep=[([q], 0.0) for q in range(6)])
    attacker(monkeypatch, tmp_path, attack_type="TMA", bs=63, target_sweep=[([0, 1, 2, 3, 4, 5, 6], 0.1 * q) for q in range(8)])  # 504 images, 3528 rows: no row limit behind the GEMM head
    with pytest.raises(ValueError, match="maskidx_sweep"):
        attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=[([0], 0.0)], maskidx_sweep=[[0]])
    with pytest.raises(ValueError, match="maskidx_sweep"):  # also when the maskidx sweep itself would be accepted
        attacker(monkeypatch, tmp_path, attack_type="UADA", target_sweep=[([0], 0.0)], maskidx_sweep=[[0]])


def test_maskidx_sweep_and_plain_attacker_are_untouched(monkeypatch, tmp_path):
    fused(monkeypatch)
    for other in ("TMA", "UPA"):
        with pytest.raises(ValueError, match="UADA only"):
            attacker(monkeypatch, tmp_path, attack_type=other, maskidx_sweep=[[0]])
    plain = attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=None, maskidx=[0, 1], target_action=0.25)
    assert plain.target_sweep is None and plain.maskidx_sweep is None and plain.maskidx == [0, 1] and plain.target_action == 0.25
    assert not hasattr(plain, "sweep_tags")
    uada = attacker(monkeypatch, tmp_path, maskidx_sweep=[[0], [0, 1, 2]])
    assert uada.maskidx_sweep == [[0], [0, 1, 2]] and uada.target_sweep is None


def test_group_labels_are_the_standalone_target_labels(monkeypatch, tmp_path):
    from roboticattack_amd.labels import tma_target_labels, tma_target_tokens

    fused(monkeypatch)
    sweep = [([0], 0.0), ([0, 1, 2], 0.25), ([0, 1, 2, 3, 4, 5, 6], -0.5)]
    att = attacker(monkeypatch, tmp_path, attack_type="TMA", target_sweep=sweep)
    att._tma_targets = [tma_target_tokens(float(t) * torch.ones(7).numpy(), m, att.action_tokenizer) for m, t in sweep]
    _, labels, _ = synthetic.synth_text_batch(3, 4)
    keep = labels.clone()
    for g, (m, t) in enumerate(sweep):
        got = att._sweep_group_labels(labels, g)
        solo = attacker(monkeypatch, tmp_path, attack_type="TMA", maskidx=m, target_action=t)
        solo._tma_target = tma_target_tokens(float(t) * torch.ones(7).numpy(), m, solo.action_tokenizer)
        assert torch.equal(got, solo._prepare_labels(labels)) and torch.equal(got, tma_target_labels(labels, att._tma_targets[g]))
        assert int((got[:, 1:] != -100).sum()) == 4 * len(m)  # the target vector labels the maskidx DoFs only (EOS is position 7: never in 0..6)
    assert torch.equal(labels, keep)  # the loader's labels are not touched


def test_new_entry_points_check_their_arguments_without_gpu():
    L = _lib.lib()
    par = _lib.f32x([5, .8, .2, 1])
    # not P equal groups / P out of range
    assert L.vaa_loss_rows_fwd_bwd_seg(None, 1, None, 8, 12, 30, 32064, 5, _lib.LOSS_CE, par, None, None, None, None, 0, None, 0, None) == -1
    assert b"P groups of equal size" in L.vaa_last_error()
    assert L.vaa_loss_rows_fwd_bwd_seg(None, 1, None, 8, 12, 30, 32064, 0, _lib.LOSS_CE, par, None, None, None, None, 0, None, 0, None) == -1
    # only the cross-entropy mode with full-row gradients
    for mode, kind in ((_lib.LOSS_UADA_DDP, _lib.GRAD_FULL), (_lib.LOSS_UADA, _lib.GRAD_FULL), (_lib.LOSS_UPA, _lib.GRAD_FULL), (_lib.LOSS_CE, _lib.GRAD_SLICE)):
        assert L.vaa_loss_rows_fwd_bwd_seg(None, 1, None, 8, 12, 30, 32064, 3, mode, par, None, None, None, None, kind, None, 0, None) != 0
        assert b"VAA_LOSS_CE with full-row gradients only" in L.vaa_last_error()
    assert L.vaa_loss_rows_fwd_bwd_seg(None, 1, None, 8, 12, 30, 32064, 3, _lib.LOSS_CE, par, None, None, None, None, 0, None, 0, None) == -1
    assert b"null pointer" in L.vaa_last_error()
    assert L.vaa_step_epilogue_seg_tail(None, 1, 7500, 3, None, None, None) == -1
    assert L.vaa_step_epilogue_seg_tail_update(None, 1, 7500, 3, None, None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-6, 1, None, None) == -1
