"""The kinds of batched sweep of the data-parallel loop (uada_ddp.OpenVLAAttacker._attack_sweep, DESIGN.md §maskidx sweep): P patch groups
optimised in ONE loop, every group ending where the standalone run of its own parameters and the same seed ends. A kind is data plus a few short
functions; the loop, its step, the validation pass, the refusals, the CLI wrapper and tools/sweep_bench.py read the kind and never ask which one it
is. A new kind is one more SweepKind in KINDS."""
from dataclasses import dataclass
from functools import partial
from typing import Callable

import numpy as np
import torch

from .. import ops
from ..labels import mask_labels, tma_target_labels, tma_target_tokens
from ..transform import frame_stage

SWEEP_MAX_ROWS = 128    # labelled rows per rank K3s covers (vaa_head_slice_applies)
SWEEP_MAX_IMAGES = 512  # images per rank K2' keeps one partial tile each (vaa_patch_grad_partials)


# ---- CLI forms and tags ----
def _parse(text, group):
    """CLI form of a sweep: `group(part)` of every ';'-separated part; "" / None -> None (no sweep)."""
    if text is None or not str(text).strip():
        return None
    return [group(part) for part in str(text).split(";")]


def _ints(text):
    return [int(v) for v in text.split(",") if v.strip() != ""]


def _target_group(part):
    idx, sep, target = part.partition(":")
    if not sep or not target.strip():
        raise ValueError(f"target sweep: every group reads maskidx[,maskidx...]:target, got {part!r}")
    return _ints(idx), float(target)


def _upa_group(part):
    alpha, sep, belta = part.partition(":")
    try:
        if sep:
            return float(alpha), float(belta)
    except ValueError:
        pass
    raise ValueError(f"UPA sweep: every group reads alpha:belta, got {part!r}")


def parse_maskidx_sweep(text):
    """CLI form of a sweep: "0;0,1,2" -> [[0], [0, 1, 2]]; "" / None -> None (no sweep)."""
    return _parse(text, _ints)


def parse_target_sweep(text):
    """CLI form of a target sweep: "0:0;1:0;0,1,2:0.25" -> [([0], 0.0), ([1], 0.0), ([0, 1, 2], 0.25)] (maskidx[,maskidx...]:target per group)."""
    return _parse(text, _target_group)


def parse_upa_sweep(text):
    """CLI form of a UPA sweep: "0.8:0.2;0.5:0.5" -> [(0.8, 0.2), (0.5, 0.5)] (alpha:belta per group)."""
    return _parse(text, _upa_group)


def sweep_tag(maskidx) -> str:
    """Directory / log tag of a sweep group: [0] -> "maskidx0", [0, 1, 2] -> "maskidx0-1-2"."""
    return "maskidx" + "-".join(str(int(v)) for v in maskidx)


def target_sweep_tag(maskidx, target) -> str:
    """... of a target sweep group: ([0], 0.25) -> "maskidx0-target0.25", ([0, 1], 0) -> "maskidx0-1-target0" (%g of the target: equal groups
    give the same string, different ones different strings)."""
    return f"{sweep_tag(maskidx)}-target{float(target):g}"


def upa_sweep_tag(alpha, belta) -> str:
    """... of a UPA sweep group: (0.8, 0.2) -> "alpha0.8-belta0.2" (%g of the weights, as above)."""
    return f"alpha{float(alpha):g}-belta{float(belta):g}"


def mask_labels_sweep(labels, sweep):
    """[Bp, L] labels -> [P*Bp, L]: group p's copy masked with maskidx_p (mask_labels, UADA_ddp.py:89-97)."""
    return torch.cat([mask_labels(labels.clone(), m) for m in sweep], dim=0)


def sweep_rows(bs: int, sweep) -> int:
    """Labelled rows per rank of a maskidx sweep step: every sample keeps |maskidx_p| action tokens + EOS."""
    return sum(bs * (len(m) + 1) for m in sweep)


# ---- the groups' validity (ValueError without the parameter's name: check() puts it in front) ----
def _valid_maskidx(groups, lists):
    if not lists or any(len(m) == 0 for m in lists):
        raise ValueError("needs at least one group, and every group at least one maskidx")
    if any(v < 0 or v > 6 or len(set(m)) != len(m) for m in lists for v in m):
        raise ValueError(f"every maskidx is a distinct DoF index 0..6, got {groups}")
    return groups


def _maskidx_groups(groups):
    groups = [[int(v) for v in m] for m in groups]
    return _valid_maskidx(groups, groups)


def _target_groups(groups):
    groups = [([int(v) for v in m], float(t)) for m, t in groups]
    return _valid_maskidx(groups, [m for m, _ in groups])


def _upa_groups(groups):
    groups = [(float(a), float(b)) for a, b in groups]
    if not groups:
        raise ValueError("needs at least one (alpha, belta) group")
    if not all(np.isfinite(v) for pair in groups for v in pair):
        raise ValueError(f"every alpha / belta is a finite number, got {groups}")
    return groups


# ---- the head of a step: from the hidden rows `h` of all groups to this rank's message, up to the exchange ----
def _slice_head(attacker, h, segmap, groups, P, read, sink, msg, scalars, update):
    """K3s with the segmented map (K3h behind it on the `read` step), backward, the segmented epilogue with its fold: engine.slice_step_tail."""
    V = int(attacker.vla.lm_head.weight.shape[0])
    return attacker.slice_step_tail(h, segmap, float(attacker.MSE_weights), V, sink, msg, scalars, read, update, P=P)


def _gemm_head(attacker, h, segmap, groups, P, read, sink, msg, scalars, update, upa=False):
    """ONE hipBLASLt head over the rows of all groups, K3 with the segmented map (LOSS_CE, or `upa`: LOSS_UPA with the groups as its (alpha, beta)
    pairs), ONE head backward, K2' — the scalars are final before the backward, so the segmented epilogue runs in a pass-through form: a zero
    tail, or on the `read` step the groups' scalars as its tail."""
    pairs, w = groups if upa else None, float(attacker.MSE_weights)
    total, sc, _, pred_full = ops.HeadLossRowsSeg.apply(h, attacker.vla.lm_head.weight, segmap, P, pairs, w, 1.0)
    total.backward()
    if not read:
        ops.step_epilogue_seg(sink["partials"], msg, scalars, P, update=update)
        return None
    ops.step_epilogue_seg_tail(sink["partials"], msg, sc, P, update=update)
    return pred_full


def _tma_prepare(attacker, groups):
    attacker._tma_targets = [tma_target_tokens(float(t) * torch.ones(7).numpy(), m, attacker.action_tokenizer).to(attacker.device) for m, t in groups]


@dataclass(frozen=True)
class SweepKind:
    param: str               # the attacker's constructor argument / the wrapper's option
    attack_type: str         # the only attack_type it runs under
    what: str                # its name in logs and errors
    parse: Callable          # CLI text -> groups | None
    normalise: Callable      # groups as given -> groups as kept; refuses what no group may be
    tag: Callable            # group -> directory / log tag
    group_labels: Callable   # (attacker, labels [Bp,L], g) -> group g's labels, a new tensor
    head: Callable           # (attacker, h, segmap, groups, P, read, sink, msg, scalars, update) -> pred_full | None
    loss_mode: int           # K3's mode in the validation pass
    select_metric: int       # the scalar best-patch selection averages: 2 = MSE distance, 0 = the attack loss (as validate())
    prepare: Callable = lambda attacker, groups: None  # once per run, before the loop
    loss_args: Callable = lambda group: {}             # group -> model_loss keywords of its validation pass
    l1_clip: float = 0.0                 # K4's L1 clip (UPA.py:157)
    k4_in_epilogue: bool = True          # may a world-1 step apply AdamW inside the epilogue launch? else the exchange + K4 are always taken
    row_limit: int = None                # labelled rows per rank (sweep_rows) its head covers; None: no limit
    group_limit: int = None              # groups per step its K3 covers; None: no limit


MASKIDX = SweepKind(
    param="maskidx_sweep", attack_type="UADA", what="UADA maskidx sweep", parse=parse_maskidx_sweep, normalise=_maskidx_groups, tag=sweep_tag,
    group_labels=lambda attacker, labels, g: attacker.mask_labels(labels.clone(), attacker.sweep_groups[g]),  # UADA_ddp.py:89-97
    head=_slice_head, loss_mode=ops.LOSS_UADA_DDP, select_metric=2, row_limit=SWEEP_MAX_ROWS)
TARGET = SweepKind(
    param="target_sweep", attack_type="TMA", what="TMA target sweep", parse=parse_target_sweep, normalise=_target_groups,
    tag=lambda group: target_sweep_tag(*group), prepare=_tma_prepare,
    group_labels=lambda attacker, labels, g: tma_target_labels(labels, attacker._tma_targets[g]),  # TMA.py:124-129
    head=_gemm_head, loss_mode=ops.LOSS_CE, select_metric=0)
UPA = SweepKind(
    param="upa_sweep", attack_type="UPA", what="UPA weight sweep", parse=parse_upa_sweep, normalise=_upa_groups,
    tag=lambda group: upa_sweep_tag(*group), loss_args=lambda group: dict(alpha=group[0], beta=group[1]),
    group_labels=lambda attacker, labels, g: labels.clone(),  # reverse_direction: labels stay unmasked (UPA.py:127-129)
    head=partial(_gemm_head, upa=True), loss_mode=ops.LOSS_UPA, select_metric=0, group_limit=ops.SEG_UPA_MAX_GROUPS,
    l1_clip=1e-3, k4_in_epilogue=False)  # the clip needs the whole gradient's norm
KINDS = (MASKIDX, TARGET, UPA)


def check(attacker, kind: SweepKind, groups):
    """The groups of `kind` as the attacker keeps them; refuses (ValueError naming the parameter and the limit) what the batched sweep does not cover.
    The constructor checks the parameters it was given in KINDS' order, so `attacker.sweep_kind` is an earlier kind that was accepted already."""
    def refuse(why):
        raise ValueError(f"{kind.param}: {why}")

    if attacker.sweep_kind is not None:
        refuse(f"cannot be combined with {' or '.join(k.param for k in KINDS[:KINDS.index(kind)])} (one kind of sweep per run)")
    try:
        groups = kind.normalise(groups)
    except ValueError as e:
        refuse(e)
    P, bs = len(groups), attacker.bs
    if len({kind.tag(g) for g in groups}) != P:
        refuse(f"groups must be distinct, got {groups}")
    if attacker.attack_type != kind.attack_type:
        others = ", ".join(f"{k.attack_type} sweeps go through {k.param}" for k in KINDS if k is not kind)
        refuse(f"{kind.attack_type} only (got attack_type={attacker.attack_type!r}; {others})")
    if attacker.randomPatchTransform.resize_patch:
        refuse("resize_patch=True is not supported (one patch size per group only)")
    if attacker.randomPatchTransform.colorjitter:
        refuse("colorjitter is not supported (one shared patch per group only)")
    stages = attacker.randomPatchTransform.frame_stages_on()
    if stages:
        refuse(f"{stages[0]} is not supported ({frame_stage(stages[0]).why['sweep']})")
    if attacker.patch_reg_on:
        refuse("tv_weight / nps_weight are not supported (the sweeps' K4 lives inside the segmented epilogue: patch.grad is never materialised)")
    if not attacker.fused_ddp_available():
        refuse("needs the fused path (a model that exposes its patch-embed weights and hidden rows, VAA_FUSED_EPILOGUE != 0)")
    if P * bs > SWEEP_MAX_IMAGES:
        refuse(f"{P} groups x bs {bs} = {P * bs} images per rank exceed the limit of {SWEEP_MAX_IMAGES} (K2' one partial tile per image)")
    if kind.row_limit is not None and sweep_rows(bs, groups) > kind.row_limit:
        refuse(f"{sweep_rows(bs, groups)} labelled rows per rank (sum of bs x (|maskidx| + 1)) exceed the limit of {kind.row_limit} "
               f"(K3s covers at most {kind.row_limit} rows)")
    if kind.group_limit is not None and P > kind.group_limit:
        refuse(f"{P} groups exceed the limit of {kind.group_limit} (the groups' loss weights travel in K3's launch arguments)")
    return groups
