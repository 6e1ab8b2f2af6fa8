#!/usr/bin/env python3
"""Measures the maskidx sweep step against P standalone steps (one GPU, world size 1, the fused data-parallel UADA step with AdamW inside the
epilogue): OpenVLA-7B shapes with random weights by default.

    python tools/sweep_bench.py --configs 2x8,8x4,8x8 --steps 10 --warmup 3 [--vla random:openvla-7b] [--out file.json] [--attack tma|upa]

--attack tma measures the TMA target sweep step (one DoF per group, the T-dof1 .. T-dof7 family) against P standalone TMA steps of the
data-parallel loop (the unfused step: K1, model, hipBLASLt head + K3, backward with K2', message, K4).

--attack upa measures the UPA weight sweep step (one (alpha, belta) pair per group, labels unmasked: 8 labelled rows per image) against P
standalone UPA steps of the data-parallel loop (K1, model, the loop's own head choice + K3, backward with K2', message, K4 with the L1 clip).

For each (P, Bp): ms per standalone step at bs = Bp (maskidx [0]), ms per sweep step over P groups x Bp images (one DoF per group), their ratio, and the library's own kernels per step (vaa_prof per-dispatch timer: the hand-written microseconds of one step).
Every step runs with full_ce on its last inner step only, as the loop does (innerLoop = `--inner`)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _groups(P):
    """One DoF per group ({0}, {1}, ..., {6}, then {0} again): two labelled rows per sample like the standalone maskidx [0] step, so (8, 8) stays
    within K3s's 128 rows (a sweep that keeps more DoFs per group needs a smaller P x Bp)."""
    return [[q % 7] for q in range(P)]


def _target_groups(P):
    """--attack tma: one DoF per group like the released T-dof1 .. T-dof7 family, target 0 (then 0.5 for an eighth group and beyond)."""
    return [([q % 7], 0.0 if q < 7 else 0.5) for q in range(P)]


def _upa_groups(P):
    """--attack upa: P distinct (alpha, belta) pairs from (1, 0) towards (0, 1)."""
    return [(1.0 - q / max(P, 2), q / max(P, 2)) for q in range(P)]


def measure(att, P, Bp, steps, warmup, inner, sweep, attack="uada"):
    from roboticattack_amd import dist as vdist, ops, synthetic
    from roboticattack_amd.attack import sweep as kinds
    from roboticattack_amd.labels import tma_target_labels, tma_target_tokens
    from roboticattack_amd.optim import PatchOptimizer, SweepPatchOptimizer

    dev = att.device
    batch = synthetic.synth_batch(1234, Bp, "noise")
    pv = att.randomPatchTransform.stage_images(batch["pixel_values"])
    labels = batch["labels"].to(dev)
    ids, am = batch["input_ids"].to(dev), batch["attention_mask"].to(dev)
    n = 3 * 50 * 50
    if sweep:  # the loop's own step (OpenVLAAttacker._attack_sweep at world 1) through the kind table
        kind, make = dict(uada=(kinds.MASKIDX, _groups), tma=(kinds.TARGET, _target_groups), upa=(kinds.UPA, _upa_groups))[attack]
        att.sweep_kind, att.sweep_groups = kind, make(P)
        kind.prepare(att, att.sweep_groups)
        patches = torch.rand(P, 3, 50, 50, device=dev, requires_grad=True)
        opt = SweepPatchOptimizer(patches, 1e-3, l1_clip=kind.l1_clip)
        img = pv.repeat(P, 1, 1, 1).contiguous()
        ids_all, am_all = ids.repeat(P, 1).contiguous(), am.repeat(P, 1).contiguous()
        lab = torch.cat([kind.group_labels(att, labels, g) for g in range(P)])
        row_index = att.vla.label_row_index(lab)
        segmap = ops.LossRowMapSeg(lab, P)
        pack = att.vla.make_pack(am_all) if hasattr(att.vla, "make_pack") else None
        sync = None if kind.k4_in_epilogue else vdist.PatchGradSync(patches.numel(), 4 * P, dev)
        msg = torch.zeros(P * (n + 4), device=dev) if sync is None else sync.buf
        sc = torch.zeros((P, 8), device=dev)

        def step(k):
            att.sweep_step(img, patches, ids_all, row_index, segmap, pack, msg, sc, k % inner == inner - 1,
                           opt.fused_update_args() if sync is None else None)
            if sync is not None:  # K4 behind the epilogue (the L1 clip)
                g_sum, _ = sync.allreduce_packed()
                opt.step(grad=g_sum.view_as(patches), grad_scale=1.0)
    elif attack == "uada":
        patch = torch.rand(3, 50, 50, device=dev, requires_grad=True)
        opt = PatchOptimizer(patch, 1e-3)
        lab = att.mask_labels(labels.clone(), [0])
        msg = torch.zeros(n + 4, device=dev)
        sc = torch.zeros(8, device=dev)

        def step(k):
            att.fused_ddp_step(pv, patch, ids, am, lab, True, 5.0, msg, sc, optimizer=opt, full_ce=k % inner == inner - 1)
    else:  # the standalone TMA / UPA step of the data-parallel loop (OpenVLAAttacker._attack at world 1)
        mode, lab, clip = (ops.LOSS_UPA, labels.clone(), 1e-3) if attack == "upa" else (
            ops.LOSS_CE, tma_target_labels(labels, tma_target_tokens(np.zeros(7), [0]).to(dev)), 0.0)
        patch = torch.rand(3, 50, 50, device=dev, requires_grad=True)
        opt = PatchOptimizer(patch, 1e-3, l1_clip=clip)
        sync = vdist.PatchGradSync(patch.numel(), 4, dev)
        pick = torch.tensor([1, 2, 7, 0], dtype=torch.int64, device=dev)

        def step(k):
            opt.zero_grad()
            full_ce = k % inner == inner - 1
            pix = att.randomPatchTransform.apply_random_patch_batch(pv, patch, mean=att.mean, std=att.std, geometry=True)
            total, scal, _ = att.model_loss(ids, am, pix, lab, mode, w=5.0, alpha=0.8, beta=0.2, full_ce=full_ce, read_scalars=full_ce)
            total.backward()
            g_sum, _ = sync.allreduce_step(patch.grad, scal, pick)
            opt.step(grad=g_sum.view_as(patch), grad_scale=1.0)

    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    ops.prof_start(4096)
    for k in range(inner):
        step(k)
    torch.cuda.synchronize()
    recs = ops.prof_collect()
    hand = sum(us for _, us in recs) / inner
    per = {}
    for nm, us in recs:
        per[nm] = per.get(nm, 0.0) + us / inner
    return ms, hand, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2x8,8x4,8x8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--vla", default="random:openvla-7b")
    ap.add_argument("--out", default="")
    ap.add_argument("--attack", default="uada", choices=["uada", "tma", "upa"],
                    help="tma: the target sweep step (one hipBLASLt head + segmented K3 for all groups) against P standalone TMA steps of the data-parallel "
                         "loop; upa: the UPA weight sweep step against P standalone UPA steps of that loop")
    a = ap.parse_args()
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    from roboticattack_amd.attack import uada_ddp

    torch.manual_seed(0)
    np.random.seed(0)
    att = uada_ddp.OpenVLAAttacker(vla_path=a.vla, dataset_name="synthetic", bs=8, use_wandb=False, maskidx=[0], MSE_weights=5,
                                   dataset_factory=lambda *x: (None, None))
    assert att.fused_ddp_available()
    out = []
    solo = {}
    for cfg in a.configs.split(","):
        P, Bp = (int(v) for v in cfg.split("x"))
        if Bp not in solo:
            solo[Bp] = measure(att, 1, Bp, a.steps, a.warmup, a.inner, sweep=False, attack=a.attack)
        sw = measure(att, P, Bp, a.steps, a.warmup, a.inner, sweep=True, attack=a.attack)
        rec = dict(attack=a.attack, P=P, Bp=Bp, images=P * Bp, standalone_ms=round(solo[Bp][0], 2), P_standalone_ms=round(P * solo[Bp][0], 2),
                   sweep_ms=round(sw[0], 2), ratio=round(sw[0] / (P * solo[Bp][0]), 3), standalone_hand_us=round(solo[Bp][1], 1),
                   sweep_hand_us=round(sw[1], 1), sweep_hand_kernels_us={k: round(v, 1) for k, v in sorted(sw[2].items())})
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
