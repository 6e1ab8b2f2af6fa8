"""UADA, data-parallel over the GPUs of one node. Mirrors VLAAttacker/white_patch/UADA_ddp.py:36-344.

One process per GPU under torchrun (RANK / WORLD_SIZE / LOCAL_RANK), `torch.distributed` backend "nccl" (= RCCL over
xGMI). Same constructor arguments and `_attack_entry(rank, params, world)` / `attack(rank, world)` entry points as the
reference. What differs by design:
  * K1/K2 run on the GPU (the reference binds the transform to the CPU while the model is still there, Appendix A-D9);
  * no DistributedDataParallel wrapper around 7.5 B frozen parameters: the single trainable tensor is synchronised by
    one fused all-reduce per inner step (`dist.PatchGradSync`) and DDP's mean is folded into K4's grad_scale;
  * every rank seeds Python/NumPy with 42 (UADA_wrapper_ddp.py:53), so transform parameters per local index are
    identical across ranks, exactly like the reference.
`bs` is the PER-RANK batch (UADA_ddp.py:158); data are sharded by rank (tf.data shard in the reference, :157-160).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib
from .. import dist as vdist
from .. import ops
from ..labels import mask_labels as _mask_labels
from ..optim import CosineWarmupSchedule, PatchOptimizer, SweepPatchOptimizer
from .engine import AttackBase, ValReadback, to_dev, wandb, wandb_enabled


def default_model_factory(vla_path: str, device):
    """`vla_path` forms: "random:openvla-7b" / "random:tiny" (random init), "surrogate[:seed]", or a local HF checkpoint dir."""
    from ..openvla_model import build_openvla, load_hf_openvla, openvla_7b_cfg, tiny_cfg

    if vla_path.startswith("surrogate"):
        from ..surrogate import SurrogateVLA

        seed = int(vla_path.split(":")[1]) if ":" in vla_path else 0
        return SurrogateVLA(seed=seed).to(device)
    if vla_path.startswith("random:"):
        cfg = tiny_cfg() if vla_path.endswith("tiny") else openvla_7b_cfg()
        return build_openvla(cfg, device=device, dtype=torch.bfloat16)  # the transform hands over bf16 pixel_values, as the reference does
    if os.path.isdir(vla_path):
        return load_hf_openvla(build_openvla(openvla_7b_cfg(), device=device), vla_path)
    raise FileNotFoundError(
        f"no local OpenVLA checkpoint at {vla_path!r} (this image has no network); use 'random:openvla-7b' for shape-exact runs")


def default_dataset_factory(dataset_name: str, bs: int, rank: int, world: int):
    """Synthetic BridgeData-shaped loaders, sharded by rank through the seed (stands in for RLDSDataset.shard)."""
    from ..synthetic import SyntheticLoader

    return (SyntheticLoader(bs, seed=1234 + 1000003 * rank, kind="noise"), SyntheticLoader(bs, seed=99991 + 1000003 * rank, kind="noise"))


SWEEP_MAX_ROWS = 128    # labelled rows per rank K3s covers (vaa_head_slice_applies)
SWEEP_MAX_IMAGES = 512  # images per rank K2' keeps one partial tile each (vaa_patch_grad_partials)


def parse_maskidx_sweep(text):
    """CLI form of a sweep: "0;0,1,2" -> [[0], [0, 1, 2]]; "" / None -> None (no sweep)."""
    if text is None or not str(text).strip():
        return None
    return [[int(v) for v in part.split(",") if v.strip() != ""] for part in str(text).split(";")]


def sweep_tag(maskidx) -> str:
    """Directory / log tag of a sweep group: [0] -> "maskidx0", [0, 1, 2] -> "maskidx0-1-2"."""
    return "maskidx" + "-".join(str(int(v)) for v in maskidx)


def mask_labels_sweep(labels, sweep):
    """[Bp, L] labels -> [P*Bp, L]: group p's copy masked with maskidx_p (mask_labels, UADA_ddp.py:89-97)."""
    return torch.cat([_mask_labels(labels.clone(), m) for m in sweep], dim=0)


def sweep_rows(bs: int, sweep) -> int:
    """Labelled rows per rank of a sweep step: every sample keeps |maskidx_p| action tokens + EOS."""
    return sum(bs * (len(m) + 1) for m in sweep)


def parse_target_sweep(text):
    """CLI form of a target sweep: "0:0;1:0;0,1,2:0.25" -> [([0], 0.0), ([1], 0.0), ([0, 1, 2], 0.25)] (maskidx[,maskidx...]:target per group);
    "" / None -> None (no sweep)."""
    if text is None or not str(text).strip():
        return None
    out = []
    for part in str(text).split(";"):
        idx, sep, target = part.partition(":")
        if not sep or not target.strip():
            raise ValueError(f"target sweep: every group reads maskidx[,maskidx...]:target, got {part!r}")
        out.append(([int(v) for v in idx.split(",") if v.strip() != ""], float(target)))
    return out


def target_sweep_tag(maskidx, target) -> str:
    """Directory / log tag of a target sweep group: ([0], 0.25) -> "maskidx0-target0.25", ([0, 1], 0) -> "maskidx0-1-target0" (%g of the
    target: equal groups give the same string, different ones different strings)."""
    return f"{sweep_tag(maskidx)}-target{float(target):g}"


def parse_upa_sweep(text):
    """CLI form of a UPA sweep: "0.8:0.2;0.5:0.5" -> [(0.8, 0.2), (0.5, 0.5)] (alpha:belta per group); "" / None -> None (no sweep)."""
    if text is None or not str(text).strip():
        return None
    out = []
    for part in str(text).split(";"):
        alpha, sep, belta = part.partition(":")
        try:
            pair = (float(alpha), float(belta)) if sep else None
        except ValueError:
            pair = None
        if pair is None:
            raise ValueError(f"UPA sweep: every group reads alpha:belta, got {part!r}")
        out.append(pair)
    return out


def upa_sweep_tag(alpha, belta) -> str:
    """Directory / log tag of a UPA sweep group: (0.8, 0.2) -> "alpha0.8-belta0.2" (%g of the weights: equal groups give the same string,
    different ones different strings)."""
    return f"alpha{float(alpha):g}-belta{float(belta):g}"


class OpenVLAAttacker(AttackBase):
    val_batches = 100  # UADA_ddp.py:240
    val_every = 200  # UADA_ddp.py:233

    def __init__(self, vla_path, dataset_name, save_dir="", resize_patch=False, patch_size=[3, 50, 50], lr=0.01, bs=1, warmup=20,
                 num_iter=10000, maskidx=[], innerLoop=1, geometry=True, use_wandb=True, MSE_weights=1,
                 model_factory=None, dataset_factory=None, device=None, attack_type="UADA", alpha=0.8, belta=0.2, target_action=0.0, maskidx_sweep=None,
                 target_sweep=None, upa_sweep=None):
        """`attack_type`, `alpha`, `belta`, `target_action` are EXTENSIONS (the reference ships DDP for UADA only):
        "UPA" = UPA.py's reverse-direction loss + L1 grad clip, "TMA" = TMA.py's target-token CE, same data-parallel loop.
        `maskidx_sweep` (EXTENSION): a list of maskidx lists optimises one patch per list in ONE loop — every group sees the same frames, draws and
        schedule, and group p ends where a standalone run with maskidx = maskidx_sweep[p] and the same seed ends (DESIGN.md §maskidx sweep).
        None keeps the loop above exactly as it is; `maskidx` is then unused.
        `target_sweep` (EXTENSION, attack_type="TMA" only): a list of (maskidx list, target action value) pairs optimises one TMA patch per pair in
        ONE loop the same way — group p ends where a standalone TMA run with maskidx = maskidx_p, target_action = target_p and the same seed ends
        (DESIGN.md §maskidx sweep); `maskidx` and `target_action` are then unused. None: no target sweep.
        `upa_sweep` (EXTENSION, attack_type="UPA" only): a list of (alpha, belta) pairs optimises one UPA patch per pair in ONE loop the same way —
        group p ends where a standalone UPA run with alpha = alpha_p, belta = belta_p and the same seed ends (DESIGN.md §maskidx sweep); `alpha` and
        `belta` are then unused. None: no UPA sweep."""
        rank, world, local = vdist.env_rank_world()
        if device is None:
            device = vdist.local_device()
        self._rank, self._world = rank, world
        vla = (model_factory or default_model_factory)(vla_path, device)
        super().__init__(vla, None, save_dir, "adamW", resize_patch)
        self.device = torch.device(device)
        self.train_loader, self.val_loader = (dataset_factory or default_dataset_factory)(dataset_name, bs, rank, world)
        self.MSE_Distance_best = 1000000
        self.bs, self.lr, self.warmup, self.num_iter = bs, lr, warmup, num_iter
        self.maskidx, self.innerLoop, self.geometry = maskidx, innerLoop, geometry
        self.use_wandb = bool(use_wandb) and use_wandb != "false"  # Appendix A-D14
        self.patch_size = patch_size
        self.val_CE_loss, self.val_MSE_Distance, self.val_UAD = [], [], []
        self.MSE_weights = MSE_weights
        if attack_type not in ("UADA", "UPA", "TMA"):
            raise ValueError(f"attack_type must be UADA, UPA or TMA, got {attack_type!r}")
        self.attack_type, self.alpha, self.belta, self.target_action = attack_type, alpha, belta, target_action
        self.maskidx_sweep = None
        if maskidx_sweep is not None:
            self.maskidx_sweep = self._check_sweep(maskidx_sweep)
        self.target_sweep = None
        if target_sweep is not None:
            self.target_sweep = self._check_target_sweep(target_sweep, maskidx_sweep)
        self.upa_sweep = None
        if upa_sweep is not None:
            self.upa_sweep = self._check_upa_sweep(upa_sweep, maskidx_sweep, target_sweep)

    def _check_sweep(self, sweep):
        """Refuses (ValueError naming the limit) what the batched sweep does not cover."""
        sweep = [[int(v) for v in m] for m in sweep]
        if not sweep or any(len(m) == 0 for m in sweep):
            raise ValueError("maskidx_sweep: needs at least one group, and every group at least one maskidx")
        if any(v < 0 or v > 6 or len(set(m)) != len(m) for m in sweep for v in m):
            raise ValueError(f"maskidx_sweep: every maskidx is a distinct DoF index 0..6, got {sweep}")
        if len({sweep_tag(m) for m in sweep}) != len(sweep):
            raise ValueError(f"maskidx_sweep: groups must be distinct, got {sweep}")
        if self.attack_type != "UADA":
            raise ValueError(f"maskidx_sweep: UADA only (got attack_type={self.attack_type!r}; UPA / TMA sweeps are not implemented)")
        if self.randomPatchTransform.resize_patch:
            raise ValueError("maskidx_sweep: resize_patch=True is not supported (one patch size per group only)")
        if not self.fused_ddp_available():
            raise ValueError("maskidx_sweep: needs the fused path (a model that exposes its patch-embed weights and hidden rows, VAA_FUSED_EPILOGUE != 0)")
        if len(sweep) * self.bs > SWEEP_MAX_IMAGES:
            raise ValueError(f"maskidx_sweep: {len(sweep)} groups x bs {self.bs} = {len(sweep) * self.bs} images per rank exceed the limit of "
                             f"{SWEEP_MAX_IMAGES} (K2' one partial tile per image)")
        rows = sweep_rows(self.bs, sweep)
        if rows > SWEEP_MAX_ROWS:
            raise ValueError(f"maskidx_sweep: {rows} labelled rows per rank (sum of bs x (|maskidx| + 1)) exceed the limit of {SWEEP_MAX_ROWS} "
                             f"(K3s covers at most {SWEEP_MAX_ROWS} rows)")
        return sweep

    def _check_target_sweep(self, sweep, maskidx_sweep):
        """Refuses (ValueError naming the limit) what the batched target sweep does not cover."""
        if maskidx_sweep is not None:
            raise ValueError("target_sweep: cannot be combined with maskidx_sweep (one kind of sweep per run)")
        sweep = [([int(v) for v in m], float(t)) for m, t in sweep]
        if not sweep or any(len(m) == 0 for m, _ in sweep):
            raise ValueError("target_sweep: needs at least one group, and every group at least one maskidx")
        if any(v < 0 or v > 6 or len(set(m)) != len(m) for m, _ in sweep for v in m):
            raise ValueError(f"target_sweep: every maskidx is a distinct DoF index 0..6, got {sweep}")
        if len({target_sweep_tag(m, t) for m, t in sweep}) != len(sweep):
            raise ValueError(f"target_sweep: groups must be distinct, got {sweep}")
        if self.attack_type != "TMA":
            raise ValueError(f"target_sweep: TMA only (got attack_type={self.attack_type!r}; UADA sweeps go through maskidx_sweep, UPA sweeps are not implemented)")
        if self.randomPatchTransform.resize_patch:
            raise ValueError("target_sweep: resize_patch=True is not supported (one patch size per group only)")
        if not self.fused_ddp_available():
            raise ValueError("target_sweep: needs the fused path (a model that exposes its patch-embed weights and hidden rows, VAA_FUSED_EPILOGUE != 0)")
        if len(sweep) * self.bs > SWEEP_MAX_IMAGES:
            raise ValueError(f"target_sweep: {len(sweep)} groups x bs {self.bs} = {len(sweep) * self.bs} images per rank exceed the limit of "
                             f"{SWEEP_MAX_IMAGES} (K2' one partial tile per image)")
        return sweep

    def _check_upa_sweep(self, sweep, maskidx_sweep, target_sweep):
        """Refuses (ValueError naming the limit) what the batched UPA sweep does not cover."""
        if maskidx_sweep is not None or target_sweep is not None:
            raise ValueError("upa_sweep: cannot be combined with maskidx_sweep or target_sweep (one kind of sweep per run)")
        sweep = [(float(a), float(b)) for a, b in sweep]
        if not sweep:
            raise ValueError("upa_sweep: needs at least one (alpha, belta) group")
        if not all(np.isfinite(v) for pair in sweep for v in pair):
            raise ValueError(f"upa_sweep: every alpha / belta is a finite number, got {sweep}")
        if len({upa_sweep_tag(a, b) for a, b in sweep}) != len(sweep):
            raise ValueError(f"upa_sweep: groups must be distinct, got {sweep}")
        if self.attack_type != "UPA":
            raise ValueError(f"upa_sweep: UPA only (got attack_type={self.attack_type!r}; UADA sweeps go through maskidx_sweep, TMA sweeps through target_sweep)")
        if self.randomPatchTransform.resize_patch:
            raise ValueError("upa_sweep: resize_patch=True is not supported (one patch size per group only)")
        if not self.fused_ddp_available():
            raise ValueError("upa_sweep: needs the fused path (a model that exposes its patch-embed weights and hidden rows, VAA_FUSED_EPILOGUE != 0)")
        if len(sweep) * self.bs > SWEEP_MAX_IMAGES:
            raise ValueError(f"upa_sweep: {len(sweep)} groups x bs {self.bs} = {len(sweep) * self.bs} images per rank exceed the limit of "
                             f"{SWEEP_MAX_IMAGES} (K2' one partial tile per image)")
        if len(sweep) > ops.SEG_UPA_MAX_GROUPS:
            raise ValueError(f"upa_sweep: {len(sweep)} groups exceed the limit of {ops.SEG_UPA_MAX_GROUPS} (the groups' loss weights travel in K3's "
                             f"launch arguments)")
        return sweep

    def setup(self, rank, world_size):
        vdist.init_process_group(device=self.device if self.device.type == "cuda" else None)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)

    def cleanup(self):
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()

    def mask_labels(self, labels, maskidx):
        return _mask_labels(labels, maskidx)

    def attack(self, rank, world_size):
        self.setup(rank, world_size)
        try:
            return self._attack(rank, world_size)
        finally:  # also when the run ends with NonFiniteAttackState: a process that leaves its group open can block at exit
            self.cleanup()

    def _attack(self, rank, world_size):
        if self.maskidx_sweep is not None or self.target_sweep is not None or self.upa_sweep is not None:
            return self._attack_sweep(rank, world_size)
        dev = self.device
        if rank == 0:
            patch = torch.rand(self.patch_size).to(dev)  # UADA_ddp.py:140-141
        else:
            patch = torch.empty(self.patch_size).to(dev)
        vdist.broadcast_patch(patch, src=0)  # C1
        patch.requires_grad_(True)
        self.patch = patch
        optimizer = PatchOptimizer(patch, self.lr, "adamW", l1_clip=1e-3 if self.attack_type == "UPA" else 0.0)  # UPA.py:157
        scheduler = CosineWarmupSchedule(optimizer, self.warmup, int(self.num_iter), 0.5)
        if self.attack_type == "TMA":
            from ..labels import tma_target_tokens

            self._tma_target = tma_target_tokens(float(self.target_action) * torch.ones(7).numpy(), self.maskidx, self.action_tokenizer).to(dev)
        sync = vdist.PatchGradSync(patch.numel(), 4, dev)
        pick = torch.tensor([1, 2, 7, 0], dtype=torch.int64, device=dev)  # CE, w^2*MSE, UAD, total of K3's scalars
        # UADA on a model that exposes its patch-embed weights: K2's final sum, K3's fold and the message packing are ONE launch
        fused = self.attack_type == "UADA" and self.fused_ddp_available()
        scalars = torch.zeros(8, dtype=torch.float32, device=dev)

        for i, data in enumerate(self.train_loader):
            if i == self.num_iter:
                break
            pixel_values, labels, attention_mask, input_ids = to_dev(data, dev)
            labels = self._prepare_labels(labels)

            def step(inner_loop):
                optimizer.zero_grad()
                # the loop reads the loss scalars of the LAST inner step only (UADA_ddp.py:214-221, below): the full-vocabulary CE is evaluated there
                full_ce = inner_loop == self.innerLoop - 1 or os.environ.get("VAA_FULL_CE_EVERY_STEP", "0") == "1"  # (=1: K3h behind K3s on every step; same patch bits)
                if fused:  # world 1: nothing to exchange, K4 runs inside the epilogue launch (five launches per step)
                    self.fused_ddp_step(pixel_values, patch, input_ids, attention_mask, labels, self.geometry, float(self.MSE_weights),
                                        sync.buf, scalars, optimizer=optimizer if world_size == 1 else None, full_ce=full_ce)
                    return None if world_size == 1 else sync.allreduce_packed  # C3 + C4 in one message: [grad | CE, MSE, UAD, total]
                pix = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std, geometry=self.geometry)
                total, sc, _ = self.model_loss(input_ids, attention_mask, pix, labels, self._loss_mode(), w=float(self.MSE_weights),
                                               alpha=self.alpha, beta=self.belta, full_ce=full_ce, read_scalars=full_ce)
                total.backward()  # K2 inside
                return lambda: sync.allreduce_step(patch.grad, sc, pick)

            s_sum, device_failure = self._inner_loop(optimizer, sync, world_size, step)
            self._end_outer(i, rank, world_size, scheduler, optimizer, s_sum, device_failure, f"{self.attack_type} (data parallel) outer iteration {i}")
        return patch

    # ---- maskidx sweep: P patches in one loop ----
    def _attack_sweep(self, rank, world_size):
        """The loop above for P patch groups at once (UADA, fused path): one [P*bs] step per inner step — K1 tile-major with one patch per group,
        ONE forward / backward, K3s with the segmented row map, K2' with a partial per image, the segmented epilogue (+ AdamW of every group);
        at world > 1 ONE all-reduce of [P gradients | P x 4 scalars] and the segmented K4. The RNG streams are consumed as by ONE standalone run:
        one patch init (every group starts from it), one transform draw per frame and step, shared by the groups.
        A target sweep (TMA) is the same loop with the groups' target labels and, per step, ONE hipBLASLt head + K3 in LOSS_CE mode over the
        segmented map (target_sweep_step) in place of K3s. A UPA sweep is that loop again with every group's labels left unmasked, K3 in LOSS_UPA
        mode with the group's (alpha, belta) (upa_sweep_step) and — the L1 clip needs the whole gradient's norm — the segmented K4 behind the
        epilogue at every world size."""
        dev = self.device
        tma, upa = self.target_sweep is not None, self.upa_sweep is not None
        sweep = self.target_sweep if tma else (self.upa_sweep if upa else self.maskidx_sweep)
        P = len(sweep)
        if upa:
            self.sweep_tags = [upa_sweep_tag(a, b) for a, b in sweep]
        elif tma:
            from ..labels import tma_target_tokens

            self.sweep_tags = [target_sweep_tag(m, t) for m, t in sweep]
            self._tma_targets = [tma_target_tokens(float(t) * torch.ones(7).numpy(), m, self.action_tokenizer).to(dev) for m, t in sweep]
        else:
            self.sweep_tags = [sweep_tag(m) for m in sweep]
        what = "TMA target sweep" if tma else ("UPA weight sweep" if upa else "UADA maskidx sweep")
        if rank == 0:
            p0 = torch.rand(self.patch_size).to(dev)  # UADA_ddp.py:140-141, drawn once: every group's standalone run draws this patch
        else:
            p0 = torch.empty(self.patch_size).to(dev)
        vdist.broadcast_patch(p0, src=0)
        patches = p0.unsqueeze(0).repeat(P, *([1] * p0.dim())).contiguous().requires_grad_(True)
        self.patch = patches
        optimizer = SweepPatchOptimizer(patches, self.lr, "adamW", l1_clip=1e-3 if upa else 0.0)  # UPA.py:157, per group
        scheduler = CosineWarmupSchedule(optimizer, self.warmup, int(self.num_iter), 0.5)
        sync = vdist.PatchGradSync(patches.numel(), 4 * P, dev)
        scalars = torch.zeros((P, 8), dtype=torch.float32, device=dev)
        W = self.vla.lm_head.weight
        V = int(W.shape[0])
        w = float(self.MSE_weights)
        self.MSE_Distance_best = {t: 1000000 for t in self.sweep_tags}
        self.val_CE_loss = {t: [] for t in self.sweep_tags}
        self.val_MSE_Distance = {t: [] for t in self.sweep_tags}
        self.val_UAD = {t: [] for t in self.sweep_tags}

        for i, data in enumerate(self.train_loader):
            if i == self.num_iter:
                break
            pixel_values, labels, attention_mask, input_ids = to_dev(data, dev)
            # the batch replicated to P groups ONCE per outer iteration (frames, ids, mask), the labels masked per group, ONE segmented row map
            img = self.randomPatchTransform.stage_images(pixel_values)
            img_all = img.repeat(P, 1, 1, 1).contiguous()
            ids_all = input_ids.repeat(P, 1).contiguous()
            am_all = attention_mask.repeat(P, 1).contiguous() if attention_mask is not None else None
            labels_all = torch.cat([self._sweep_group_labels(labels, g) for g in range(P)], dim=0)
            row_index = self.vla.label_row_index(labels_all)
            R = int(row_index.numel())
            if R == 0:
                raise ValueError(f"{what}: no labelled position in the batch")
            if not tma and not upa and not self._slice_head(R, None, W):
                raise ValueError(f"maskidx sweep: K3s does not take {R} labelled rows per rank here (limit {SWEEP_MAX_ROWS} rows, bf16 head)")
            segmap = ops.LossRowMapSeg(labels_all, P)
            pack = self.vla.make_pack(am_all) if (hasattr(self.vla, "make_pack") and am_all is not None) else None

            def step(inner_loop):
                read = inner_loop == self.innerLoop - 1  # the step whose loss scalars the loop reads (UADA_ddp.py:214-221)
                if upa:  # the clip keeps K4 out of the epilogue: at world 1 the exchange hands the message back as it is, K4 follows
                    self.upa_sweep_step(img_all, patches, ids_all, row_index, segmap, pack, sync.buf, scalars, read)
                    return sync.allreduce_packed
                upd = optimizer.fused_update_args() if world_size == 1 else None
                if tma:
                    self.target_sweep_step(img_all, patches, ids_all, row_index, segmap, pack, sync.buf, scalars, read, upd)
                else:
                    self.sweep_step(img_all, patches, ids_all, labels_all, row_index, segmap, pack, w, V, sync.buf, scalars, read, upd)
                return None if world_size == 1 else sync.allreduce_packed

            s_sum, device_failure = self._inner_loop(optimizer, sync, world_size, step)
            self._end_outer(i, rank, world_size, scheduler, optimizer, s_sum, device_failure,
                            f"{what} (data parallel) outer iteration {i}", tags=self.sweep_tags)
        return patches

    def _inner_loop(self, optimizer, sync, world_size, step):
        """The inner steps of one outer iteration (both loops above). `step(inner_loop)` runs this rank's step up to the exchange and returns the
        all-reduce of its message (-> gradient sum, scalar sums), or None when there is nothing to exchange (world 1: K4 ran inside the epilogue);
        K4 then takes the rank-mean gradient (DDP's mean folded into grad_scale). Returns (the scalar sums of the last step, device_failure)."""
        s_sum = sync.buf[sync.n_grad :]
        inv_world = 1.0 / world_size
        device_failure = None  # a library call of THIS rank reported a device-side failure (the sticky word, e.g. a hand-over that timed out)
        for inner_loop in range(self.innerLoop):
            exchanged = False
            if device_failure is None:
                try:
                    exchange = step(inner_loop)
                    if exchange is None:
                        s_sum = sync.buf[sync.n_grad :]
                        continue
                    exchanged = True
                    g_sum, s_sum = exchange()
                    optimizer.step(grad=g_sum.view_as(optimizer.patch), grad_scale=inv_world)  # K4, DDP mean folded in
                except _lib.VaaError as e:
                    # The failure word is sticky: every library call of this rank fails until it is polled. Raising here would leave the OTHER
                    # ranks waiting in this step's all-reduce until the RCCL timeout: poll it now (the poll clears it), keep the
                    # collective's cadence with a NaN message for the rest of the outer iteration, and let the all-reduced verdict of
                    # assert_finite_state take every rank out of the loop together.
                    device_failure = str(e)
                    try:
                        ops.async_error_check()
                    except _lib.VaaError:
                        pass
            if device_failure is not None and world_size > 1 and not exchanged:
                sync.buf.fill_(float("nan"))
                _, s_sum = sync.allreduce_packed()
        return s_sum, device_failure

    def _end_outer(self, i, rank, world_size, scheduler, optimizer, s_sum, device_failure, where, tags=None):
        """The end of an outer iteration (both loops): schedule, the one read-back, the all-ranks finiteness verdict, the train log (one flat dict;
        per group tag for a sweep) and the validation cadence."""
        scheduler.step()
        s = (s_sum * (1.0 / world_size)).cpu().numpy()
        if tags is not None:
            s = s.reshape(len(tags), 4)
        self.assert_finite_state(optimizer.patch, optimizer, s, where, all_ranks=True, device_failure=device_failure)
        # UADA_ddp.py:207,216-217: `patch.grad.mean()` AFTER DistributedDataParallel averaged the gradient, i.e. the mean of the averaged
        # gradient (identical on every rank, so the reference's MAX all-reduce of it is the value itself): K4 reports it
        stats = optimizer.last_stats.cpu().numpy().reshape(-1, 2)
        lr = optimizer.param_groups[0]["lr"]
        logs = [{"TRAIN_attack_loss(CE)": float(sg[0]), "TRAIN_patch_gradient": float(st[1]), "TRAIN_LR": lr,
                 "TRAIN_attack_loss (MSE_Distance)": float(sg[1]), "TRAIN_UAD": float(sg[2])} for sg, st in zip(s.reshape(-1, 4), stats)]
        if tags is None:
            self.last_train_log = logs[0]
            if rank == 0 and self.use_wandb and wandb is not None:
                wandb.log(logs[0], step=i)
        else:
            self.last_train_log = dict(zip(tags, logs))
            for tag, log in self.last_train_log.items():
                if rank == 0 and self.use_wandb and wandb is not None:
                    wandb.log({f"{tag}/{k}": v for k, v in log.items()}, step=i)
        if i % self.val_every == 0:
            (self.validate if tags is None else self.validate_sweep)(i, optimizer.patch, rank)

    def sweep_step(self, img_all, patches, input_ids, labels_all, row_index, segmap, pack, w, V, msg, scalars, full_ce, update=None):
        """One inner step of the sweep up to the exchange: K1 (one draw per frame, every group) -> body over P*bs images -> K3s (segmented map: each
        row normalised by its group's count; K3h behind it when `full_ce`) -> K2' (a partial per image) -> ONE segmented epilogue: msg = [P gradients
        | P x {CE, w^2*MSE, UAD, total}] (zero tail unless `full_ce`), scalars [P,8] folded per group; `update` = AdamW of every group inside it."""
        sink = {}
        pe = self.randomPatchTransform.apply_sweep_batch(img_all, patches, self.mean, self.std, self.geometry, sink)
        h = self.vla.hidden_rows(input_ids, None, row_index, patch_embeds=pe, pack=pack)
        return self.slice_step_tail(h, segmap, w, V, sink, msg, scalars, full_ce, update, P=int(patches.shape[0]))

    def target_sweep_step(self, img_all, patches, input_ids, row_index, segmap, pack, msg, scalars, read, update=None):
        """One inner step of the target sweep up to the exchange: K1 (one draw per frame, every group) -> body over P*bs images -> ONE hipBLASLt head
        over the rows of all groups -> K3 in LOSS_CE mode with the segmented map (each row normalised by its group's row count, every group folded on
        its own) -> ONE dh = g @ W, backward, K2' (a partial per image) -> ONE segmented epilogue in its pass-through form: msg = [P gradients |
        P x {CE, 0, UAD, total}] on the step whose scalars are `read` (K3 made them final before the backward), a zero tail on the others (`scalars`
        [P,8] is then left as it is); `update` = AdamW of every group inside the launch."""
        sink = {}
        P = int(patches.shape[0])
        pe = self.randomPatchTransform.apply_sweep_batch(img_all, patches, self.mean, self.std, self.geometry, sink)
        h = self.vla.hidden_rows(input_ids, None, row_index, patch_embeds=pe, pack=pack)
        total, sc, _, pred_full = ops.HeadLossRowsSeg.apply(h, self.vla.lm_head.weight, segmap, P, 1.0)
        total.backward()
        if not read:
            ops.step_epilogue_seg(sink["partials"], msg, scalars, P, update=update)
            return None
        ops.step_epilogue_seg_tail(sink["partials"], msg, sc, P, update=update)
        return pred_full

    def upa_sweep_step(self, img_all, patches, input_ids, row_index, segmap, pack, msg, scalars, read, pairs=None):
        """One inner step of the UPA sweep up to the exchange: K1 (one draw per frame, every group) -> body over P*bs images -> ONE hipBLASLt head
        over the rows of all groups -> K3 in LOSS_UPA mode with the segmented map (every group's batch means and (alpha, belta) its own) -> ONE
        dh = g_slice @ W[31744:32000], backward, K2' (a partial per image) -> ONE segmented epilogue in its pass-through form: msg = [P gradients |
        P x {CE, w^2*MSE, UAD, total}] on the step whose scalars are `read`, a zero tail on the others (`scalars` [P,8] is then left as it is). K4
        is never fused here: the caller runs the segmented K4 with the L1 clip on the (all-reduced) message. `pairs`: the groups' (alpha, belta), the
        attacker's `upa_sweep` when None."""
        sink = {}
        P = int(patches.shape[0])
        pe = self.randomPatchTransform.apply_sweep_batch(img_all, patches, self.mean, self.std, self.geometry, sink)
        h = self.vla.hidden_rows(input_ids, None, row_index, patch_embeds=pe, pack=pack)
        total, sc, _, pred_full = ops.HeadLossRowsSegUpa.apply(h, self.vla.lm_head.weight, segmap, P, self.upa_sweep if pairs is None else pairs,
                                                              float(self.MSE_weights), 1.0)
        total.backward()
        if not read:
            ops.step_epilogue_seg(sink["partials"], msg, scalars, P)
            return None
        ops.step_epilogue_seg_tail(sink["partials"], msg, sc, P)
        return pred_full

    def _sweep_group_labels(self, labels, g):
        """Group g's labels of a sweep (a new tensor): masked with its maskidx (UADA_ddp.py:89-97), its TMA target labels (TMA.py:124-129), or —
        UPA reverse_direction — left unmasked (UPA.py:127-129)."""
        if self.upa_sweep is not None:
            return labels.clone()
        if self.target_sweep is not None:
            from ..labels import tma_target_labels

            return tma_target_labels(labels, self._tma_targets[g])
        return self.mask_labels(labels.clone(), self.maskidx_sweep[g])

    def validate_sweep(self, i, patches, rank):
        """validate() per group: every validation batch is drawn ONCE (the RNG consumption of one standalone pass) and evaluated with each group's
        patch and labels; per group the averages, the AVG all-reduces, best-patch selection and the files under save_dir/<group tag>/."""
        tma, upa = self.target_sweep is not None, self.upa_sweep is not None
        mode = ops.LOSS_CE if tma else (ops.LOSS_UPA if upa else ops.LOSS_UADA_DDP)
        rbs = [ValReadback(self.val_batches, self.device) for _ in self.sweep_tags]
        last_images = [None] * len(rbs)
        ph, pw = int(patches.shape[2]), int(patches.shape[3])
        with torch.no_grad():
            for j, data in enumerate(self.val_loader):
                if j == self.val_batches:
                    break
                pixel_values, labels, attention_mask, input_ids = to_dev(data, self.device)
                img = self.randomPatchTransform.stage_images(pixel_values)
                draws = self.randomPatchTransform.draw_params(int(img.shape[0]), ph, pw, self.geometry)
                for g in range(len(rbs)):
                    modified = self.randomPatchTransform.apply_random_patch_batch(img, patches[g].detach(), mean=self.mean, std=self.std,
                                                                                   geometry=self.geometry, draws=draws)
                    lab = self._sweep_group_labels(labels, g)
                    ab = dict(alpha=self.upa_sweep[g][0], beta=self.upa_sweep[g][1]) if upa else {}
                    _, sc, _ = self.model_loss(input_ids, attention_mask, modified, lab, mode, w=float(self.MSE_weights), need_grad=False, **ab)
                    rbs[g].add(sc)
                    last_images[g] = modified
        self.last_val_log = {}
        for g, tag in enumerate(self.sweep_tags):
            # selection metric: MSE distance (UADA) or the attack loss (TMA, UPA), as validate() picks it
            self.last_val_log[tag] = self._val_record(i, rank, rbs[g].read()[0], 0 if (tma or upa) else 2, patches[g], last_images[g], tag)

    def _loss_mode(self):
        return {"UADA": ops.LOSS_UADA_DDP, "UPA": ops.LOSS_UPA, "TMA": ops.LOSS_CE}[self.attack_type]

    def _prepare_labels(self, labels):
        if self.attack_type == "UADA":
            return self.mask_labels(labels, self.maskidx)
        if self.attack_type == "TMA":
            from ..labels import tma_target_labels

            return tma_target_labels(labels, self._tma_target)
        return labels  # UPA reverse_direction: labels stay unmasked (UPA.py:127-129)

    def validate(self, i, patch, rank):
        """UADA_ddp.py:233-324: 100 local val batches, 3 scalar all-reduces (C5), rank 0 writes the files."""
        modified_images = None
        rb = ValReadback(self.val_batches, self.device)  # one read-back behind the last batch instead of one per batch
        with torch.no_grad():
            for j, data in enumerate(self.val_loader):
                if j == self.val_batches:
                    break
                pixel_values, labels, attention_mask, input_ids = to_dev(data, self.device)
                modified_images = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch.detach(), mean=self.mean,
                                                                                      std=self.std, geometry=self.geometry)
                labels = self._prepare_labels(labels)
                _, scalars, _ = self.model_loss(input_ids, attention_mask, modified_images, labels, self._loss_mode(),
                                                w=float(self.MSE_weights), alpha=self.alpha, beta=self.belta, need_grad=False)
                rb.add(scalars)
        # selection metric: MSE distance (UADA) or the attack loss
        self.last_val_log = self._val_record(i, rank, rb.read()[0], 2 if self.attack_type == "UADA" else 0, patch, modified_images)

    def _val_record(self, i, rank, host, metric, patch, images, tag=None):
        """What validate() does with the scalars of its batches — the run's or, with a sweep group's `tag`, that group's (containers keyed by
        the tag, files under save_dir/<tag>/): the averages, the 3 AVG all-reduces, best-patch selection, the saved patches and the lists.
        `metric`: the scalar the selection averages. Returns the validation log."""
        avg_CE = avg_MSE = avg_UAD = 0.0
        for s in host:
            avg_MSE += float(np.float32(s[metric]))
            avg_UAD += float(np.float32(s[7]))
            avg_CE += float(np.float32(s[1]))
        avg_MSE /= self.val_batches
        avg_UAD /= self.val_batches
        avg_CE /= self.val_batches
        g_MSE = vdist.allreduce_scalar(avg_MSE, "AVG", self.device)
        g_UAD = vdist.allreduce_scalar(avg_UAD, "AVG", self.device)
        g_CE = vdist.allreduce_scalar(avg_CE, "AVG", self.device)
        log = {"VAL_MSE_Distance": g_MSE, "VAL_UAD": g_UAD}
        if rank == 0:
            pre = "" if tag is None else f"{tag}/"
            best = self.MSE_Distance_best if tag is None else self.MSE_Distance_best[tag]
            if g_MSE < best:
                if tag is None:
                    self.MSE_Distance_best = g_MSE
                else:
                    self.MSE_Distance_best[tag] = g_MSE
                d = self.save_patch(patch, pre + str(i))
                _, pil = self.save_val_images(images, d)
                if self.use_wandb and wandb is not None:
                    wandb.log({pre + k: v for k, v in log.items()}, step=i)
                    wandb.log({pre + "AdvImg": [wandb.Image(p) for p in pil]})
            d = self.save_patch(patch, pre + "last")
            os.makedirs(os.path.join(d, "val_related_data"), exist_ok=True)
            for lst, v in ((self.val_CE_loss, g_CE), (self.val_MSE_Distance, g_MSE), (self.val_UAD, g_UAD)):
                (lst if tag is None else lst[tag]).append(v)
        return log

    @classmethod
    def run(cls, **instance_params):
        """UADA_ddp.py:326-336 spawns one process per visible GPU; torchrun is the supported launcher here."""
        import torch.multiprocessing as mp

        world_size = max(torch.cuda.device_count(), 1)
        mp.spawn(cls._spawn_entry, args=(instance_params, world_size), nprocs=world_size)

    @staticmethod
    def _spawn_entry(rank, instance_params, world_size):
        os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world_size))
        OpenVLAAttacker._attack_entry(rank, instance_params, world_size)

    @staticmethod
    def _attack_entry(rank, instance_params, world_size):
        """UADA_ddp.py:338-344."""
        instance = OpenVLAAttacker(**instance_params)
        return instance.attack(rank, world_size)
