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
from ..labels import tma_target_labels, tma_target_tokens
from ..optim import CosineWarmupSchedule, PatchOptimizer, SweepPatchOptimizer
from .engine import AttackBase, ValReadback, to_dev, wandb, wandb_enabled
from .sweep import (KINDS, SWEEP_MAX_IMAGES, SWEEP_MAX_ROWS, check as check_sweep, mask_labels_sweep, parse_maskidx_sweep,  # noqa: F401 (the names
                    parse_target_sweep, parse_upa_sweep, sweep_rows, sweep_tag, target_sweep_tag, upa_sweep_tag)  # live in sweep.py; importable here)


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


class OpenVLAAttacker(AttackBase):
    val_batches = 100  # UADA_ddp.py:240
    val_every = 200  # UADA_ddp.py:233

    def __init__(self, vla_path, dataset_name, save_dir="", resize_patch=False, patch_size=[3, 50, 50], lr=0.01, bs=1, warmup=20,
                 num_iter=10000, maskidx=[], innerLoop=1, geometry=True, use_wandb=True, MSE_weights=1,
                 model_factory=None, dataset_factory=None, device=None, attack_type="UADA", alpha=0.8, belta=0.2, target_action=0.0, maskidx_sweep=None,
                 target_sweep=None, upa_sweep=None, colorjitter=False, tv_weight=0.0, nps_weight=0.0, nps_palette=None, train_crop=None,
                 train_crop_scale=0.9, scene_jitter=False, defocus_blur=False):
        """`attack_type`, `alpha`, `belta`, `target_action` are EXTENSIONS (the reference ships DDP for UADA only):
        "UPA" = UPA.py's reverse-direction loss + L1 grad clip, "TMA" = TMA.py's target-token CE, same data-parallel loop.
        `maskidx_sweep`, `target_sweep` (attack_type="TMA" only), `upa_sweep` (attack_type="UPA" only) are EXTENSIONS, at most one per run (sweep.KINDS):
        a list of maskidx lists / (maskidx list, target action value) pairs / (alpha, belta) pairs optimises one patch per entry in ONE loop — every
        group sees the same frames, draws and schedule, and group p ends where a standalone run with entry p in place of `maskidx` / `maskidx` and
        `target_action` / `alpha` and `belta` (then unused) and the same seed ends (DESIGN.md §maskidx sweep). None keeps the loop as it is.
        `colorjitter` is an EXTENSION (True or three strengths): every training step pastes a per-image brightness / contrast / saturation variant
        of the patch through the per-image forms of K1 / K2'; validation evaluates the patch as it is saved. Not available with a sweep.
        `tv_weight`, `nps_weight`, `nps_palette` are EXTENSIONS (AttackBase.set_patch_reg): the total-variation and non-printability terms of the
        patch; every rank adds their gradient before the exchange, so the rank mean carries it once. Not available with a sweep.
        `train_crop` / `train_crop_scale`, `scene_jitter`, `defocus_blur` are EXTENSIONS: the frame stages K9 / K10 / K11 of every training step, as
        RandomPatchTransform.set_frame_stages states them (the un-fused step). Not available with a sweep."""
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
        self.randomPatchTransform.colorjitter = colorjitter
        self.randomPatchTransform.set_frame_stages(train_crop, train_crop_scale, scene_jitter, defocus_blur)
        if tv_weight or nps_weight or nps_palette is not None:
            self.set_patch_reg(tv_weight, nps_weight, nps_palette)
        # at most one kind of sweep; the parameters are checked in KINDS' order, so a refusal of an earlier one comes first
        self.sweep_kind = self.sweep_groups = None
        given = dict(maskidx_sweep=maskidx_sweep, target_sweep=target_sweep, upa_sweep=upa_sweep)
        for kind in KINDS:
            groups = given[kind.param]
            if groups is not None:
                groups = check_sweep(self, kind, groups)
                self.sweep_kind, self.sweep_groups = kind, groups
            setattr(self, kind.param, groups)

    def setup(self, rank, world_size):
        vdist.init_process_group(device=self.device if self.device.type == "cuda" else None)
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)

    def cleanup(self):
        import torch.distributed as dist

        if dist.is_initialized():
            dist.destroy_process_group()

    def attack(self, rank, world_size):
        self.setup(rank, world_size)
        try:
            return self._attack(rank, world_size)
        finally:  # also when the run ends with NonFiniteAttackState: a process that leaves its group open can block at exit
            self.cleanup()

    def _attack(self, rank, world_size):
        if self.sweep_kind is not None:
            return self._attack_sweep(rank, world_size)
        dev = self.device
        patch = self._initial_patch(rank).requires_grad_(True)
        self.patch = patch
        optimizer = PatchOptimizer(patch, self.lr, "adamW", l1_clip=1e-3 if self.attack_type == "UPA" else 0.0)  # UPA.py:157
        scheduler = CosineWarmupSchedule(optimizer, self.warmup, int(self.num_iter), 0.5)
        if self.attack_type == "TMA":
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
                pix = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std, geometry=self.geometry,
                                                                          colorjitter=self.randomPatchTransform.colorjitter)
                total, sc, _ = self.model_loss(input_ids, attention_mask, pix, labels, self._loss_mode(), w=float(self.MSE_weights),
                                               alpha=self.alpha, beta=self.belta, full_ce=full_ce, read_scalars=full_ce)
                total.backward()  # K2 inside
                self.add_patch_reg(patch)  # K6: + the TV / NPS gradient on every rank, before the exchange (a no-op while both weights are 0)
                return lambda: sync.allreduce_step(patch.grad, sc, pick)

            s_sum, device_failure = self._inner_loop(optimizer, sync, world_size, step)
            self._end_outer(i, rank, world_size, scheduler, optimizer, s_sum, device_failure, f"{self.attack_type} (data parallel) outer iteration {i}")
        return patch

    def _initial_patch(self, rank):
        """UADA_ddp.py:140-141: the patch drawn on rank 0 (ONE torch.rand) and broadcast to every rank (C1)."""
        patch = (torch.rand if rank == 0 else torch.empty)(self.patch_size).to(self.device)
        vdist.broadcast_patch(patch, src=0)
        return patch

    # ---- sweeps: P patches in one loop ----
    def _attack_sweep(self, rank, world_size):
        """The loop above for the P patch groups of a sweep at once (fused path): one [P*bs] step per inner step (sweep_step) — K1 tile-major with one
        patch per group, ONE forward / backward, the kind's head with the segmented row map, K2' with a partial per image, the segmented epilogue
        (+ AdamW of every group); at world > 1, and for a kind that keeps K4 out of the epilogue, ONE all-reduce of [P gradients | P x 4 scalars]
        and the segmented K4. The RNG streams are consumed as by ONE standalone run: one patch init (every group starts from it), one transform draw
        per frame and step, shared by the groups. What differs between the kinds is stated in sweep.KINDS."""
        dev, kind, groups, P = self.device, self.sweep_kind, self.sweep_groups, len(self.sweep_groups)
        self.sweep_tags = [kind.tag(g) for g in groups]
        kind.prepare(self, groups)
        p0 = self._initial_patch(rank)  # drawn once: every group's standalone run draws this patch
        patches = p0.unsqueeze(0).repeat(P, *([1] * p0.dim())).contiguous().requires_grad_(True)
        self.patch = patches
        optimizer = SweepPatchOptimizer(patches, self.lr, "adamW", l1_clip=kind.l1_clip)  # per group
        scheduler = CosineWarmupSchedule(optimizer, self.warmup, int(self.num_iter), 0.5)
        sync = vdist.PatchGradSync(patches.numel(), 4 * P, dev)
        scalars = torch.zeros((P, 8), dtype=torch.float32, device=dev)
        fused_k4 = kind.k4_in_epilogue and world_size == 1  # nothing to exchange: AdamW runs inside the epilogue launch
        self.MSE_Distance_best = {t: 1000000 for t in self.sweep_tags}
        self.val_CE_loss, self.val_MSE_Distance, self.val_UAD = ({t: [] for t in self.sweep_tags} for _ in range(3))

        for i, data in enumerate(self.train_loader):
            if i == self.num_iter:
                break
            pixel_values, labels, attention_mask, input_ids = to_dev(data, dev)
            # the batch replicated to P groups ONCE per outer iteration (frames, ids, mask), the labels per group, ONE segmented row map
            img = self.randomPatchTransform.stage_images(pixel_values)
            img_all = img.repeat(P, 1, 1, 1).contiguous()
            ids_all = input_ids.repeat(P, 1).contiguous()
            am_all = attention_mask.repeat(P, 1).contiguous() if attention_mask is not None else None
            labels_all = torch.cat([self._sweep_group_labels(labels, g) for g in range(P)], dim=0)
            row_index = self.vla.label_row_index(labels_all)
            R = int(row_index.numel())
            if R == 0:
                raise ValueError(f"{kind.what}: no labelled position in the batch")
            if kind.row_limit is not None and not self._slice_head(R, None, self.vla.lm_head.weight):
                raise ValueError(f"{kind.what}: K3s does not take {R} labelled rows per rank here (limit {kind.row_limit} rows, bf16 head)")
            segmap = ops.LossRowMapSeg(labels_all, P)
            pack = self.vla.make_pack(am_all) if (hasattr(self.vla, "make_pack") and am_all is not None) else None

            def step(inner_loop):
                read = inner_loop == self.innerLoop - 1  # the step whose loss scalars the loop reads (UADA_ddp.py:214-221)
                self.sweep_step(img_all, patches, ids_all, row_index, segmap, pack, sync.buf, scalars, read,
                                optimizer.fused_update_args() if fused_k4 else None)
                return None if fused_k4 else sync.allreduce_packed  # (world 1: the exchange hands the message back as it is, K4 follows)

            s_sum, device_failure = self._inner_loop(optimizer, sync, world_size, step)
            self._end_outer(i, rank, world_size, scheduler, optimizer, s_sum, device_failure,
                            f"{kind.what} (data parallel) outer iteration {i}", tags=self.sweep_tags)
        return patches

    def sweep_step(self, img_all, patches, input_ids, row_index, segmap, pack, msg, scalars, read, update=None, groups=None):
        """One inner step of a sweep up to the exchange: K1 (one draw per frame, every group) -> body over P*bs images -> the kind's head over the
        rows of all groups -> backward, K2' (a partial per image) -> ONE segmented epilogue: msg = [P gradients | P x 4 scalars] on the step whose
        scalars are `read`, a zero tail on the others (`scalars` [P,8] is then left as it is); `update` = AdamW of every group inside that launch.
        Returns the full-vocabulary predictions on the `read` step, else None. `groups`: the attacker's `sweep_groups` when None. Per kind:
          maskidx — K3s with the segmented map (each row normalised by its group's count; K3h behind it when `read`), the epilogue folds K3's
            statistics per group: tail {CE, w^2*MSE, UAD, total}, `scalars` [P,8] written;
          target — ONE hipBLASLt head, K3 in LOSS_CE mode (each row normalised by its group's row count, every group folded on its own), ONE
            dh = g @ W; K3 made the scalars final before the backward, so the epilogue passes them through: tail {CE, 0, UAD, total};
          UPA — that head with K3 in LOSS_UPA mode (every group's batch means and (alpha, belta) its own), ONE dh = g_slice @ W[31744:32000]: tail
            {CE, w^2*MSE, UAD, total}. K4 is never fused (`update` None): the caller runs the segmented K4 with the L1 clip on the exchanged message."""
        sink = {}
        P = int(patches.shape[0])
        pe = self.randomPatchTransform.apply_sweep_batch(img_all, patches, self.mean, self.std, self.geometry, sink)
        h = self.vla.hidden_rows(input_ids, None, row_index, patch_embeds=pe, pack=pack)
        return self.sweep_kind.head(self, h, segmap, self.sweep_groups if groups is None else groups, P, read, sink, msg, scalars, update)

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
            logs[0].update(self.patch_reg_log("TRAIN"))
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

    def _sweep_group_labels(self, labels, g):
        """Group g's labels of a sweep (a new tensor): masked with its maskidx, its TMA target labels, or left unmasked — the kind's."""
        return self.sweep_kind.group_labels(self, labels, g)

    def validate_sweep(self, i, patches, rank):
        """validate() per group: every validation batch is drawn ONCE (the RNG consumption of one standalone pass) and evaluated with each group's
        patch and labels; per group the averages, the AVG all-reduces, best-patch selection and the files under save_dir/<group tag>/."""
        kind = self.sweep_kind
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
                    _, sc, _ = self.model_loss(input_ids, attention_mask, modified, lab, kind.loss_mode, w=float(self.MSE_weights), need_grad=False,
                                               **kind.loss_args(self.sweep_groups[g]))
                    rbs[g].add(sc)
                    last_images[g] = modified
        self.last_val_log = {}
        for g, tag in enumerate(self.sweep_tags):
            self.last_val_log[tag] = self._val_record(i, rank, rbs[g].read()[0], kind.select_metric, patches[g], last_images[g], tag)

    def _loss_mode(self):
        return {"UADA": ops.LOSS_UADA_DDP, "UPA": ops.LOSS_UPA, "TMA": ops.LOSS_CE}[self.attack_type]

    def _prepare_labels(self, labels):
        if self.attack_type == "UADA":
            return self.mask_labels(labels, self.maskidx)
        if self.attack_type == "TMA":
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
        if tag is None:
            log.update(self.patch_reg_log("VAL", patch))
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
