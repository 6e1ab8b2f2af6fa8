"""Shared machinery of the UADA / UPA / TMA attack loops (the hot inner step and the validation/checkpoint side).

One inner step = K1 (paste/warp, HIP) -> model forward/backward (PyTorch-ROCm) -> K3 (loss fwd+bwd, HIP) ->
K2 (patch-grad gather, HIP, inside autograd backward) -> [RCCL all-reduce of the 30 KB patch gradient] -> K4 (update, HIP).
Nothing in the step synchronises with the host: the loss scalars of all innerLoop steps of an outer iteration are kept
in a device buffer and read back once (the reference calls `.item()` 4-5 times per inner step, UADA.py:149-154).
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch

from .. import _lib, ops, palette as _palette
from ..action_tokenizer import ActionTokenizer
from ..constants import MEAN0, MEAN1, STD0, STD1
from ..labels import mask_labels as _mask_labels
from ..optim import CosineWarmupSchedule, PatchOptimizer
from ..transform import RandomPatchTransform

try:  # optional, exactly like a reference run with --wandb_project false
    import wandb  # type: ignore
except Exception:  # pragma: no cover
    wandb = None


class NonFiniteAttackState(RuntimeError):
    """The attack state (loss scalars, optimiser moments, patch) stopped being finite, or a kernel reported a device-side failure: raised
    before anything is written to disk. The reference would silently keep optimising and save the patch (UADA.py:257-275)."""


def wandb_enabled(args) -> bool:
    return wandb is not None and args is not None and getattr(args, "wandb_project", "false") != "false"


class ValReadback:
    """What a validation pass reads back from the device — the loss scalars of every batch and, where the metrics need them, the prediction
    and label maps — kept ON the device while the batches are enqueued and fetched ONCE at the end (one [batches, 8] copy + one copy of
    the concatenated maps). The reference calls `.item()` / `.cpu()` several times per batch (UADA.py:229-246); round 5 still read
    `scalars.cpu()` once per batch, i.e. the host waited for every forward before it enqueued the next one.
    VAA_VAL_SYNC_EVERY_BATCH=1 restores the per-batch read-back (A/B measurements). The accumulation below runs in the order of the
    batches on the host, in the reference's precision: the same numbers as the per-batch form."""

    def __init__(self, batches: int, device):
        self.scal = torch.zeros((max(batches, 1), 8), dtype=torch.float32, device=device)
        self.k = 0
        self.maps = []  # per batch: (pred i32 [B,L-1] device, labels[:,1:] i64 device) or None
        self.sync_every = os.environ.get("VAA_VAL_SYNC_EVERY_BATCH", "0") == "1"

    def add(self, scalars, pred=None, labels=None):
        self.scal[self.k].copy_(scalars)
        self.maps.append((pred, labels[:, 1:]) if pred is not None else None)
        self.k += 1
        if self.sync_every:
            self.scal[self.k - 1].cpu()

    def read(self):
        """-> (scalars float64 [batches, 8] on the host, [(pred, gt) numpy int arrays per batch | None])."""
        host = self.scal[: self.k].cpu().numpy().astype(np.float64)
        have = [m for m in self.maps if m is not None]
        out = [None] * len(self.maps)
        if have:
            flat = torch.cat([m[0].reshape(-1).to(torch.int64) for m in have] + [m[1].reshape(-1) for m in have]).cpu().numpy()
            sizes = [int(m[0].numel()) for m in have]
            off, off2, j = 0, sum(sizes), 0
            for i, m in enumerate(self.maps):
                if m is None:
                    continue
                n = sizes[j]
                out[i] = (flat[off : off + n].reshape(tuple(m[0].shape)), flat[off2 : off2 + n].reshape(tuple(m[1].shape)))
                off, off2, j = off + n, off2 + n, j + 1
        return host, out


class AttackBase:
    """State every OpenVLAAttacker variant shares (UADA.py:34-74, UPA.py:31-71, TMA.py:29-64)."""

    val_batches = 1000  # UADA.py:202; subclasses override (UPA/TMA: 100)

    def __init__(self, vla, processor=None, save_dir: str = "", optimizer: str = "pgd", resize_patch: bool = False):
        self.vla = vla.eval()
        self.processor = processor
        tok = getattr(processor, "tokenizer", None)
        self.action_tokenizer = ActionTokenizer(tok)
        self.base_tokenizer = tok
        self.predict_stop_token = True
        self.pad_token_id = 32000
        self.model_max_length = 2048
        self.loss_buffer = []
        self.save_dir = save_dir
        self.device = torch.device(getattr(vla, "device", "cuda"))
        self.randomPatchTransform = RandomPatchTransform(self.device, resize_patch)
        if os.environ.get("VAA_FUSED_EMBED_GRAD", "1") != "0" and hasattr(vla, "forward_rows") and hasattr(vla, "patch_embed_params"):
            # a model that exposes its patch-embed parameters is handed patch-embed OUTPUTS in training steps and K2' never
            # builds the dense pixel gradient (the embed backward runs on the ~20 flagged tiles under the patch only; per-image patches of
            # resize_patch=True included). A black-box model (no patch_embed_params) and VAA_FUSED_EMBED_GRAD=0 keep the pixel_values
            # boundary of the reference.
            self.randomPatchTransform.embed_with = vla
        self.mean = [torch.tensor(MEAN0), torch.tensor(MEAN1)]
        self.std = [torch.tensor(STD0), torch.tensor(STD1)]
        self.optimizer = optimizer
        self.use_rows = hasattr(vla, "forward_rows")  # LM head on labelled rows only (no [B,S,32064] logits)
        self.n_img_tokens = vla.vision_backbone.featurizer.patch_embed.num_patches
        self.tv_weight = self.nps_weight = 0.0  # the patch regulariser (K6) is off until set_patch_reg turns it on
        self._reg_palette_host = self._reg_palette = self._reg_part = None

    # ---- smoothness / printability terms of the patch (K6: total variation + non-printability score) ----
    def set_patch_reg(self, tv_weight: float = 0.0, nps_weight: float = 0.0, palette=None):
        """An EXTENSION (the reference has no such term): every training step adds the gradient of tv_weight*TV(patch) + nps_weight*NPS(patch, palette)
        — always minimised — to the patch gradient (add_patch_reg). `palette`: [K,3] RGB in [0,1], K <= 64; None = the built-in 27-colour grid
        (palette.default_palette: a placeholder for a measured printer palette). Both weights 0 (the default) leaves every step as it is."""
        tv_weight, nps_weight = float(tv_weight), float(nps_weight)
        if not (np.isfinite(tv_weight) and np.isfinite(nps_weight)) or tv_weight < 0 or nps_weight < 0:
            raise ValueError(f"tv_weight / nps_weight must be finite and >= 0, got {tv_weight}, {nps_weight}")
        self.tv_weight, self.nps_weight = tv_weight, nps_weight
        self._reg_palette_host = _palette.check_palette(palette) if palette is not None else _palette.default_palette()
        self._reg_palette = self._reg_part = None

    @property
    def patch_reg_on(self) -> bool:
        return self.tv_weight != 0.0 or self.nps_weight != 0.0

    def _reg_palette_on(self, device):
        if self._reg_palette is None or self._reg_palette.device != device:
            self._reg_palette = torch.from_numpy(self._reg_palette_host).to(device)
        return self._reg_palette

    def add_patch_reg(self, patch, scale: float = 1.0):
        """Right after `total.backward()`: patch.grad += scale * d(tv_weight*TV + nps_weight*NPS)/d patch, in place, ONE launch (in front of UPA's L1
        clip, the PGD sign and the data-parallel exchange); the launch's partial sums of the two values are kept for the log (patch_reg_log).
        Both weights 0: nothing happens — no launch, no allocation."""
        if not self.patch_reg_on:
            return
        if patch.grad is None:
            raise ValueError("add_patch_reg: patch.grad is not materialised (the fused single-patch paths are off while a weight is non-zero)")
        _, self._reg_part = ops.patch_reg_grad(patch.detach(), self._reg_palette_on(patch.device), self.tv_weight * scale, self.nps_weight * scale,
                                               grad=patch.grad, accumulate=True, part=self._reg_part)

    def patch_reg_log(self, prefix: str, patch=None) -> dict:
        """{prefix_tv: TV, prefix_nps: NPS} for a log, {} while the regulariser is off. `patch` None: the values of the last add_patch_reg, folded
        from the partial sums that launch left (call it behind the outer iteration's read-back); a patch: the values-only launch on it."""
        if not self.patch_reg_on:
            return {}
        if patch is not None:
            _, part = ops.patch_reg_grad(patch.detach(), self._reg_palette_on(patch.device), self.tv_weight, self.nps_weight, want_grad=False)
        else:
            part, patch = self._reg_part, self.patch
        if part is None:
            return {}
        tv, nps = (float(v) for v in torch.stack(ops.patch_reg_values(part, patch.numel())).cpu())
        return {f"{prefix}_patch_tv": tv, f"{prefix}_patch_nps": nps}

    # ---- the model + loss leg of a step ----
    def model_loss(self, input_ids, attention_mask, pix, labels, mode, w=5.0, alpha=0.8, beta=0.2, scale=1.0, need_grad=True, full_ce=True, read_scalars=True):
        """Returns (total [autograd scalar or None], scalars f32[8] device, pred i32 [B,L-1] device).

        `full_ce=False` (slice modes — UADA_DDP, UPA — on a model that exposes its hidden rows): the caller will not read this step's
        full-vocabulary CE (scalars[1]) nor the full argmax (`pred`): the reference reads them on the LAST inner step of an outer iteration
        only (UADA_ddp.py:214-221) and never in UPA's reverse-direction mode (UPA.py:145-186). The step then runs K3s alone — 2.1 MB of head
        weights instead of the 263 MB stream; scalars[1] = 0, pred = -1. The gradient path is the same on every step either way.
        `read_scalars=False` (same models and modes, training steps): the caller reads NONE of this step's loss scalars — the loops read the
        scalars of the last inner step of an outer iteration only (UADA_ddp.py:214-221, UPA.py:171-186) — so not even the slice statistics are
        folded: scalars = 0 (implies full_ce=False).

        `pred` is the argmax over the WHOLE vocabulary at every labelled position (-1 elsewhere), i.e. the reference's
        `action_logits.argmax(dim=2)` (UADA.py:165-167, TMA.py:148-149) that its relative-distance / L1 / ASR metrics and the
        best-patch selection read; the action-slice argmax of UADA.py:395 only feeds UAD, which K3 reports in scalars[7]."""
        if self.use_rows:
            pack = self._rows_cache(labels, attention_mask)
            pe = pix if isinstance(pix, ops.PatchEmbeds) else None  # patched batch handed over as patch-embed outputs (pixel gradient never built)
            if need_grad and hasattr(self.vla, "hidden_rows"):
                # LM head + loss on the labelled rows: the head's backward contracts over the 256 action
                # columns when the loss lives there (UADA_DDP, UPA)
                h = self.vla.hidden_rows(input_ids, None if pe is not None else pix, self._row_index, patch_embeds=pe, pack=pack)
                W = self.vla.lm_head.weight
                # ... and with the LM head FUSED into K3's statistics there (K3h: no [R,V] logits at all); UADA's 1/CE and TMA's CE gradients need
                # every logit and keep the GEMM head
                if mode in ops.SLICE_MODES and self._slice_head(int(h.shape[0]), h, W):
                    # K3s: slice-only head + statistics + gradient + head backward in ONE launch, on every step; K3h's 263 MB stream only
                    # behind it on the steps whose CE / full argmax is read
                    total, scalars, _, pred_full = ops.HeadSliceLoss.apply(h, W, self._row_map, mode, w, alpha, beta, scale, bool(full_ce), bool(read_scalars))
                    return total, scalars, pred_full
                head = ops.HeadLossRowsFused if (mode in ops.SLICE_MODES and self._fused_head(int(h.shape[0]), h, W)) else ops.HeadLossRows
                total, scalars, _, pred_full = head.apply(h, W, self._row_map, mode, w, alpha, beta, scale)
                return total, scalars, pred_full
            if not need_grad and hasattr(self.vla, "hidden_rows") and self._row_count > 0 and self._fused_head(self._row_count, None, self.vla.lm_head.weight):
                # evaluation only (validation passes, every mode): head + statistics + fold without logits in memory when K3h covers the shape
                h = self.vla.hidden_rows(input_ids, None if pe is not None else pix, self._row_index, patch_embeds=pe, pack=pack)
                if not full_ce and mode in ops.SLICE_MODES and self._slice_head(self._row_count, h, self.vla.lm_head.weight):
                    o = ops.head_slice_fwd_bwd(h.detach().contiguous(), self.vla.lm_head.weight, self._row_map, mode, w, alpha, beta, scale, want_dh=False)
                    return None, o["scalars"], o["pred_full"]
                if h.dtype == torch.bfloat16:
                    scalars, _, pred_full, _ = ops.head_loss_rows_fwd_bwd(h.detach().contiguous(), self.vla.lm_head.weight, self._row_map, mode, w, alpha, beta,
                                                                          scale, want_grad=False)
                    return None, scalars, pred_full
                logits = self.vla.lm_head(h)
                scalars, _, pred_full, _ = ops.loss_rows_fwd_bwd(logits.detach().contiguous(), self._row_map, mode, w, alpha, beta, scale, want_grad=False)
                return None, scalars, pred_full
            logits = self.vla.forward_rows(input_ids, None if pe is not None else pix, labels, self._row_index, patch_embeds=pe, pack=pack)
            if need_grad:
                total, scalars, _, pred_full = ops.DiscrepancyLossRows.apply(logits.contiguous(), self._row_map, mode, w, alpha, beta, scale)
                return total, scalars, pred_full
            scalars, _, pred_full, _ = ops.loss_rows_fwd_bwd(logits.detach().contiguous(), self._row_map, mode, w, alpha, beta, scale, want_grad=False)
            return None, scalars, pred_full
        out = self.vla(input_ids=input_ids, attention_mask=attention_mask, pixel_values=pix, labels=None)
        logits = out.logits
        if need_grad:
            total, scalars, _, pred_full = ops.DiscrepancyLoss.apply(logits.contiguous(), labels, mode, w, alpha, beta, scale, ops.LAYOUT_FULL)
            return total, scalars, pred_full
        scalars, _, _, pred_full = ops.loss_fwd_bwd(logits.detach().contiguous(), labels, mode, w, alpha, beta, scale, ops.LAYOUT_FULL,
                                                    want_grad=False, want_pred_full=True)
        return None, scalars, pred_full

    def _rows_cache(self, labels, attention_mask):
        """labels are fixed during an outer iteration: the row index (one host sync) and the device row map of K3 are cached per
        tensor OBJECT; the cache holds a reference, so identity cannot be recycled by the allocator, and in-place edits bump _version.
        Returns the sequence pack (or None)."""
        if getattr(self, "_row_ref", None) is not labels or self._row_ver != labels._version:
            self._row_ref, self._row_ver, self._row_index = labels, labels._version, self.vla.label_row_index(labels)
            self._row_map = ops.LossRowMap(labels)
            self._row_count = int(self._row_index.numel())
        pack = None
        if hasattr(self.vla, "make_pack") and attention_mask is not None:  # drop the padding rows (cached like the row index)
            if getattr(self, "_pack_ref", None) is not attention_mask or self._pack_ver != attention_mask._version:
                self._pack_ref, self._pack_ver, self._pack = attention_mask, attention_mask._version, self.vla.make_pack(attention_mask)
            pack = self._pack
        return pack

    # ---- the data-parallel UADA step with the fused epilogue ----
    def fused_ddp_available(self) -> bool:
        """K1 (tile-major) -> model -> K3 statistics (+ gradient slice) -> K2' tiles + scatter -> ONE epilogue launch (K2's final sum, K3's
        fold, the DDP message) needs a model that exposes its patch-embed weights and its hidden rows, and one patch per batch (no resize_patch,
        no colorjitter: their per-image patches go through the per-image forms of K1 / K2'), and no patch regulariser (K6 adds to a materialised
        patch.grad, which this path never builds), and no train_crop, scene_jitter or defocus_blur (K2' cannot take the gradient behind K9 / K10 /
        K11: the planar K1 -> K11 -> K9 -> K10 path runs)."""
        t = self.randomPatchTransform
        return (os.environ.get("VAA_FUSED_EPILOGUE", "1") != "0" and self.use_rows and hasattr(self.vla, "hidden_rows")
                and t.embed_with is not None and not t.resize_patch and not t.colorjitter and not t.frame_stages_on() and not self.patch_reg_on)

    @staticmethod
    def _fused_head(R, h, W) -> bool:
        """LM head fused with K3's statistics (vaa_head_loss_rows_stats) for this shape? Whenever the kernel covers it (bf16, up to 128 labelled
        rows = bs 64 with maskidx=[0]): one pass over the 263 MB head weight, the [R,V] logits are never written. In the step, same box:
        bs = 8 (16 rows) 45 us (5.8 TB/s) + 7 us fold against 64 + 10 us for the hipBLASLt GEMM + K3 statistics; bs = 32: 47 + 8 against
        62 + 10; bs = 64 (128 rows, where a CU's line rate, not HBM, bounds the kernel): 54 + 8 against 55-57 + 11
        (profiles/r04_head_fused.txt). VAA_FUSED_HEAD=0 restores the GEMM path."""
        mode = os.environ.get("VAA_FUSED_HEAD", "auto")
        if mode == "0" or (h is not None and h.dtype != torch.bfloat16) or W.dtype != torch.bfloat16 or not W.is_cuda:
            return False
        return ops.head_loss_rows_applies(R, int(W.shape[1]), int(W.shape[0]))

    @staticmethod
    def _slice_head(R, h, W) -> bool:
        """K3s (vaa_head_slice_fwd_bwd) for this shape? bf16, up to 128 labelled rows, D a multiple of 64 up to 4096. VAA_HEAD_EVERY_STEP=1
        restores the round-5 behaviour (K3h + finish + the 256-column GEMM on every step), VAA_FUSED_HEAD=0 the GEMM head."""
        if os.environ.get("VAA_HEAD_EVERY_STEP", "0") == "1" or os.environ.get("VAA_FUSED_HEAD", "auto") == "0":
            return False
        if (h is not None and h.dtype != torch.bfloat16) or W.dtype != torch.bfloat16 or not W.is_cuda:
            return False
        return ops.head_slice_applies(R, int(W.shape[1]), int(W.shape[0]))

    def fused_ddp_step(self, pixel_values, patch, input_ids, attention_mask, labels, geometry, w, msg, scalars, optimizer=None, full_ce=True):
        """The UADA_ddp inner step (UADA_ddp.py:189-206) up to the gradient exchange, six hand-written launches around the model:
        K1 -> [ViTs, Llama, LM head on the labelled rows] -> K3 statistics + gradient slice -> [head / model backward] -> K2' tile GEMM ->
        scatter -> epilogue. On return `msg` (f32 [3*ph*pw + 4]) holds [patch gradient | CE, w^2*MSE, UAD, total] of THIS rank, ready for
        one all-reduce, and `scalars` (f32[8]) the loss scalars; returns the full-vocabulary predictions [B,L-1] (i32, device) — all three only on
        the steps the caller marks `full_ce` (the steps whose scalars are read; else the tail / `scalars` are left as they were and None is returned).
        Nothing is synchronised; patch.grad is not touched. `optimizer` (single-GPU run, no L1 clip): K4 is applied by the epilogue launch
        itself — five launches per step, the caller then calls neither the all-reduce nor optimizer.step()."""
        pack = self._rows_cache(labels, attention_mask)
        if self._row_count == 0:
            raise ValueError("fused_ddp_step: no labelled position in the batch")
        sink = {}
        pe = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std, geometry=geometry, grad_sink=sink)
        h = self.vla.hidden_rows(input_ids, None, self._row_index, patch_embeds=pe, pack=pack)
        W = self.vla.lm_head.weight
        R = int(h.shape[0])
        if self._slice_head(R, h, W):
            return self.slice_step_tail(h, self._row_map, w, int(W.shape[0]), sink, msg, scalars, full_ce,
                                        optimizer.fused_update_args() if optimizer is not None else None)
        gsl = torch.empty((R, ops.N_ACTION), dtype=h.dtype, device=h.device)
        if self._fused_head(R, h, W):
            # SURVEY.md 8f-2 as the survey wrote it: LM head + K3 statistics in ONE weight-streaming kernel — the [R,V] logits are never written
            ws = ops.head_loss_rows_stats(h.detach().contiguous(), W, self._row_map, ops.LOSS_UADA_DDP, w, grad=gsl)
        else:
            logits = torch.nn.functional.linear(h.detach(), W)  # [R,V]: the LM head on the labelled rows through hipBLASLt
            ws = ops.loss_rows_stats(logits, self._row_map, ops.LOSS_UADA_DDP, w, grad=gsl)  # K3: statistics + d loss / d action logits
        h.backward(gsl @ W[ops.ACTION_LO : ops.ACTION_LO + ops.N_ACTION])                     # head backward over 256 columns, model backward, K2'
        _, pred_full = ops.step_epilogue(sink["partials"], msg, scalars, rowmap=self._row_map, R=R, V=int(W.shape[0]),
                                         mode=ops.LOSS_UADA_DDP, w=w, loss_ws=ws,
                                         update=optimizer.fused_update_args() if optimizer is not None else None)
        return pred_full

    def slice_step_tail(self, h, rowmap, w, V, sink, msg, scalars, full_ce, update, P=None):
        """The data-parallel UADA step after the model forward, on the K3s head: shared by fused_ddp_step (P None: vaa_step_epilogue) and the
        maskidx sweep's sweep_step (P groups, a segmented `rowmap`: vaa_step_epilogue_seg). K3s: slice logits -> statistics -> gradient slice ->
        d total / d hidden in ONE launch (2.1 MB of head weights); the full-vocabulary stream (K3h, 263 MB) runs behind it only on the steps whose
        CE / full argmax is read (`full_ce`: UADA_ddp.py:214-221); the backward, which leaves K2''s partial tiles in `sink`; then ONE epilogue launch
        (+ K4 when `update` is given)."""
        W = self.vla.lm_head.weight
        hd = h.detach().contiguous()
        o = ops.head_slice_fwd_bwd(hd, W, rowmap, ops.LOSS_UADA_DDP, w, want_dh=True, want_scalars=False)
        ws = ops.head_loss_rows_stats(hd, W, rowmap, ops.LOSS_UADA_DDP, w) if full_ce else None
        h.backward(o["dh"])
        partials = sink["partials"]
        epilogue, groups = (ops.step_epilogue, ()) if P is None else (ops.step_epilogue_seg, (P,))
        if not full_ce:
            # nobody reads this step's loss scalars (the loop reads those of the LAST inner step of an outer iteration: UADA_ddp.py:214-221):
            # the epilogue in its pass-through form — K2's final sum (+ K4), no fold; `scalars` keep the last read step's values
            epilogue(partials, msg, scalars, *groups, update=update)
            return None
        _, pred_full = epilogue(partials, msg, scalars, *groups, rowmap=rowmap, R=int(hd.shape[0]), V=V, mode=ops.LOSS_UADA_DDP, w=w, loss_ws=ws,
                                update=update)
        return pred_full

    # ---- single-GPU loops: K2's final sum + K4 as one launch after the backward ----
    def fused_update_sink(self, optimizer):
        """A gradient sink ({}) for `apply_random_patch_batch(grad_sink=...)` when the step can end with ONE launch that adds K2''s partial tiles
        and applies the optimiser to every gradient element as it is produced (`fused_update`), else None: needs one patch per batch and no
        L1 clip (UPA's clip needs the whole gradient's norm first). Works behind both boundaries: K2' (a model that exposes its patch-embed
        weights) and K2 on a black-box model's pixel gradient."""
        t = self.randomPatchTransform
        ok = (os.environ.get("VAA_FUSED_EPILOGUE", "1") != "0" and not t.resize_patch and not t.colorjitter and not t.frame_stages_on()
              and not optimizer.l1_clip and not self.patch_reg_on)  # (K6 adds to patch.grad, which the fused update never materialises)
        return {} if ok else None

    def fused_update(self, sink, patch, optimizer, scalars):
        """After `total.backward()` of a step whose transform was given `sink`: vaa_step_epilogue_update in its pass-through form (the loss
        scalars are final already) — patch / m / v get the bits `optimizer.step()` would write; patch.grad stays None."""
        n = patch.numel()
        msg = getattr(self, "_epi_msg", None)
        if msg is None or msg.numel() != n + 4 or msg.device != patch.device:
            msg = self._epi_msg = torch.zeros(n + 4, dtype=torch.float32, device=patch.device)
        ops.step_epilogue(sink["partials"], msg, scalars, update=optimizer.fused_update_args())

    # ---- fail loud, never NaN: once per outer iteration, behind the read-back that synchronises anyway ----
    def assert_finite_state(self, patch, optimizer, host_scalars, where: str, all_ranks: bool = False, device_failure=None):
        """`host_scalars`: the loss scalars of the outer iteration's inner steps, already on the host (their read-back was the sync).
        AdamW's m / v are the sticky witnesses of any non-finite gradient of ANY inner step (a NaN that entered them never leaves, while the
        clamp turns the patch itself into a finite 0), the library's failure word covers kernels that had to give up (vaa_async_error: a
        per-PROCESS word). `all_ranks` (the data-parallel loop): the verdict is all-reduced (MIN) before anyone raises, so that every rank
        leaves the loop together instead of one rank raising while the others wait in the next all-reduce until the RCCL timeout."""
        # `device_failure`: a failure this rank's inner loop already caught (and polled) — the data-parallel loop keeps its collectives going and
        # hands it over here, so that the verdict below is all-reduced instead of one rank raising alone
        try:
            ops.async_error_check()
        except _lib.VaaError as e:  # reported like every other non-finite state (and cleared: the poll is the consumer of the sticky word)
            device_failure = device_failure or str(e)
        ok_dev = torch.isfinite(patch.detach()).all()
        if getattr(optimizer, "m", None) is not None:
            ok_dev = ok_dev & torch.isfinite(optimizer.m).all() & torch.isfinite(optimizer.v).all()
        stats = getattr(optimizer, "last_stats", None)
        if stats is not None:
            ok_dev = ok_dev & torch.isfinite(stats).all()
        ok_host = bool(np.isfinite(np.asarray(host_scalars, dtype=np.float64)).all())
        ok_local = ok_host and bool(ok_dev) and device_failure is None
        ok = ok_local
        if all_ranks:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                flag = torch.tensor([1.0 if ok_local else 0.0], dtype=torch.float32, device=patch.device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = bool(flag.item() > 0.5)
        if not ok:
            raise NonFiniteAttackState(f"{where}: non-finite attack state (loss scalars finite: {ok_host}; patch / moments / gradient statistics "
                                       f"finite: {bool(ok_dev)}; device-side failure: {device_failure or 'none'}"
                                       + ("" if ok_local else "; detected on THIS rank") + (" — raised on every rank" if all_ranks else "")
                                       + ") — nothing was saved for this iteration")

    # ---- metrics (host, once per outer iteration) ----
    def decode_pred_gt(self, pred: torch.Tensor, labels: torch.Tensor):
        """Continuous predicted / ground-truth actions of the action rows, (b,k) order (UADA.py:165-175)."""
        return self.decode_pred_gt_np(pred.detach().cpu().numpy(), labels[:, 1:].detach().cpu().numpy())

    def decode_pred_gt_np(self, p: np.ndarray, gt: np.ndarray):
        """decode_pred_gt on maps that are already on the host (ValReadback.read): p [B,L-1] predictions, gt = labels[:, 1:]."""
        m = gt > self.action_tokenizer.action_token_begin_idx
        return (torch.tensor(self.action_tokenizer.decode_token_ids_to_actions(p[m])),
                torch.tensor(self.action_tokenizer.decode_token_ids_to_actions(gt[m])))

    def calculate_relative_distance(self, pred, gt, maskidx, relative_distance):
        """UADA.py:354-369."""
        pred = pred.clone().view(pred.shape[0] // len(maskidx), len(maskidx))
        gt = gt.clone().view(gt.shape[0] // len(maskidx), len(maskidx))
        for i1 in range(pred.shape[0]):
            for i2 in range(pred.shape[1]):
                anchor = gt[i1, i2]
                max_boundary = max(1 - anchor, anchor - (-1))
                relative_distance[f"{str(maskidx[i2])}"].append((abs(pred[i1, i2] - anchor) / max_boundary).item())
        return relative_distance

    def filter_train(self, data):
        """UADA.py:308-339 — optional gripper filtering; keeps the reference's thresholds."""
        import random

        pixel_values = data["pixel_values"]
        labels = data["labels"].to(self.device)
        attention_mask = data["attention_mask"].to(self.device)
        input_ids = data["input_ids"].to(self.device)
        masked = labels[labels > self.action_tokenizer.action_token_begin_idx]
        masked = masked.view(masked.shape[0] // 7, 7)
        one_index = [i for i in range(masked.shape[0]) if masked[i, 6] == 31744]
        chosen = None
        if 1 < len(one_index) < 8:
            chosen = one_index
        elif len(one_index) > 8:
            chosen = random.sample(one_index, k=8)
        if chosen is not None:
            labels, attention_mask, input_ids = labels[chosen, :], attention_mask[chosen, :], input_ids[chosen, :]
            pixel_values = [pixel_values[i] for i in chosen]
        return labels, attention_mask, input_ids, pixel_values

    # ---- outputs (a-12) ----
    def save_patch(self, patch: torch.Tensor, sub: str) -> str:
        """`torch.save(patch.detach().cpu(), <save_dir>/<sub>/patch.pt)` — plain fp32 [3,ph,pw] CPU tensor (UADA.py:257-275)."""
        d = os.path.join(self.save_dir, sub)
        host = patch.detach().float().cpu().contiguous().clone()
        if not bool(torch.isfinite(host).all()):  # belt and braces behind assert_finite_state
            raise NonFiniteAttackState(f"save_patch({sub!r}): the patch holds non-finite values")
        os.makedirs(d, exist_ok=True)
        torch.save(host, os.path.join(d, "patch.pt"))
        return d

    def save_val_images(self, modified_images: torch.Tensor, d: str):
        """De-normalised first-3-channel frames as PNG (UADA.py:260-268): ToPILImage == mul(255).byte()."""
        from PIL import Image

        path = os.path.join(d, "val_related_data")
        os.makedirs(path, exist_ok=True)
        imgs = self.randomPatchTransform.denormalize(modified_images[:, 0:3].detach().float().cpu(), self.mean[0], self.std[0])
        pil = []
        for o in range(imgs.shape[0]):
            arr = imgs[o].mul(255).byte().permute(1, 2, 0).numpy()
            im = Image.fromarray(arr)
            im.save(os.path.join(path, f"{o}.png"))
            pil.append(im)
        return path, pil

    def plot_loss(self):
        """UADA.py:76-91 (seaborn theme dropped; the curve is identical)."""
        try:
            import matplotlib

            matplotlib.use("Agg")
            import matplotlib.pyplot as plt

            plt.plot(list(range(len(self.loss_buffer))), self.loss_buffer, label="Target Loss")
            plt.title("Loss Plot")
            plt.xlabel("Iters")
            plt.ylabel("Loss")
            plt.legend(loc="best")
            plt.savefig("%s/loss_curve.png" % (self.save_dir))
            plt.clf()
        except Exception:  # plotting is best effort
            pass
        torch.save(self.loss_buffer, "%s/loss" % (self.save_dir))

    def dump_lists(self, names):
        """`names`: attributes pickled under their own name, or (file name, attribute) pairs where the reference names the file differently."""
        for fname, attr in ((n, n) if isinstance(n, str) else n for n in names):
            with open(os.path.join(self.save_dir, f"{fname}.pkl"), "wb") as f:
                pickle.dump(getattr(self, attr), f)

    # ---- the single-GPU drivers (attack/uada.py, upa.py, tma.py): what they share; DESIGN.md §1 lists the hooks and what differs ----
    accumulates = True  # the driver's inner step takes `do_step` (UADA's runs its optimiser on every step: False there)

    def mask_labels(self, labels, maskidx):
        return _mask_labels(labels, maskidx)

    def begin_run(self, patch_size, lr, l1_clip, warmup, num_iter, accumulate_steps, innerLoop, colorjitter, train_crop, train_crop_scale, scene_jitter,
                  defocus_blur):
        """-> (patch, optimizer, scheduler | None, scalar buffer [max(innerLoop, 1), 10]). The patch is the FIRST draw a run takes from torch's CPU
        generator (then H2D: same values as UADA.py:104); `l1_clip` applies with AdamW only (UPA.py:157).
        The keywords of `patchattack_unconstrained` the reference does not have are EXTENSIONS, all off by default:
        colorjitter (True or three strengths): every training step pastes a per-image brightness / contrast / saturation variant of the patch;
        validation evaluates the patch as it is saved (in the reference's TMA the keyword exists and is dead, Appendix A-D3).
        train_crop / train_crop_scale, scene_jitter, defocus_blur: the frame stages K9 / K10 / K11 of every training step, as
        RandomPatchTransform.set_frame_stages states them."""
        self.randomPatchTransform.colorjitter = colorjitter
        self.randomPatchTransform.set_frame_stages(train_crop, train_crop_scale, scene_jitter, defocus_blur)
        patch = torch.rand(patch_size).to(self.device)
        patch.requires_grad_(True)
        self.patch = patch
        adam = self.optimizer == "adamW"
        optimizer = PatchOptimizer(patch, lr, "adamW" if adam else "pgd", l1_clip=l1_clip if adam else 0.0)
        scheduler = CosineWarmupSchedule(optimizer, warmup, int(num_iter / accumulate_steps), 0.5) if adam else None
        return patch, optimizer, scheduler, torch.zeros((max(innerLoop, 1), 10), dtype=torch.float32, device=self.device)

    def fetch_batch(self, data, maskidx, filterGripTrainTo1):
        """-> (pixel_values, labels, attention_mask, input_ids) on the device; the gripper filter only for maskidx == [6] (UADA.py:120-127)."""
        if gripper_only(maskidx) and filterGripTrainTo1:
            labels, attention_mask, input_ids, pixel_values = self.filter_train(data)
            return pixel_values, labels, attention_mask, input_ids
        return to_dev(data, self.device)

    def run_outer_loop(self, run, patch, optimizer, scheduler, scal, train_dataloader, val_dataloader, num_iter):
        """UADA.py:117-292, UPA.py:118-275, TMA.py:110-383 around the driver's hooks. Nothing waits for the device inside the inner loop: the scalars
        of an outer iteration's steps stay in `scal` and are read back ONCE (the reference syncs 4-5 times per inner step); nothing of an
        iteration is logged or written before assert_finite_state has seen them. A step that ended in the fused update (fused_update) leaves
        its row in `self._stats_row`: the gradient statistics of the last such step are folded from its block sums here, once (whether steps
        end fused follows from the run's arguments, so the steps of an iteration all do or none does).
        A driver that does not accumulate asks for the `do_step` rule, and so for the loader's length, only where a scheduler follows it."""
        train_iterator, val_iterator = iter(train_dataloader), iter(val_dataloader)
        for i in range(num_iter):
            pixel_values, labels, attention_mask, input_ids = self.fetch_batch(next(train_iterator), run.maskidx, run.filterGripTrainTo1)
            labels = self._train_labels(run, labels)
            do_step = (scheduler is None and not self.accumulates) or (i + 1) % run.accumulate_steps == 0 or (i + 1) == len(train_dataloader)
            self._stats_row = None
            preds = [self._loop_step(run, patch, optimizer, pixel_values, input_ids, attention_mask, labels, scal, k, do_step) for k in range(run.innerLoop)]
            if scheduler is not None and do_step:
                scheduler.step()
            if self._stats_row is not None:
                scal[self._stats_row, 8:10] = optimizer.last_stats
            host = scal[: run.innerLoop].cpu().numpy()
            self.assert_finite_state(patch, optimizer, host[:, :8], f"{self.attack_name} outer iteration {i}")
            self.last_train_log = self._train_log(run, host, preds, labels, optimizer, self.patch_reg_log("TRAIN"))
            if wandb_enabled(run.args):
                wandb.log(self.last_train_log, step=i)
            if i % 100 == 0:
                self.plot_loss()
                val_iterator = self.validate(i, patch, val_dataloader, val_iterator, run)
        return patch

    def val_pass(self, val_batch, patch, val_dataloader, val_iterator):
        """The no-grad sweep every `validate` starts with: `val_batches` batches, the iterator restarted when it runs out, nothing read back
        inside the loop (the host enqueues batch after batch), ONE read-back behind the last batch.
        `val_batch(rb, patch, pixel_values, labels, attention_mask, input_ids)` pastes, labels, calls the model and `rb.add`s; it returns
        (pasted frames, the labels it used — their rows are the samples counted) or None for a batch it leaves out.
        -> (val_iterator, samples, frames of the last batch kept, *ValReadback.read())."""
        rb = ValReadback(self.val_batches, self.device)
        samples, frames = 0, None
        with torch.no_grad():
            for _ in range(self.val_batches):
                data, val_iterator = next_or_restart(val_iterator, val_dataloader)
                kept = val_batch(rb, patch, *to_dev(data, self.device))
                if kept is not None:
                    frames, samples = kept[0], samples + kept[1].shape[0]
        return (val_iterator, samples, frames) + rb.read()

    def save_best_and_last(self, patch, i, best_attr: str, value):
        """patch.pt into `<i>/` when `value` is below the attacker's best so far (`best_attr`, then updated), and into `last/` always
        (UADA.py:257-275) -> the directories written, `last/` last."""
        improved = value < getattr(self, best_attr)
        if improved:
            setattr(self, best_attr, value)
        return ([self.save_patch(patch, f"{str(i)}")] if improved else []) + [self.save_patch(patch, "last")]


def gripper_only(maskidx) -> bool:
    """The attack is on the gripper DoF alone: what turns on the train filter (UADA.py:120) and TMA's validation filter (TMA.py:222)."""
    return len(maskidx) == 1 and maskidx[0] == 6


def to_dev(batch, device):
    """labels/attention_mask/input_ids .to(device) (UADA.py:125-127); `.to` on a same-device tensor aliases, and
    mask_labels mutates in place, so labels are cloned to keep the loader's copy intact."""
    return (batch["pixel_values"], batch["labels"].to(device).clone(), batch["attention_mask"].to(device),
            batch["input_ids"].to(device))


def next_or_restart(iterator, loader):
    try:
        return next(iterator), iterator
    except StopIteration:
        iterator = iter(loader)
        return next(iterator), iterator
