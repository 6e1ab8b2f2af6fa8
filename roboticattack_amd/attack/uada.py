"""UADA — untargeted action-discrepancy attack, single GPU. Mirrors VLAAttacker/white_patch/UADA.py:33-418.

Same class name, constructor and `patchattack_unconstrained` signature, same RNG consumption order, same output
files (`<save_dir>/<iter>/patch.pt`, `last/patch.pt`, PNG dumps, pickled metric lists). The inner loop body is the
HIP path: K1 -> model -> K3 -> K2 -> K4, with no host synchronisation inside the innerLoop. The outer loop and the
validation sweep are AttackBase's (engine.py); this file holds what UADA.py defines differently from UPA.py and TMA.py.
"""
from __future__ import annotations

from functools import partial
from types import SimpleNamespace

import numpy as np

from .. import ops
from .engine import AttackBase, wandb, wandb_enabled


class OpenVLAAttacker(AttackBase):
    val_batches = 1000  # UADA.py:202
    attack_name = "UADA"
    accumulates = False  # the optimiser runs on EVERY inner step whatever accumulate_steps is (UADA.py:155-157): do_step moves the scheduler alone

    def __init__(self, vla, processor=None, save_dir="", optimizer="pgd", resize_patch=False):
        super().__init__(vla, processor, save_dir, optimizer, resize_patch)
        self.MSE_Distance_best = 10000  # UADA.py:59
        self.mse_weight = 5.0  # UADA.py:396
        self.loss_mode = ops.LOSS_UADA  # MSE + 1/CE (UADA.py:147)

    # ------------------------------------------------------------------------------------------
    def inner_step(self, patch, optimizer, pixel_values, input_ids, attention_mask, labels, geometry, scalars_out, k):
        """One iteration of the hot inner loop (UADA.py:133-159). With K2' (a model that exposes its patch-embed weights) the step ends with ONE
        launch that adds K2''s partial tiles and applies AdamW + clamp; the logged gradient statistics are then folded once per outer iteration."""
        sink = self.fused_update_sink(optimizer)
        pix = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std, geometry=geometry,
                                                                  colorjitter=self.randomPatchTransform.colorjitter, **({"grad_sink": sink} if sink is not None else {}))
        total, scalars, pred = self.model_loss(input_ids, attention_mask, pix, labels, self.loss_mode, w=self.mse_weight)
        total.backward()
        self.add_patch_reg(patch)  # K6: + the TV / NPS gradient (a no-op while both weights are 0)
        scalars_out[k, :8] = scalars
        if sink is not None and "partials" in sink:
            self.fused_update(sink, patch, optimizer, scalars)  # K2's final sum + K4 (AdamW + clamp(0,1)) in one launch
            self._stats_row = k
        else:
            scalars_out[k, 8:10] = optimizer.step()  # K4: AdamW + clamp(0,1); patch.data updated in place
        optimizer.zero_grad()
        return pred, pix

    def patchattack_unconstrained(self, train_dataloader, val_dataloader, num_iter=5000, target_action=np.zeros(7),
                                  patch_size=[3, 50, 50], lr=1 / 255, accumulate_steps=1, maskidx=[], warmup=20,
                                  filterGripTrainTo1=False, geometry=False, innerLoop=1, args=None, colorjitter=False, train_crop=None,
                                  train_crop_scale=0.9, scene_jitter=False, defocus_blur=False):
        """UADA.py:93-292; the keywords behind `args` are the EXTENSIONS AttackBase.begin_run states."""
        self.val_CE_loss, self.val_MSE_Distance, self.val_UAD = [], [], []
        self.train_CE_loss, self.train_MSE_distance_loss, self.train_UAD = [], [], []
        run = SimpleNamespace(maskidx=maskidx, geometry=geometry, args=args, accumulate_steps=accumulate_steps, innerLoop=innerLoop,
                              filterGripTrainTo1=filterGripTrainTo1)
        begun = self.begin_run(patch_size, lr, 0.0, warmup, num_iter, accumulate_steps, innerLoop, colorjitter, train_crop, train_crop_scale,
                               scene_jitter, defocus_blur)
        return self.run_outer_loop(run, *begun, train_dataloader, val_dataloader, num_iter)

    def _train_labels(self, run, labels):
        return self.mask_labels(labels, run.maskidx)

    def _loop_step(self, run, patch, optimizer, pixel_values, input_ids, attention_mask, labels, scal, k, do_step):
        return self.inner_step(patch, optimizer, pixel_values, input_ids, attention_mask, labels, run.geometry, scal, k)[0]

    def _train_log(self, run, host, preds, labels, optimizer, reg):
        self.train_CE_loss.extend(host[:, 1].tolist())
        self.train_MSE_distance_loss.extend(host[:, 0].tolist())
        self.train_UAD.extend(host[:, 7].tolist())
        cont_pred, cont_gt = self.decode_pred_gt(preds[-1], labels)
        rd = self.calculate_relative_distance(cont_pred, cont_gt, run.maskidx, {f"{idx}": [] for idx in run.maskidx})
        log = {"TRAIN_attack_loss(CE)": float(host[-1, 1]), "TRAIN_patch_gradient": float(host[-1, 9]), "TRAIN_LR": optimizer.param_groups[0]["lr"],
               "TRAIN_attack_loss (MSE_Distance)": float(host[-1, 0]), "TRAIN_UAD": float(host[-1, 7]), **reg}
        for key, value in rd.items():
            log[f"train_rd_{key}"] = sum(value) / len(value)
        return log

    # ------------------------------------------------------------------------------------------
    def _val_batch(self, run, rb, patch, pixel_values, labels, attention_mask, input_ids):
        frames = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch.detach(), mean=self.mean, std=self.std, geometry=run.geometry)
        labels = self.mask_labels(labels, run.maskidx)
        # (validation is scored with the data-parallel loop's loss, whatever self.loss_mode trains with: UADA.py:227)
        _, scalars, pred = self.model_loss(input_ids, attention_mask, frames, labels, ops.LOSS_UADA_DDP, w=self.mse_weight, need_grad=False)
        rb.add(scalars, pred, labels)
        return frames, labels

    def validate(self, i, patch, val_dataloader, val_iterator, run):
        """UADA.py:193-292: no-grad sweep, best-patch selection by summed MSE distance / #samples, `last/` always."""
        val_iterator, val_num_sample, frames, host, maps = self.val_pass(partial(self._val_batch, run), patch, val_dataloader, val_iterator)
        avg_CE_loss = avg_MSE_Distance = avg_UAD = val_UAD = 0.0
        relative_distance = {f"{idx}": [] for idx in run.maskidx}
        for s, (p_np, gt_np) in zip(host, maps):  # the reference's per-batch bookkeeping (UADA.py:229-246), in batch order
            cont_pred, cont_gt = self.decode_pred_gt_np(p_np, gt_np)
            relative_distance = self.calculate_relative_distance(cont_pred, cont_gt, run.maskidx, relative_distance)
            avg_MSE_Distance += float(np.float32(s[2]))
            val_UAD = float(np.float32(s[7]))
            avg_UAD += val_UAD
            avg_CE_loss += float(np.float32(s[1]))
        avg_MSE_Distance /= val_num_sample
        avg_UAD /= val_num_sample
        avg_CE_loss /= val_num_sample
        log_data = {"VAL_MSE_Distance": avg_MSE_Distance, "VAL_UAD": val_UAD}  # (VAL_UAD: the LAST batch's, UADA.py:251)
        log_data.update(self.patch_reg_log("VAL", patch))
        for key, value in relative_distance.items():
            log_data[f"val_rd_{key}"] = sum(value) / len(value)
        self.last_val_log = log_data
        if wandb_enabled(run.args):
            wandb.log(log_data, step=i)
        dirs = self.save_best_and_last(patch, i, "MSE_Distance_best", avg_MSE_Distance)
        for d in dirs:  # the frames of the last batch go into the best AND the last directory
            _, pil = self.save_val_images(frames, d)
            if wandb_enabled(run.args):
                wandb.log({"Last_Step_AdvImg" if d is dirs[-1] else "AdvImg": [wandb.Image(p) for p in pil]})
        self.val_CE_loss.append(avg_CE_loss)
        self.val_MSE_Distance.append(avg_MSE_Distance)
        self.val_UAD.append(avg_UAD)
        self.save_info(path=self.save_dir)
        return val_iterator

    def save_info(self, path):
        """UADA.py:341-353."""
        self.dump_lists(["train_CE_loss", "train_MSE_distance_loss", "train_UAD", "val_CE_loss", "val_MSE_Distance", "val_UAD"])

    # kept for API parity with the reference class (UADA.py:381-418); the loop itself uses the fused K3
    def weighted_loss(self, logits, labels, maskid=None):
        total, scalars, _ = ops.DiscrepancyLoss.apply(logits.contiguous(), labels, ops.LOSS_UADA_DDP, self.mse_weight, 0.8, 0.2, 1.0,
                                                      ops.LAYOUT_FULL)
        return total, scalars[7]
