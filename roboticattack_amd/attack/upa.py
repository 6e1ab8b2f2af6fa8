"""UPA — untargeted position-aware attack. Mirrors VLAAttacker/white_patch/UPA.py:30-387.

reverse_direction=True (the CLI default): labels stay unmasked and the loss is
    alpha*mean_b(cos(e', l') + 1) + beta/(mean_b ||e' - l'||_2 + 1e-3)        (UPA.py:367-387)
over the soft-argmax of the first three action tokens (x, y, z). Other modes: `guide` (+CE against flipped targets,
UPA.py:130-131,143-144,358-364) and plain -CE (UPA.py:149-150). Every step clips the patch gradient to L1 norm 1e-3
before AdamW (UPA.py:157) — fused into K4. Validation: 100 batches, best patch by reverse-direction loss (UPA.py:193-275).
The outer loop and the validation sweep are AttackBase's (engine.py).
"""
from __future__ import annotations

import os
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from .engine import AttackBase, wandb, wandb_enabled


class OpenVLAAttacker(AttackBase):
    val_batches = 100  # UPA.py:205
    attack_name = "UPA"

    def __init__(self, vla, processor=None, save_dir="", optimizer="pgd", resize_patch=False, alpha=0.8, belta=0.2):
        super().__init__(vla, processor, save_dir, optimizer, resize_patch)
        self.alpha, self.belta = alpha, belta
        self.avg_angle_loss, self.avg_distance_loss, self.avg_reserve_loss = [], [], []
        self.reverse_direction_loss = 100000
        self.min_val_avg_L1_loss = 1000000

    def change_target(self, gt):
        """UPA.py:358-364, reproduced statement by statement. The reference assigns SEQUENTIALLY on the tensor it is rewriting: ties at
        31872 are first broken at random (one torch.randint draw, kept so the RNG stream matches), then every label > 31872 becomes
        31744, then every label < 31872 — which by now includes all the 31744s just written and the EOS token 2 — becomes 31999. The
        net effect of the shipped code is therefore "every non-ignored label -> 31999"; kept as is for parity (guide mode is off by
        default: UPA_wrapper.py passes guide=False)."""
        mask = gt != -100
        mid = mask & (gt == 31872)
        r = torch.randint(0, 2, gt[mid].shape, dtype=torch.bool).to(gt.device)
        gt[mid] = torch.where(r, torch.tensor(31744, dtype=gt.dtype, device=gt.device), torch.tensor(31999, dtype=gt.dtype, device=gt.device))
        gt[mask & (gt > 31872)] = 31744
        gt[mask & (gt < 31872)] = 31999
        return gt

    def _mode(self, guide, reverse_direction):
        if guide:
            return ops.LOSS_CE, 1.0
        if reverse_direction:
            return ops.LOSS_UPA, 1.0
        return ops.LOSS_CE, -1.0  # loss = -output.loss (UPA.py:150)

    def inner_step(self, patch, optimizer, pixel_values, input_ids, attention_mask, labels, geometry, mode, scale, scalars_out, k, do_step=True, read_scalars=True):
        """One iteration of the hot inner loop (UPA.py:127-159): [K0 per-image patch resize ->] K1 -> model -> K3 (K3h when the loss lives in the
        action slice) -> backward -> K2 / K2' (MULTI forms with resize_patch) -> K4 with the L1 clip (UPA.py:157) in front of AdamW."""
        pix = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std, geometry=geometry,
                                                                  colorjitter=self.randomPatchTransform.colorjitter)
        # the reverse-direction loop never reads output.loss nor a full-vocabulary argmax (UPA.py:145-150,171-186): slice-only head (K3s)
        # (`read_scalars`: the loop prints / logs the loss terms of the LAST inner step of an outer iteration only, UPA.py:171-186: the others skip the fold)
        total, scalars, pred = self.model_loss(input_ids, attention_mask, pix, labels, mode, alpha=self.alpha, beta=self.belta, scale=scale, full_ce=False,
                                               read_scalars=read_scalars)
        total.backward()
        self.add_patch_reg(patch)  # K6: + the TV / NPS gradient, in front of the L1 clip (a no-op while both weights are 0)
        if do_step:
            stats = optimizer.step()  # K4: L1 clip 1e-3 -> AdamW -> clamp
            if read_scalars:
                scalars_out[k, 8:10] = stats
            optimizer.zero_grad()
        if read_scalars:
            scalars_out[k, :8] = scalars
        return pred

    def patchattack_unconstrained(self, train_dataloader, val_dataloader, num_iter=5000, target_action=np.zeros(7),
                                  patch_size=[3, 50, 50], lr=1 / 255, accumulate_steps=1, maskidx=[], warmup=20,
                                  filterGripTrainTo1=False, geometry=False, innerLoop=1, guide=False, reverse_direction=False, args=None, colorjitter=False,
                                  train_crop=None, train_crop_scale=0.9, scene_jitter=False, defocus_blur=False):
        """UPA.py:93-275; the keywords behind `args` are the EXTENSIONS AttackBase.begin_run states."""
        self.val_CE_loss, self.val_L1_loss, self.val_ASR, self.train_CE_loss, self.val_relative_distance = [], [], [], [], []
        mode, scale = self._mode(guide, reverse_direction)
        run = SimpleNamespace(maskidx=maskidx, geometry=geometry, args=args, accumulate_steps=accumulate_steps, innerLoop=innerLoop,
                              filterGripTrainTo1=filterGripTrainTo1, guide=guide, reverse_direction=reverse_direction, mode=mode, scale=scale)
        begun = self.begin_run(patch_size, lr, 1e-3, warmup, num_iter, accumulate_steps, innerLoop, colorjitter, train_crop, train_crop_scale,
                               scene_jitter, defocus_blur)
        return self.run_outer_loop(run, *begun, train_dataloader, val_dataloader, num_iter)

    def _train_labels(self, run, labels):
        if not run.reverse_direction:
            labels = self.mask_labels(labels, run.maskidx)
        return self.change_target(labels) if run.guide else labels

    def _loop_step(self, run, patch, optimizer, pixel_values, input_ids, attention_mask, labels, scal, k, do_step):
        every = os.environ.get("VAA_FULL_CE_EVERY_STEP", "0") == "1"  # (=1: every step folds its scalars; same patch bits)
        return self.inner_step(patch, optimizer, pixel_values, input_ids, attention_mask, labels, run.geometry, run.mode, run.scale, scal, k, do_step=do_step,
                               read_scalars=every or k == run.innerLoop - 1)

    def _train_log(self, run, host, preds, labels, optimizer, reg):
        loss = float(host[-1, 0])
        print(f"loss: {loss}, " if run.reverse_direction else f"target_loss: {loss}")
        self.train_CE_loss.append(loss)
        return {"TRAIN_attack_loss(CE)": loss, "TRAIN_patch_gradient": float(host[-1, 9]), "TRAIN_LR": optimizer.param_groups[0]["lr"],
                "TRAIN_ANGLE_LOSS": float(host[-1, 3]), "TRAIN_DISTANCE_LOSS": float(host[-1, 4]), **reg}

    def _val_batch(self, run, rb, patch, pixel_values, labels, attention_mask, input_ids):
        frames = self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch.detach(), mean=self.mean, std=self.std, geometry=run.geometry)
        if not run.reverse_direction:
            labels = self.mask_labels(labels, run.maskidx)
        _, scalars, _ = self.model_loss(input_ids, attention_mask, frames, labels, run.mode, alpha=self.alpha, beta=self.belta, scale=run.scale,
                                        need_grad=False, full_ce=False)
        rb.add(scalars)
        return frames, labels

    def validate(self, i, patch, val_dataloader, val_iterator, run):
        val_iterator, val_num_sample, frames, host, _ = self.val_pass(partial(self._val_batch, run), patch, val_dataloader, val_iterator)
        avg_angle = avg_dist = avg_res = 0.0
        for s in host:
            avg_angle += float(np.float32(s[3]))
            avg_dist += float(np.float32(s[4]))
            avg_res += float(np.float32(s[0]))
        avg_angle /= val_num_sample
        avg_dist /= val_num_sample
        avg_res /= val_num_sample
        self.last_val_log = {"reverse_direction_loss": avg_res, "avg_angle_loss": avg_angle, "avg_distance_loss": avg_dist}
        self.last_val_log.update(self.patch_reg_log("VAL", patch))
        if wandb_enabled(run.args):
            wandb.log(self.last_val_log, step=i)
        dirs = self.save_best_and_last(patch, i, "reverse_direction_loss", avg_res)
        if len(dirs) == 2:  # frames into the best directory only; last/ gets the empty folder (UPA.py:247-265)
            self.save_val_images(frames, dirs[0])
        os.makedirs(os.path.join(dirs[-1], "val_related_data"), exist_ok=True)
        self.val_CE_loss.append(0)
        self.val_L1_loss.append(0)
        self.val_ASR.append(0 / val_num_sample)
        self.avg_angle_loss.append(avg_angle / val_num_sample)  # UPA.py:269-271 divides a second time
        self.avg_distance_loss.append(avg_dist / val_num_sample)
        self.avg_reserve_loss.append(avg_res / val_num_sample)
        self.save_info(self.save_dir)
        return val_iterator

    def save_info(self, path):
        """UPA.py:309-325 (three file names differ from the attribute names there)."""
        self.dump_lists(["val_relative_distance", "val_CE_loss", "val_L1_loss", "val_ASR", "train_CE_loss", ("val_avg_angle_loss", "avg_angle_loss"),
                         ("val_avg_distance_loss", "avg_distance_loss"), ("val_avg_reserve_loss", "avg_reserve_loss")])
