"""TMA — targeted manipulation attack. Mirrors VLAAttacker/white_patch/TMA.py:28-483.

Loss = HF mean CE against a fixed target-token vector on the `maskidx` DoFs, divided by accumulate_steps (TMA.py:148);
AdamW (+cosine) or PGD sign step (TMA.py:164-175); without geometry the patch is pasted by `paste_patch_fix`
(mask rule canvas != -100, TMA.py:133-135), with geometry or colorjitter by `apply_random_patch_batch`.
Validation: 100 batches, ASR / L1 metrics, best patch by L1 (TMA.py:202-383). The outer loop and the validation sweep are AttackBase's (engine.py).
"""
from __future__ import annotations

import os
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from ..labels import tma_target_labels, tma_target_tokens
from .engine import AttackBase, gripper_only, wandb, wandb_enabled


class OpenVLAAttacker(AttackBase):
    val_batches = 100  # TMA.py:211
    attack_name = "TMA"

    def __init__(self, vla, processor=None, save_dir="", optimizer="pgd", resize_patch=False):
        super().__init__(vla, processor, save_dir, optimizer, resize_patch)
        self.adv_action_L1_loss = []
        self.min_val_avg_CE_loss = 1000000
        self.min_val_avg_L1_loss = 1000000

    def _images(self, pixel_values, patch, geometry, colorjitter, grad_sink=None, jitter=True):
        """`colorjitter` picks the operator as in the reference (TMA.py:133-135); `jitter=False` (validation) pastes the patch un-jittered."""
        if not geometry and not colorjitter:
            return self.randomPatchTransform.paste_patch_fix(pixel_values, patch, mean=self.mean, std=self.std)
        kw = {"grad_sink": grad_sink} if grad_sink is not None else {}
        return self.randomPatchTransform.apply_random_patch_batch(pixel_values, patch, mean=self.mean, std=self.std,
                                                                   geometry=geometry, colorjitter=colorjitter if jitter else False, **kw)

    def calculate_relative_distance_target(self, pred, gt):
        """TMA.py:470-483."""
        if pred.shape[0] == 0:
            return torch.tensor(0.0)
        max_b = torch.maximum(1 - gt, gt - (-1))
        return (torch.abs(pred - gt) / max_b).sum() / pred.shape[0]

    def calculate_01_ASR(self, pred, gt):
        """TMA.py:398-420 (gripper ASR bookkeeping)."""
        s02 = n0 = s12 = n1 = so2 = no = 0
        for idx in range(gt.shape[0]):
            if gt[idx] == 31872:
                n0 += 1
                s02 += int(pred[idx] != 31872)
            elif gt[idx] == 31744:
                n1 += 1
                s12 += int(pred[idx] != 31744)
            else:
                no += 1
                so2 += int(pred[idx] == 31872)
        return s02, n0, s12, n1, so2, no

    def inner_step(self, patch, optimizer, pixel_values, input_ids, attention_mask, newlabels, geometry, colorjitter, scalars_out, k,
                   accumulate_steps=1, do_step=True):
        """One iteration of the hot inner loop (TMA.py:131-175): K1 -> model -> GEMM head + K3 (CE gradient over every logit of the labelled rows) ->
        backward -> K2 / K2' -> K4. Without gradient accumulation the step ends with ONE launch: K2's final sum + the optimiser (AdamW or PGD
        sign step) + clamp. Returns (full-vocabulary predictions, whether the update ran inside that launch)."""
        sink = self.fused_update_sink(optimizer) if (accumulate_steps == 1 and geometry) else None
        pix = self._images(pixel_values, patch, geometry, colorjitter, grad_sink=sink)
        total, scalars, pred = self.model_loss(input_ids, attention_mask, pix, newlabels, ops.LOSS_CE, scale=1.0 / accumulate_steps)
        total.backward()
        self.add_patch_reg(patch, scale=1.0 / accumulate_steps)  # K6: + the TV / NPS gradient, scaled like the loss, in front of the PGD sign
        fused = sink is not None and "partials" in sink
        if fused:
            self.fused_update(sink, patch, optimizer, scalars)
            self._stats_row = k
            optimizer.zero_grad()
        elif do_step:
            scalars_out[k, 8:10] = optimizer.step()
            optimizer.zero_grad()
        scalars_out[k, :8] = scalars
        return pred, fused

    def patchattack_unconstrained(self, train_dataloader, val_dataloader, num_iter=5000, target_action=np.zeros(7),
                                  patch_size=[3, 50, 50], alpha=1 / 255, accumulate_steps=1, maskidx=[], warmup=20,
                                  filterGripTrainTo1=False, geometry=False, colorjitter=False, innerLoop=1, args=None, train_crop=None,
                                  train_crop_scale=0.9, scene_jitter=False, defocus_blur=False):
        """TMA.py:82-383 (`alpha` is the step size); `colorjitter` and the keywords behind `args` are the EXTENSIONS AttackBase.begin_run states."""
        self.val_CE_loss, self.val_L1_loss, self.val_ASR, self.val_inner_relatived_distance = [], [], [], []
        self.train_CE_loss, self.train_inner_avg_loss, self.train_inner_relatived_distance = [], [], []
        begun = self.begin_run(patch_size, alpha, 0.0, warmup, num_iter, accumulate_steps, innerLoop, colorjitter, train_crop, train_crop_scale,
                               scene_jitter, defocus_blur)
        target = tma_target_tokens(target_action, maskidx, self.action_tokenizer).to(self.device)  # TMA.py:93-99, behind the patch's draw
        print(f"target_action: {target}")
        run = SimpleNamespace(maskidx=maskidx, geometry=geometry, args=args, accumulate_steps=accumulate_steps, innerLoop=innerLoop,
                              filterGripTrainTo1=filterGripTrainTo1, colorjitter=colorjitter, target=target, gripper=gripper_only(maskidx))
        return self.run_outer_loop(run, *begun, train_dataloader, val_dataloader, num_iter)

    def _train_labels(self, run, labels):
        return tma_target_labels(labels, run.target)  # TMA.py:124-129

    def _loop_step(self, run, patch, optimizer, pixel_values, input_ids, attention_mask, labels, scal, k, do_step):
        return self.inner_step(patch, optimizer, pixel_values, input_ids, attention_mask, labels, run.geometry, run.colorjitter, scal, k,
                               accumulate_steps=run.accumulate_steps, do_step=do_step)[0]

    def _train_log(self, run, host, preds, labels, optimizer, reg):
        inner_avg_loss = float(host[:, 0].mean())
        inner_rel = 0.0
        for p in preds:  # the predictions of EVERY inner step (TMA.py:153-162)
            cp, cg = self.decode_pred_gt(p, labels)
            inner_rel += float(self.calculate_relative_distance_target(cp, cg))
        inner_rel /= run.innerLoop
        loss = float(host[-1, 0])
        self.loss_buffer.append(loss)
        print(f"target_loss: {loss}")
        self.train_CE_loss.append(loss)
        self.train_inner_avg_loss.append(inner_avg_loss)
        self.train_inner_relatived_distance.append(inner_rel)
        return {"TRAIN_attack_loss(CE)": loss, "TRAIN_patch_gradient": float(host[-1, 9]), "TRAIN_LR": optimizer.param_groups[0]["lr"],
                "TRAIN_inner_avg_loss": inner_avg_loss, "TRAIN_inner_relatived_distance": inner_rel, **reg}

    def _val_batch(self, run, orig_gt, rb, patch, pixel_values, labels, attention_mask, input_ids):
        if run.gripper:  # keep only samples whose clean gripper prediction is right (TMA.py:222-248): the NEXT forward's batch depends
            # on this forward's predictions — the one read-back per batch that cannot be deferred
            clean = self.randomPatchTransform.im_process(pixel_values, mean=self.mean, std=self.std)
            _, _, pre = self.model_loss(input_ids, attention_mask, clean, labels, ops.LOSS_CE, need_grad=False)
            pm = pre.cpu().numpy()
            gt = labels[:, 1:].cpu().numpy()
            ok = [b for b in range(gt.shape[0]) if pm[b][gt[b] > 31743][-1] == gt[b][gt[b] > 31743][-1]]
            if not ok:
                print("No Correct in Val!")
                return None  # no read-back row, no samples
            labels, attention_mask, input_ids = labels[ok], attention_mask[ok], input_ids[ok]
            pixel_values = [pixel_values[b] for b in ok]
            orig_gt.append(gt[ok])
        frames = self._images(pixel_values, patch.detach(), run.geometry, run.colorjitter, jitter=False)
        newlabels = tma_target_labels(labels, run.target)
        _, scalars, pred = self.model_loss(input_ids, attention_mask, frames, newlabels, ops.LOSS_CE, need_grad=False)
        rb.add(scalars, pred, newlabels)
        return frames, newlabels

    def validate(self, i, patch, val_dataloader, val_iterator, run):
        orig_gt = []  # gripper mode: the unmodified labels of the kept samples (already on the host there: the filter has to look at them)
        val_iterator, val_num_sample, frames, host, maps = self.val_pass(partial(self._val_batch, run, orig_gt), patch, val_dataloader, val_iterator)
        avg_CE = avg_L1 = val_rel = 0.0
        success = 0
        asr6 = [0] * 6
        cont_pred = cont_gt = None
        n = max(len(run.maskidx), 1)
        for k, (sc, (p_np, gt_np)) in enumerate(zip(host, maps)):  # the reference's per-batch bookkeeping (TMA.py:250-290), in batch order
            cont_pred, cont_gt = self.decode_pred_gt_np(p_np, gt_np)
            val_rel += float(self.calculate_relative_distance_target(cont_pred, cont_gt))
            if run.gripper:
                tm = gt_np > 31743
                r = self.calculate_01_ASR(p_np[tm], orig_gt[k][tm])
                asr6 = [a + b for a, b in zip(asr6, r)]
            avg_L1 += float(torch.nn.functional.l1_loss(cont_pred, cont_gt)) if cont_pred.numel() else 0.0
            if cont_pred.numel():
                eq = (cont_pred.view(-1, n) == cont_gt.view(-1, n)).all(dim=1)
                success += int(eq.sum())
            avg_CE += float(np.float32(sc[1]))
        val_num_sample = max(val_num_sample, 1)
        avg_L1 /= val_num_sample
        avg_CE /= val_num_sample
        ASR = success / val_num_sample
        val_rel /= val_num_sample
        self.last_val_log = {"VAL_avg_CE_loss": avg_CE, "VAL_avg_L1_loss": avg_L1, "VAL_ASR": ASR, "VAL_inner_relatived_distance": val_rel}
        self.last_val_log.update(self.patch_reg_log("VAL", patch))
        if run.gripper:
            s02, n0, s12, n1, so2, no = asr6
            self.last_val_log.update({"ASR_02other": s02 / n0 if n0 else 0, "ASR_12other": s12 / n1 if n1 else 0,
                                      "ASR_other20": so2 / no if no else 0, "ALL_ASR_6": (s02 + s12) / (n0 + n1) if (n0 + n1) else 0})
        if wandb_enabled(run.args):
            wandb.log(self.last_val_log, step=i)
        dirs = self.save_best_and_last(patch, i, "min_val_avg_L1_loss", avg_L1)
        for k, d in enumerate(dirs):  # frames only into the best directory when there are two; the last batch's actions into every one
            if frames is not None and (k == 0 and len(dirs) == 2):
                path, _ = self.save_val_images(frames, d)
            else:
                path = os.path.join(d, "val_related_data")
                os.makedirs(path, exist_ok=True)
            if cont_pred is not None:
                torch.save(cont_pred.detach().cpu(), os.path.join(path, "continuous_actions_pred.pt"))
                torch.save(cont_gt.detach().cpu(), os.path.join(path, "continuous_actions_gt.pt"))
        self.val_CE_loss.append(avg_CE)
        self.val_L1_loss.append(avg_L1)
        self.val_ASR.append(success / val_num_sample)
        self.val_inner_relatived_distance.append(val_rel)
        self.save_info(self.save_dir)
        return val_iterator

    def save_info(self, path):
        """TMA.py:454-468."""
        self.dump_lists(["val_CE_loss", "val_L1_loss", "val_ASR", "val_inner_relatived_distance", "train_CE_loss",
                         "train_inner_avg_loss", "train_inner_relatived_distance"])
