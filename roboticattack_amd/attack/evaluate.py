"""Open-loop evaluation of a finished patch: what it does to the greedily decoded actions on recorded frames once the evaluation's own image
path is applied — the part of the reference's LIBERO evaluation (experiments/robot/libero/run_libero_eval_args_geo_batch.py:205-221,
experiments/robot/openvla_utils.py:127-170) that needs no simulator. Per camera frame the reference pastes the patch at a fixed angle, shear and
position (K5, RandomPatchTransform.simulation_patch_batch), centre-crops to 0.9 of the area and resizes back, converts to uint8, runs the
processor (K7, RandomPatchTransform.eval_pixel_values) and calls predict_action; here the same chain runs on a batch of (frame, placement)
pairs and is compared with the clean frames' actions.

`summarise` holds the metric arithmetic on CPU tensors; `evaluate_patch` is the device driver.
"""
from __future__ import annotations

import numpy as np
import torch

from ..action_tokenizer import ActionTokenizer
from ..predict import unnormalize_actions


def _target_tokens(target, action_dim: int):
    """(maskidx, target_action) -> (maskidx list, int64 token per entry). target_action: a scalar, one value per maskidx entry, or a whole
    action vector of `action_dim` values indexed by maskidx (TMA's convention, TMA.py:93-99)."""
    maskidx, action = target
    maskidx = [int(i) for i in maskidx]
    if any(i < 0 or i >= action_dim for i in maskidx):
        raise ValueError(f"target maskidx {maskidx} outside the {action_dim} action dimensions")
    a = np.atleast_1d(np.asarray(action, dtype=np.float64))
    if a.size == 1:
        a = np.full(len(maskidx), float(a[0]))
    elif a.size == action_dim:
        a = a[maskidx]
    elif a.size != len(maskidx):
        raise ValueError(f"target action has {a.size} values for {len(maskidx)} maskidx entries")
    return maskidx, torch.from_numpy(ActionTokenizer().action_to_token_ids(a))


def _rates(clean: torch.Tensor, patched: torch.Tensor, unnorm_stats, target):
    """clean, patched int64 [N,A] (row n of both is the same frame) -> the metrics of those N rows."""
    at = ActionTokenizer()
    flip = clean != patched
    a_c, a_p = at.decode_token_ids_to_actions(clean.numpy()), at.decode_token_ids_to_actions(patched.numpy())
    out = {
        "token_flip_rate": flip.double().mean(0),
        "nad": torch.from_numpy(np.abs(a_p - a_c).mean(0) / 2.0),
        "any_flip_rate": float(flip.any(1).double().mean()),
    }
    if unnorm_stats is not None:
        out["l1_unnorm"] = torch.from_numpy(np.abs(unnormalize_actions(a_p, unnorm_stats) - unnormalize_actions(a_c, unnorm_stats)).mean(0))
    if target is not None:
        maskidx, tok = _target_tokens(target, clean.shape[1])
        out["target_hit_rate"] = (patched[:, maskidx] == tok[None, :]).double().mean(0)
    return out


def summarise(tokens_clean: torch.Tensor, tokens_patched: torch.Tensor, unnorm_stats=None, target=None) -> dict:
    """tokens_clean int64 [F,A], tokens_patched int64 [P,F,A] (CPU) -> {"per_placement": [P dicts], "overall": dict}. Each dict holds
      token_flip_rate [A]  share of frames whose decoded token of that DoF changed
      nad [A]              mean |a_patched - a_clean| / 2 on the tokens' bin centres in [-1, 1] (normalised action discrepancy)
      any_flip_rate        share of frames with at least one changed token
      l1_unnorm [A]        mean |difference| of the un-normalised actions (only with unnorm_stats: q01, q99, optional mask)
      target_hit_rate [len(maskidx)]  share of frames whose patched token of DoF maskidx[i] is the token of the target action
                           (only with target = (maskidx, target_action))
    "overall" treats every (placement, frame) pair as one row."""
    tokens_clean, tokens_patched = torch.as_tensor(tokens_clean).to(torch.int64).cpu(), torch.as_tensor(tokens_patched).to(torch.int64).cpu()
    if tokens_clean.dim() != 2 or tokens_patched.dim() != 3 or tuple(tokens_patched.shape[1:]) != tuple(tokens_clean.shape):
        raise ValueError(f"expected tokens_clean [F,A] and tokens_patched [P,F,A], got {tuple(tokens_clean.shape)} and {tuple(tokens_patched.shape)}")
    P, F, A = tokens_patched.shape
    per = [_rates(tokens_clean, tokens_patched[p], unnorm_stats, target) for p in range(P)]
    overall = _rates(tokens_clean.repeat(P, 1), tokens_patched.reshape(P * F, A), unnorm_stats, target)
    return {"per_placement": per, "overall": overall}


@torch.no_grad()
def evaluate_patch(model, transform, frames_u8, input_ids, attention_mask, patch, placements, *, center_crop=True, crop_scale=0.9, mean, std,
                   unnorm_stats=None, action_dim=7, target=None, bs=8, quant_model=None, resize=None, rot180=False, jpeg_quality=None,
                   jpeg_compare=False) -> dict:
    """Clean and patched greedy actions of `model` on F recorded frames with their prompts (right-padded input_ids / attention_mask [F,L]).
    placements: list of (geometry, angle, shx, shy, x, y), the per-frame arguments of simulation_patch_batch. The clean actions are decoded
    once per frame and reused for every placement; the patched rows are the P*F (placement, frame) pairs in placement-major order, run in
    batches of at most `bs` rows (K5 paste -> K7 crop / normalise -> predict_action). Nothing but token ids travels to the host: predict_action's
    own read-back and one copy of the collected ids at the end.
    Returns {"tokens_clean" [F,A], "tokens_patched" [P,F,A], "placements", **summarise(...)}.
    quant_model (the same model converted by quant.quantize_llm): every batch is decoded on it as well, from the same pixel values; the report
    gains "quantised" (the same four entries for that model, "quant_type") and "clean_agreement" (see clean_agreement) — without the latter the
    two models' patched rates cannot be compared.
    resize="lanczos3": frames_u8 are a simulator's camera frames [F,H,W,3] of any size; each is resized to 224x224 once (K8,
    transform.eval_frames; rot180=True rotates it by 180 degrees first, as the LIBERO evaluation does), before the clean pass, and everything
    above runs on the resized frames. Without it the frames must be 224x224 and are used as they are.
    jpeg_quality (an integer 1..100, with resize="lanczos3" only: it is a step of the simulators' resize_image): every frame goes through a JPEG
    encoder and decoder at that quality between the rotation and the resize (K12), as libero_utils.py:42-43 does at 95. jpeg_compare=True
    (with a jpeg_quality): the clean pass runs once more on the frames resized WITHOUT the JPEG step, and the report gains "jpeg_agreement"
    (clean_agreement of the two clean token sets of `model`): what the step is worth on these frames."""
    if bs < 1:
        raise ValueError("bs must be at least 1")
    if resize not in (None, "lanczos3"):
        raise ValueError(f"resize must be None or 'lanczos3', got {resize!r}")
    if resize is None and rot180:
        raise ValueError("rot180 is part of the frame resize: pass resize='lanczos3'")
    if jpeg_quality is not None and resize is None:
        raise ValueError("jpeg_quality is part of the frame resize: pass resize='lanczos3'")
    if jpeg_quality is not None and (isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, (int, np.integer)) or not 1 <= jpeg_quality <= 100):
        raise ValueError(f"jpeg_quality must be an integer in 1..100, got {jpeg_quality!r}")
    if jpeg_compare and jpeg_quality is None:
        raise ValueError("jpeg_compare compares with and without the JPEG step: pass a jpeg_quality")
    dev = transform.device
    frames_nojpeg = None
    if resize is not None and jpeg_quality is None:
        frames_u8 = transform.eval_frames(frames_u8, rot180)
    elif resize is not None:
        if jpeg_compare:
            frames_nojpeg = transform.stage_images(transform.eval_frames(frames_u8, rot180))
        frames_u8 = transform.eval_frames(frames_u8, rot180, jpeg_quality=int(jpeg_quality))
    frames = transform.stage_images(frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.as_tensor(np.asarray(frames_u8)))
    ids, mask = input_ids.to(dev), attention_mask.to(dev)
    F, P = int(frames.shape[0]), len(placements)
    if ids.shape[0] != F or mask.shape[0] != F:
        raise ValueError(f"{F} frames but {ids.shape[0]} prompts")
    patch = patch.detach().to(dev, torch.float32).contiguous()
    placements = [(bool(g), float(a), float(sx), float(sy), int(x), int(y)) for g, a, sx, sy, x, y in placements]

    models = [model] + ([quant_model] if quant_model is not None else [])

    def decode(pix, rows):
        return torch.stack([m.predict_action(ids[rows], mask[rows], pix, unnorm_stats=unnorm_stats, action_dim=action_dim)[0] for m in models], 1)

    clean = []
    for i in range(0, F, bs):
        rows = torch.arange(i, min(i + bs, F), device=dev)
        clean.append(decode(transform.eval_pixel_values(frames[rows], mean, std, center_crop, crop_scale), rows))
    patched = []
    for i in range(0, P * F, bs):
        pairs = range(i, min(i + bs, P * F))
        rows = torch.tensor([r % F for r in pairs], device=dev)
        geo, ang, shx, shy, pos = zip(*[(g, a, sx, sy, (x, y)) for g, a, sx, sy, x, y in (placements[r // F] for r in pairs)])
        pasted = transform.simulation_patch_batch(frames[rows], patch, geo, ang, shx, shy, pos)
        patched.append(decode(transform.eval_pixel_values(pasted, mean, std, center_crop, crop_scale), rows))
    clean = torch.cat(clean).cpu()  # [F, models, A]
    clean_nojpeg = None
    if frames_nojpeg is not None:
        clean_nojpeg = []
        for i in range(0, F, bs):
            rows = torch.arange(i, min(i + bs, F), device=dev)
            pix = transform.eval_pixel_values(frames_nojpeg[rows], mean, std, center_crop, crop_scale)
            clean_nojpeg.append(model.predict_action(ids[rows], mask[rows], pix, unnorm_stats=unnorm_stats, action_dim=action_dim)[0])
        clean_nojpeg = torch.cat(clean_nojpeg).cpu()
    patched = torch.cat(patched).cpu() if patched else torch.empty((0, len(models), action_dim), dtype=torch.int64)

    def report(i):
        tokens_clean, tokens_patched = clean[:, i].contiguous(), patched[:, i].reshape(P, F, action_dim)
        return {"tokens_clean": tokens_clean, "tokens_patched": tokens_patched, **summarise(tokens_clean, tokens_patched, unnorm_stats, target)}

    out = {"placements": placements, **report(0)}
    if quant_model is not None:
        out["quantised"] = dict(report(1), quant_type=getattr(quant_model, "quant_type", None))
        out["clean_agreement"] = clean_agreement(out["tokens_clean"], out["quantised"]["tokens_clean"])
    if clean_nojpeg is not None:
        out["jpeg_agreement"] = clean_agreement(out["tokens_clean"], clean_nojpeg)
    return out


def clean_agreement(tokens_a: torch.Tensor, tokens_b: torch.Tensor) -> dict:
    """Two models' clean tokens int64 [F,A] -> {"frames": share of frames whose whole action is the same, "tokens": share of equal tokens}."""
    same = torch.as_tensor(tokens_a).cpu() == torch.as_tensor(tokens_b).cpu()
    return {"frames": float(same.all(1).double().mean()), "tokens": float(same.double().mean())}


def to_jsonable(report: dict):
    """The report with tensors / arrays as nested lists (what the CLI writes)."""
    if isinstance(report, dict):
        return {k: to_jsonable(v) for k, v in report.items()}
    if isinstance(report, (list, tuple)):
        return [to_jsonable(v) for v in report]
    if isinstance(report, (torch.Tensor, np.ndarray)):
        return report.tolist()
    if isinstance(report, (np.floating, np.integer, np.bool_)):
        return report.item()
    return report
