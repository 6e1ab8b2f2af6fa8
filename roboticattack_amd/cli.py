"""Shared pieces of the four wrapper CLIs (VLAAttacker/*_wrapper.py): flags, seeding, model/data factories, run dirs.

Flag names, types and defaults are the reference's (UADA_wrapper.py:87-121, UADA_wrapper_ddp.py:87-119,
TMA_wrapper.py:89-124, UPA_wrapper.py:90-127). Added flags (all optional, defaults keep reference behaviour where the
environment allows): --vla_path (local checkpoint dir, or random:openvla-7b / random:tiny / surrogate), --data (synthetic),
--colorjitter / --colorjitter_strength (photometric draw on the patch in training steps; off by default),
--train_crop / --train_crop_scale (the evaluation's crop inside the training steps; off by default),
--scene_jitter / --scene_jitter_strength (brightness / contrast / saturation / hue draw of the whole pasted frame in training steps; off by default),
--defocus_blur / --defocus_blur_sigma (per-image Gaussian blur of the whole pasted frame in training steps; off by default),
--tv_weight / --nps_weight / --nps_palette (total-variation and non-printability terms of the patch; off by default).
"""
from __future__ import annotations

import argparse
import os
import random
import uuid

import numpy as np
import torch


def list_of_ints(arg):
    return list(map(int, arg.split(",")))


def three_floats(arg):
    vals = tuple(map(float, arg.split(",")))
    if len(vals) != 3:
        raise argparse.ArgumentTypeError("three comma-separated floats expected (brightness,contrast,saturation)")
    return vals


def colorjitter_arg(args):
    """--colorjitter / --colorjitter_strength as the attackers take them: False, or the three strengths."""
    return tuple(args.colorjitter_strength) if args.colorjitter else False


def train_crop_args(args):
    """--train_crop / --train_crop_scale as the attackers take them: dict(train_crop=None | "center" | "random", train_crop_scale=area share)."""
    return {"train_crop": None if args.train_crop == "none" else args.train_crop, "train_crop_scale": float(args.train_crop_scale)}


def four_floats(s: str):
    """'0.2,0.2,0.2,0.05' -> (0.2, 0.2, 0.2, 0.05) (the --scene_jitter_strength value)."""
    try:
        v = tuple(float(x) for x in s.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"four comma-separated numbers expected, got {s!r}")
    if len(v) != 4 or not all(0.0 <= x <= 1.0 for x in v[:3]) or not 0.0 <= v[3] <= 0.5:
        raise argparse.ArgumentTypeError(f"four strengths expected (brightness, contrast, saturation in [0, 1], hue in [0, 0.5]), got {s!r}")
    return v


def scene_jitter_arg(args):
    """--scene_jitter / --scene_jitter_strength as the attackers take them: dict(scene_jitter=False | the four strengths)."""
    return {"scene_jitter": tuple(args.scene_jitter_strength) if args.scene_jitter else False}


def blur_sigma(s: str):
    """'1.0' -> 1.0 (the --defocus_blur_sigma value: the maximum sigma in pixels, in (0, 2.0])."""
    try:
        v = float(s)
    except ValueError:
        raise argparse.ArgumentTypeError(f"a number expected, got {s!r}")
    if not 0.0 < v <= 2.0:
        raise argparse.ArgumentTypeError(f"a maximum sigma in (0, 2.0] pixels expected, got {s!r}")
    return v


def defocus_blur_arg(args):
    """--defocus_blur / --defocus_blur_sigma as the attackers take them: dict(defocus_blur=False | the maximum sigma)."""
    return {"defocus_blur": float(args.defocus_blur_sigma) if args.defocus_blur else False}


def patch_reg_args(args):
    """--tv_weight / --nps_weight / --nps_palette as AttackBase.set_patch_reg (and the data-parallel attacker's constructor) take them:
    (tv_weight, nps_weight, palette [K,3] | None = the built-in grid). The file is read here, so a bad palette stops the run before the model loads."""
    from .palette import load_palette

    return float(args.tv_weight), float(args.nps_weight), (load_palette(args.nps_palette) if args.nps_palette else None)


def str2bool(value):
    if isinstance(value, bool):
        return value
    if value.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if value.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def set_seed(seed: int):
    """UADA_wrapper.py:15-23."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


DATASET_TO_CKPT = (  # UADA_wrapper.py:29-40
    ("bridge_orig", "openvla/openvla-7b"),
    ("libero_spatial", "openvla/openvla-7b-finetuned-libero-spatial"),
    ("libero_object", "openvla/openvla-7b-finetuned-libero-object"),
    ("libero_goal", "openvla/openvla-7b-finetuned-libero-goal"),
    ("libero_10", "openvla/openvla-7b-finetuned-libero-10"),
)


def vla_path_for(dataset: str) -> str:
    for key, path in DATASET_TO_CKPT:
        if key in dataset:
            return path
    assert False, "Invalid dataset"


def add_common(parser: argparse.ArgumentParser, *, lr, maskidx, iters, warmup, inner, device_default, tags):
    parser.add_argument("--maskidx", default=maskidx, type=list_of_ints)
    parser.add_argument("--lr", default=lr, type=float)
    if device_default is not None:
        parser.add_argument("--device", default=device_default, type=int)
    parser.add_argument("--iter", default=iters, type=int)
    parser.add_argument("--accumulate", default=1, type=int)
    parser.add_argument("--bs", default=8, type=int)
    parser.add_argument("--warmup", default=warmup, type=int)
    parser.add_argument("--tags", nargs="+", default=tags)
    parser.add_argument("--geometry", type=str2bool, nargs="?", default=True, help="add geometry trans to path")
    parser.add_argument("--patch_size", default="3,50,50", type=list_of_ints)
    parser.add_argument("--wandb_project", default="xxx", type=str)
    parser.add_argument("--wandb_entity", default="xxx", type=str)
    parser.add_argument("--innerLoop", default=inner, type=int)
    parser.add_argument("--dataset", default="bridge_orig", type=str)
    parser.add_argument("--resize_patch", type=str2bool, default=False)
    # additions
    parser.add_argument("--vla_path", default=None, type=str,
                        help="local OpenVLA checkpoint dir, or random:openvla-7b | random:tiny | surrogate (no network here)")
    parser.add_argument("--data", default="synthetic", type=str, help="data source; only 'synthetic' exists in this image")
    parser.add_argument("--colorjitter", type=str2bool, default=False,
                        help="training steps paste a per-image brightness / contrast / saturation variant of the patch")
    parser.add_argument("--colorjitter_strength", type=three_floats, default=(0.2, 0.2, 0.2),
                        help="brightness,contrast,saturation strengths s: factors ~ U(1-s, 1+s)")
    parser.add_argument("--train_crop", choices=("none", "center", "random"), default="none",
                        help="training steps crop the pasted frames as the evaluation does (center: its centre box; random: the same side at a "
                             "random offset per image) and resize back; validation passes use the centre box")
    parser.add_argument("--train_crop_scale", type=float, default=0.9, help="the crop's share of the area, in [0.25, 1] (the evaluation: 0.9)")
    parser.add_argument("--scene_jitter", type=str2bool, nargs="?", const=True, default=False,
                        help="training steps end in a per-image brightness / contrast / saturation / hue draw of the whole pasted frame "
                             "(OpenVLA's image_aug, behind --train_crop); validation passes get none")
    parser.add_argument("--scene_jitter_strength", type=four_floats, default=(0.2, 0.2, 0.2, 0.05),
                        help="B,C,S,H: brightness delta ~ U(-B, B), contrast / saturation factors ~ U(1-s, 1+s), hue ~ U(-H, H) turns")
    parser.add_argument("--defocus_blur", type=str2bool, nargs="?", const=True, default=False,
                        help="training steps blur the whole pasted frame with a per-image Gaussian (camera defocus, in front of --train_crop "
                             "and --scene_jitter); validation passes see the sharp frame")
    parser.add_argument("--defocus_blur_sigma", type=blur_sigma, default=1.0, help="maximum sigma in pixels, in (0, 2.0]: sigma ~ U(0, this) per image")
    parser.add_argument("--tv_weight", type=float, default=0.0, help="weight of the patch's total variation (smoothness) in every training step")
    parser.add_argument("--nps_weight", type=float, default=0.0, help="weight of the patch's non-printability score in every training step")
    parser.add_argument("--nps_palette", type=str, default=None,
                        help="text file of printable colours, one `r g b` in [0,1] per line, '#' comments, at most 64 rows "
                             "(default: the built-in 27-colour grid {0.15,0.5,0.85}^3, a placeholder for a measured printer palette)")


def resolve_device(index: int):
    """`--device N` as the reference uses it (UADA_wrapper.py:52 defaults to GPU 1). On a box with fewer GPUs the run would die with
    'invalid device ordinal' before doing anything; fall back to GPU 0 and say so."""
    import torch

    if not torch.cuda.is_available():
        return torch.device("cpu")
    if index >= torch.cuda.device_count():
        print(f"[vaa] --device {index} does not exist on this host ({torch.cuda.device_count()} GPU(s)) -> using cuda:0")
        index = 0
    return torch.device(f"cuda:{index}")


def resolve_model(args, device):
    """The reference downloads `openvla/...` from the HF hub (UADA_wrapper.py:56-65); offline, a local directory of that
    name is used if present, otherwise the shape-exact random-init model."""
    from .attack.uada_ddp import default_model_factory

    path = args.vla_path
    if path is None:
        hub = vla_path_for(args.dataset)
        path = hub if os.path.isdir(hub) else "random:openvla-7b"
        if path != hub:
            print(f"[vaa] checkpoint {hub!r} not available offline -> random-init OpenVLA-7B-shaped model")
    return default_model_factory(path, device), path


def synthetic_loaders(bs: int, rank: int = 0):
    from .synthetic import SyntheticLoader

    return SyntheticLoader(bs, seed=1234 + 1000003 * rank), SyntheticLoader(bs, seed=99991 + 1000003 * rank)


def maybe_wandb_init(args, name, rank=0):
    if args.wandb_project == "false" or rank != 0:
        return
    try:
        import wandb

        wandb.init(entity=args.wandb_entity, project=args.wandb_project, name=name, tags=args.tags)
        wandb.config = {"iteration": args.iter, "learning_rate": args.lr, "attack_target": args.maskidx, "accumulate_steps": args.accumulate}
    except Exception as e:  # wandb is optional in this image
        print(f"[vaa] wandb unavailable ({e}); continuing with --wandb_project false")
        args.wandb_project = "false"


def new_exp_id() -> str:
    return str(uuid.uuid4())


# ---- VLAAttacker/eval_patch.py: open-loop evaluation of a finished patch ----
def two_ints(arg):
    vals = tuple(map(int, arg.split(",")))
    if len(vals) != 2 or min(vals) < 1:
        raise argparse.ArgumentTypeError("two comma-separated positive integers expected (GX,GY)")
    return vals


def target_arg(arg):
    """`maskidx:value`, e.g. `0:0.5` or `0,1,2:0` -> (maskidx list, target value): TMA's --maskidx / --targetAction pair."""
    try:
        idx, value = arg.split(":")
        return list_of_ints(idx), float(value)
    except ValueError:
        raise argparse.ArgumentTypeError("maskidx:value expected, e.g. 0:0.5 or 0,1,2:0")


def add_eval(parser: argparse.ArgumentParser):
    parser.add_argument("--patch", required=True, type=str, help="a patch.pt written by a wrapper run (fp32 [3,ph,pw])")
    parser.add_argument("--vla_path", default=None, type=str, help="local OpenVLA checkpoint dir, or random:openvla-7b | random:tiny")
    parser.add_argument("--dataset", default="bridge_orig", type=str)
    parser.add_argument("--device", default=0, type=int)
    parser.add_argument("--bs", default=8, type=int, help="(frame, placement) rows per evaluated batch")
    parser.add_argument("--frames", default=16, type=int, help="number of synthetic BridgeData-shaped frames and prompts")
    parser.add_argument("--seed", default=7, type=int)
    parser.add_argument("--center_crop", type=str2bool, nargs="?", const=True, default=True,
                        help="centre crop to 0.9 of the area and resize back (mandatory for the fine-tuned LIBERO checkpoints)")
    parser.add_argument("--crop_scale", default=0.9, type=float)
    # the reference script's placement flags (run_libero_eval_args_geo_batch.py:333-337); angle / shear default to simulation_random_patch's
    parser.add_argument("--geometry", type=str2bool, nargs="?", const=True, default=True)
    parser.add_argument("--angle", default=1, type=float, help="rotation in degrees")
    parser.add_argument("--shx", default=0.1, type=float)
    parser.add_argument("--shy", default=0.1, type=float)
    parser.add_argument("--x", default=2, type=int)
    parser.add_argument("--y", default=2, type=int)
    parser.add_argument("--grid", default=None, type=two_ints, help="GX,GY: a grid of positions over the valid range at that angle and shear")
    parser.add_argument("--target", default=None, type=target_arg, help="maskidx:value — also report how often the patched token hits that action")
    parser.add_argument("--out", default=None, type=str, help="write the report as JSON (tokens included)")
    # the reference's quantised deployment (run_libero_eval_args_geo_batch.py:312-313 -> from_pretrained, openvla_utils.py:43-51)
    parser.add_argument("--load_in_8bit", type=str2bool, nargs="?", const=True, default=False,
                        help="accepted and refused: no bitsandbytes-pinned LLM.int8 exists here; --llm_int8 runs this project's statement of it")
    parser.add_argument("--llm_int8", type=str2bool, nargs="?", const=True, default=False,
                        help="also evaluate the model with its Llama projections as int8 codes, per-call int8 activations and bf16 outlier columns "
                             "(quant.quantize_llm(model, 'int8')) and report both: this project's statement of LLM.int8 (include/vaa_model_ops.h), "
                             "not one pinned against bitsandbytes")
    parser.add_argument("--llm_int8_threshold", default=6.0, type=float,
                        help="a column whose largest |activation| over the rows of a call reaches this is carried in bf16 (transformers' "
                             "llm_int8_threshold; 0: no outlier split)")
    parser.add_argument("--load_in_4bit", type=str2bool, nargs="?", const=True, default=False,
                        help="also evaluate the model with its Llama projections quantised to 4 bits (quant.quantize_llm) and report both")
    parser.add_argument("--bnb_4bit_quant_type", default="fp4", choices=("fp4", "nf4"), help="the 4-bit table (transformers' BitsAndBytesConfig default: fp4)")


def check_eval_quant(parser: argparse.ArgumentParser, args):
    """--load_in_8bit is parsed so that the reference's command lines are understood, and refused: what it asks for is bitsandbytes' LLM.int8,
    and no value here was ever compared with bitsandbytes. --llm_int8 asks for this project's statement of the method;
    together with --load_in_4bit it is an error, as the reference asserts for its two flags."""
    if args.load_in_8bit:
        parser.error("--load_in_8bit is not supported (bitsandbytes' LLM.int8 cannot be pinned here); --llm_int8 evaluates this project's "
                     "statement of the int8 deployment, --load_in_4bit the 4-bit one")
    if args.llm_int8 and args.load_in_4bit:
        parser.error("--llm_int8 and --load_in_4bit exclude each other: one quantised model per run")
    if not 0.0 <= args.llm_int8_threshold < float("inf"):
        parser.error("--llm_int8_threshold must be finite and >= 0")


def add_eval_frame_flags(parser: argparse.ArgumentParser):
    """Recorded camera frames instead of the synthetic ones, and what the reference's simulators do to a frame before the paste
    (experiments/robot/libero/libero_utils.py:44-58, experiments/robot/bridge/bridgev2_utils.py:112)."""
    parser.add_argument("--frames_file", default=None, type=str,
                        help="an .npz with `frames` uint8 [F,H,W,3] and optionally `input_ids` / `attention_mask` int64 [F,T] (right-padded); "
                             "without the prompts, those of the synthetic batch of --seed are used")
    parser.add_argument("--frame_resize", default=None, choices=("lanczos3",),
                        help="resize the file's frames to 224x224 as the simulators' wrappers do (lanczos3 with antialias, round, clip)")
    parser.add_argument("--rotate180", type=str2bool, nargs="?", const=True, default=False,
                        help="rotate every frame by 180 degrees in front of the resize (the LIBERO evaluation does)")
    parser.add_argument("--frame_jpeg", type=str2bool, nargs="?", const=True, default=False,
                        help="JPEG-encode and decode every frame between the rotation and the resize, as LIBERO's resize_image does")
    parser.add_argument("--frame_jpeg_quality", default=95, type=int, help="the quality of --frame_jpeg (1..100; tf.image.encode_jpeg's default: 95)")
    parser.add_argument("--frame_jpeg_compare", type=str2bool, nargs="?", const=True, default=False,
                        help="with --frame_jpeg: run the clean pass once more without the JPEG step and report how often the actions agree")


def load_frames_file(path: str):
    """--frames_file -> (frames uint8 [F,H,W,3] numpy, input_ids | None, attention_mask | None); the prompts are int64 tensors [F,T]."""
    with np.load(path) as z:
        if "frames" not in z.files:
            raise ValueError(f"{path}: no `frames` array")
        frames = np.ascontiguousarray(z["frames"])
        ids = torch.from_numpy(z["input_ids"].astype(np.int64)) if "input_ids" in z.files else None
        mask = torch.from_numpy(z["attention_mask"].astype(np.int64)) if "attention_mask" in z.files else None
    if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
        raise ValueError(f"{path}: `frames` must be uint8 [F,H,W,3], got {frames.dtype} {frames.shape}")
    if (ids is None) != (mask is None):
        raise ValueError(f"{path}: `input_ids` and `attention_mask` come together or not at all")
    if ids is not None and (ids.dim() != 2 or ids.shape != mask.shape or ids.shape[0] != frames.shape[0]):
        raise ValueError(f"{path}: prompts {tuple(ids.shape)} / {tuple(mask.shape)} do not match {frames.shape[0]} frames")
    return frames, ids, mask


def check_eval_frames(parser: argparse.ArgumentParser, args):
    """Reads --frames_file (into args.frames_data) so that a file the command cannot use stops the run before the model loads: frames that
    are not 224x224 need --frame_resize. Without --frames_file the two other flags have nothing to act on."""
    from .constants import IMG

    args.frames_data = None
    if args.frame_jpeg_compare and not args.frame_jpeg:
        parser.error("--frame_jpeg_compare compares with and without the JPEG step: pass --frame_jpeg true")
    if args.frame_jpeg and (args.frames_file is None or args.frame_resize is None):
        parser.error("--frame_jpeg is a step of the simulators' frame resize: it needs --frames_file and --frame_resize lanczos3")
    if args.frame_jpeg and not 1 <= args.frame_jpeg_quality <= 100:
        parser.error("--frame_jpeg_quality must be in 1..100")
    if args.frames_file is None:
        if args.frame_resize is not None or args.rotate180:
            parser.error("--frame_resize / --rotate180 act on the frames of --frames_file")
        return
    try:
        args.frames_data = load_frames_file(args.frames_file)
    except (OSError, ValueError, KeyError) as e:
        parser.error(f"--frames_file: {e}")
    h, w = args.frames_data[0].shape[1:3]
    if args.frame_resize is None:
        if (h, w) != (IMG, IMG):
            parser.error(f"--frames_file {args.frames_file}: the frames are {h}x{w}, not {IMG}x{IMG}: pass --frame_resize lanczos3")
        if args.rotate180:
            parser.error("--rotate180 is part of the frame resize: pass --frame_resize lanczos3")
    elif not (8 <= h <= 2048 and 8 <= w <= 2048):
        parser.error(f"--frames_file {args.frames_file}: {h}x{w} frames are outside what --frame_resize takes (8 to 2048 per side)")


def eval_placements(args, ph: int, pw: int):
    """One (geometry, angle, shx, shy, x, y) from the flags, or with --grid GX,GY the GX x GY positions spread evenly over the valid range
    [0, 224 - pw] x [0, 224 - ph], row-major (y outer); an axis with one point keeps --x / --y."""
    from .constants import IMG

    if min(args.x, args.y) < 0 or args.x > IMG - pw or args.y > IMG - ph:
        raise ValueError(f"position ({args.x}, {args.y}) leaves the frame for a {ph}x{pw} patch")
    gx, gy = args.grid if args.grid else (1, 1)
    xs = [args.x] if gx == 1 else [int(round(v)) for v in np.linspace(0, IMG - pw, gx)]
    ys = [args.y] if gy == 1 else [int(round(v)) for v in np.linspace(0, IMG - ph, gy)]
    return [(bool(args.geometry), args.angle, args.shx, args.shy, x, y) for y in ys for x in xs]
