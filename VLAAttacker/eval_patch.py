#!/usr/bin/env python3
"""Open-loop evaluation of a finished patch: clean vs patched greedy actions on recorded frames through the evaluation's own image path
(paste at a fixed angle / shear / position, centre crop, processor, predict_action). The placement flags are those of the reference's
experiments/robot/libero/run_libero_eval_args_geo_batch.py:333-337; the simulator itself is out of scope."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roboticattack_amd import cli, ops, synthetic  # noqa: E402
from roboticattack_amd.attack.evaluate import evaluate_patch, to_jsonable  # noqa: E402
from roboticattack_amd.constants import MEAN6, STD6  # noqa: E402
from roboticattack_amd.transform import RandomPatchTransform  # noqa: E402


def arg_parser(argv=None):
    parser = argparse.ArgumentParser(description=__doc__)
    cli.add_eval(parser)
    cli.add_eval_frame_flags(parser)
    args = parser.parse_args(argv)
    cli.check_eval_quant(parser, args)
    cli.check_eval_frames(parser, args)
    return args


def main(argv=None):
    args = arg_parser(argv)
    cli.set_seed(args.seed)
    device = cli.resolve_device(args.device)
    patch = torch.load(args.patch, map_location="cpu")
    if not isinstance(patch, torch.Tensor) or patch.dim() != 3 or patch.shape[0] != 3:
        raise ValueError(f"{args.patch}: expected a [3,ph,pw] tensor")
    placements = cli.eval_placements(args, int(patch.shape[1]), int(patch.shape[2]))
    vla, path = cli.resolve_model(args, device)
    vla_q4 = None
    if args.load_in_4bit:  # a second model whose Llama projections are 4-bit codes; towers, projector, embeddings and head are copies
        import copy

        from roboticattack_amd.quant import quantize_llm

        vla_q4 = quantize_llm(copy.deepcopy(vla), args.bnb_4bit_quant_type)
    elif args.llm_int8:  # likewise with int8 codes, per-call int8 activations and bf16 outlier columns (this project's statement of LLM.int8)
        import copy

        from roboticattack_amd.quant import quantize_llm

        vla_q4 = quantize_llm(copy.deepcopy(vla), "int8", threshold=args.llm_int8_threshold)
    source = {}
    if args.frames_data is None:
        frames, input_ids, attention_mask = synthetic.synth_eval_batch(args.seed, args.frames)
    else:  # recorded frames; their prompts, or the synthetic batch's
        frames, input_ids, attention_mask = args.frames_data
        args.frames = int(frames.shape[0])
        if input_ids is None:
            _, input_ids, attention_mask = synthetic.synth_eval_batch(args.seed, args.frames)
        source = dict(frames_file=args.frames_file, source_size=[int(frames.shape[1]), int(frames.shape[2])], frame_resize=args.frame_resize,
                      rotate180=bool(args.rotate180), frame_jpeg=int(args.frame_jpeg_quality) if args.frame_jpeg else None)
    target = (args.target[0], args.target[1]) if args.target else None
    jpeg = dict(jpeg_quality=int(args.frame_jpeg_quality), jpeg_compare=bool(args.frame_jpeg_compare)) if args.frame_jpeg else {}
    report = evaluate_patch(vla, RandomPatchTransform(device), frames, input_ids, attention_mask, patch.float(), placements,
                            center_crop=args.center_crop, crop_scale=args.crop_scale, mean=[MEAN6[:3], MEAN6[3:]], std=[STD6[:3], STD6[3:]],
                            target=target, bs=args.bs, quant_model=vla_q4, resize=args.frame_resize, rot180=bool(args.rotate180), **jpeg)
    torch.cuda.synchronize()
    ops.async_error_check()
    for (geo, angle, shx, shy, x, y), r in zip(report["placements"], report["per_placement"]):
        hit = "" if "target_hit_rate" not in r else " target_hit=" + ",".join(f"{v:.3f}" for v in r["target_hit_rate"].tolist())
        print(f"placement x={x} y={y} angle={angle:g} shx={shx:g} shy={shy:g} geometry={int(geo)}: any_flip={r['any_flip_rate']:.3f} "
              f"flip=" + ",".join(f"{v:.3f}" for v in r["token_flip_rate"].tolist()) + " nad=" + ",".join(f"{v:.4f}" for v in r["nad"].tolist()) + hit)
    o = report["overall"]
    print(f"overall ({len(placements)} placements x {args.frames} frames, model {path}): any_flip={o['any_flip_rate']:.3f} "
          f"mean_nad={float(o['nad'].mean()):.4f}")
    if vla_q4 is not None:
        q, ca = report["quantised"], report["clean_agreement"]
        name = f"8-bit (int8, threshold {args.llm_int8_threshold:g})" if q["quant_type"] == "int8" else f"4-bit ({q['quant_type']})"
        print(f"{name} model: any_flip={q['overall']['any_flip_rate']:.3f} mean_nad={float(q['overall']['nad'].mean()):.4f}; "
              f"clean actions equal to the bf16 model's on {ca['frames']:.3f} of the frames, {ca['tokens']:.3f} of the tokens")
    if "jpeg_agreement" in report:
        ja = report["jpeg_agreement"]
        print(f"JPEG step (quality {args.frame_jpeg_quality}): clean actions equal to those without it on {ja['frames']:.3f} of the frames, "
              f"{ja['tokens']:.3f} of the tokens")
    out = to_jsonable(dict(report, patch=args.patch, vla_path=path, frames=args.frames, center_crop=bool(args.center_crop),
                           crop_scale=args.crop_scale, **source))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f)
        print(f"wrote {args.out}")
    return out


if __name__ == "__main__":
    main()
