"""ms per OpenVLAShaped.predict_action at the 7B shape (random:openvla-7b, prompts of 28-36 tokens, action_dim 7) for bs = 1 and bs = 8, five ways:

    kernel    KV cache + vaa_model_attention_decode (the default)
    stock     KV cache + the stock formulation of the decode step (VAA_NO_FUSED_ATTENTION=1: rotate_half, index_put, masked SDPA)
    no_cache  VAA_PREDICT_NO_CACHE=1: action_dim full forward calls (what the code before predict_action could do)
    q4        the kernel route on the model after quant.quantize_llm(model, --quant_type): vaa_model_q4_gemv in the decode steps, dequant + GEMM
              in the prefill. This child also prints torch.cuda.memory_allocated before and after the conversion and, from one more
              predict_action per bs under the library's per-dispatch timer, the GEMV's median microseconds for the four projection shapes
              with the fraction of 8 TB/s their codes + scales bytes amount to.
    q8        the kernel route on the model after quant.quantize_llm(model, "int8", threshold=--int8_threshold): per projection
              vaa_model_q8_act_quant + vaa_model_q8_matmul (split-K form in the decode steps, tiled integer GEMM in the prefill). Memory before
              and after as for q4, and per projection shape the median microseconds of the split-K matmul (with the fraction of 8 TB/s its
              codes + scales amount to), of the quantise launch in front of it, and of the prefill's GEMM dispatch.

    python tools/predict_bench.py [--iters 5] [--warmup 2] [--bs 1,8] [--out file.json]

Every setting runs in a fresh child process under `timeout` (the switches are read from the environment), one after the other; the first child
that fails ends the run. Prints one JSON line per (setting, bs) and a summary line with the ratios.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = {"kernel": {}, "stock": {"VAA_NO_FUSED_ATTENTION": "1"}, "no_cache": {"VAA_PREDICT_NO_CACHE": "1"}, "q4": {}, "q8": {}}
HBM_BYTES_PER_S = 8e12


def _by_projection(us, shapes, nbytes=None):
    """Dispatch times that come in the order qkv, o, gate+up, down per layer (and step) -> per projection shape: count, median, minimum."""
    out = {}
    for i, (what, N, K) in enumerate(shapes):
        ts = sorted(us[i::4])
        if not ts:
            continue
        med = ts[len(ts) // 2]
        out[what] = dict(N=N, K=K, dispatches=len(ts), us_median=round(med, 2), us_min=round(ts[0], 2))
        if nbytes is not None:
            out[what].update(bytes=nbytes(N, K), hbm_fraction=round(nbytes(N, K) / (med * 1e-6) / HBM_BYTES_PER_S, 3))
    return out


def q8_dispatches(model, ids, mask, pix, bs):
    """One predict_action under vaa_prof_*: per projection shape the split-K matmul of the decode steps (against the bytes of its codes and
    scales), the one-launch quantise in front of it, and the prefill's GEMM with its three quantise launches."""
    from roboticattack_amd import ops

    cfg = model.cfg
    d, mlp = cfg.llm_dim, cfg.llm_mlp
    shapes = (("qkv", 3 * d, d), ("o", d, d), ("gate_up", 2 * mlp, d), ("down", d, mlp))
    ops.prof_start(32768)
    model.predict_action(ids, mask, pix)
    prof = ops.prof_collect()
    pick = lambda key: [t for name, t in prof if key in name]
    return dict(matmul=_by_projection(pick("q8_gemv"), shapes, lambda N, K: N * K + N * 4),
                act_quant=_by_projection(pick("q8_rows_kernel<false>"), shapes),
                prefill_gemm=_by_projection(pick("q8_gemm"), shapes),
                prefill_act_quant_us_total=round(sum(pick("q8_colflag") + pick("q8_rows_kernel<true>") + pick("q8_compact")), 2),
                prefill_gemm_us_total=round(sum(pick("q8_gemm")), 2))


def gemv_dispatches(model, ids, mask, pix, bs):
    """One predict_action under vaa_prof_*: the q4_gemv_kernel dispatches come in the order qkv, o, gate+up, down per layer and step."""
    from roboticattack_amd import ops

    cfg = model.cfg
    d, mlp = cfg.llm_dim, cfg.llm_mlp
    shapes = (("qkv", 3 * d, d), ("o", d, d), ("gate_up", 2 * mlp, d), ("down", d, mlp))
    ops.prof_start(16384)
    model.predict_action(ids, mask, pix)
    us = [t for name, t in ops.prof_collect() if "q4_gemv" in name]
    out = {}
    for i, (what, N, K) in enumerate(shapes):
        ts = sorted(us[i::4])
        med = ts[len(ts) // 2]
        nbytes = N * K // 2 + N * K // 64 * 4
        out[what] = dict(N=N, K=K, dispatches=len(ts), us_median=round(med, 2), us_min=round(ts[0], 2), bytes=nbytes,
                         hbm_fraction=round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3))
    return out


def child(setting: str, batches, iters: int, warmup: int, quant_type: str = "fp4", int8_threshold: float = 6.0) -> int:
    import torch

    from roboticattack_amd.constants import BOS_ID, PAD_ID
    from roboticattack_amd.openvla_model import build_openvla, openvla_7b_cfg

    dev = torch.device("cuda:0")
    model = build_openvla(openvla_7b_cfg(), device=dev, dtype=torch.bfloat16)
    if setting in ("q4", "q8"):
        from roboticattack_amd import quant

        torch.cuda.synchronize()
        before, llm_before = torch.cuda.memory_allocated(), quant.llm_weight_bytes(model)
        if setting == "q8":
            quant_type = "int8"
            quant.quantize_llm(model, "int8", threshold=int8_threshold)
        else:
            quant.quantize_llm(model, quant_type)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        print(json.dumps(dict(setting=setting, quant_type=quant_type, memory_allocated_before=before, memory_allocated_after=torch.cuda.memory_allocated(),
                              llm_bytes_before=llm_before, llm_bytes_after=quant.llm_weight_bytes(model))), flush=True)
    for bs in batches:
        g = torch.Generator().manual_seed(100 + bs)
        lens = torch.randint(28, 37, (bs,), generator=g)
        L = int(lens.max())
        ids = torch.randint(3, 31000, (bs, L), generator=g)
        ids[:, 0] = BOS_ID
        mask = torch.arange(L)[None, :] < lens[:, None]
        ids = torch.where(mask, ids, torch.full_like(ids, PAD_ID)).to(dev)
        mask = mask.long().to(dev)
        pix = torch.randn((bs, 6, 224, 224), generator=g).to(torch.bfloat16).to(dev)
        for _ in range(warmup):
            tokens, _ = model.predict_action(ids, mask, pix)
        torch.cuda.synchronize()
        times = []
        for _ in range(iters):
            t0 = time.perf_counter()
            tokens, _ = model.predict_action(ids, mask, pix)  # returns after the tokens reached the host (the actions are host values)
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        print(json.dumps(dict(setting=setting, bs=bs, ms_median=round(times[len(times) // 2], 3), ms_min=round(times[0], 3), ms_max=round(times[-1], 3),
                              iters=iters, tokens_row0=tokens[0].tolist())), flush=True)
        if setting == "q4":
            print(json.dumps(dict(setting=setting, bs=bs, gemv=gemv_dispatches(model, ids, mask, pix, bs))), flush=True)
        if setting == "q8":
            print(json.dumps(dict(setting=setting, bs=bs, q8=q8_dispatches(model, ids, mask, pix, bs))), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bs", default="1,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--quant_type", default="fp4", choices=("fp4", "nf4"), help="the table of the q4 setting")
    ap.add_argument("--int8_threshold", type=float, default=6.0, help="the outlier threshold of the q8 setting")
    ap.add_argument("--settings", default=",".join(SETTINGS), help="comma-separated subset of " + ",".join(SETTINGS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    batches = [int(b) for b in a.bs.split(",")]
    if a.child:
        return child(a.child, batches, a.iters, a.warmup, a.quant_type, a.int8_threshold)
    res, extra = {}, []
    chosen = [n for n in SETTINGS if n in a.settings.split(",")]
    for name in chosen:
        env = SETTINGS[name]
        e = {k: v for k, v in os.environ.items() if k not in ("VAA_NO_FUSED_ATTENTION", "VAA_PREDICT_NO_CACHE", "VAA_NO_FUSED_MODEL_OPS")}
        e.update(env)
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--bs", a.bs, "--quant_type", a.quant_type, "--int8_threshold", str(a.int8_threshold)]
        p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stderr[-4000:])
            print(json.dumps(dict(setting=name, failed=p.returncode)))
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                if "ms_median" in d:
                    res[(d["setting"], d["bs"])] = d
                else:
                    extra.append(d)
    summary = {}
    for bs in batches:
        ms = {x: res[(x, bs)]["ms_median"] for x in chosen}
        row = {x + "_ms": v for x, v in ms.items()}
        if "kernel" in ms:
            row.update({x + "_over_kernel": round(ms[x] / ms["kernel"], 3) for x in ms if x != "kernel"})
        summary["bs%d" % bs] = row
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(results=[v for v in res.values()] + extra, summary=summary), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
