"""ms per OpenVLAShaped.predict_action at the 7B shape (random:openvla-7b, prompts of 28-36 tokens, action_dim 7) for bs = 1 and bs = 8, three ways:

    kernel    KV cache + vaa_model_attention_decode (the default)
    stock     KV cache + the stock formulation of the decode step (VAA_NO_FUSED_ATTENTION=1: rotate_half, index_put, masked SDPA)
    no_cache  VAA_PREDICT_NO_CACHE=1: action_dim full forward calls (what the code before predict_action could do)

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

SETTINGS = {"kernel": {}, "stock": {"VAA_NO_FUSED_ATTENTION": "1"}, "no_cache": {"VAA_PREDICT_NO_CACHE": "1"}}


def child(setting: str, batches, iters: int, warmup: int) -> int:
    import torch

    from roboticattack_amd.constants import BOS_ID, PAD_ID
    from roboticattack_amd.openvla_model import build_openvla, openvla_7b_cfg

    dev = torch.device("cuda:0")
    model = build_openvla(openvla_7b_cfg(), device=dev, dtype=torch.bfloat16)
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
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bs", default="1,8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    batches = [int(b) for b in a.bs.split(",")]
    if a.child:
        return child(a.child, batches, a.iters, a.warmup)
    res = {}
    for name, env in SETTINGS.items():
        e = {k: v for k, v in os.environ.items() if k not in ("VAA_NO_FUSED_ATTENTION", "VAA_PREDICT_NO_CACHE", "VAA_NO_FUSED_MODEL_OPS")}
        e.update(env)
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(a.iters),
               "--warmup", str(a.warmup), "--bs", a.bs]
        p = subprocess.run(cmd, env=e, cwd=ROOT, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:  # nothing more is started on the GPU after a failure
            sys.stderr.write(p.stderr[-4000:])
            print(json.dumps(dict(setting=name, failed=p.returncode)))
            return 1
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                res[(d["setting"], d["bs"])] = d
    summary = {}
    for bs in batches:
        k, s, n = (res[(x, bs)]["ms_median"] for x in ("kernel", "stock", "no_cache"))
        summary["bs%d" % bs] = dict(kernel_ms=k, stock_ms=s, no_cache_ms=n, no_cache_over_kernel=round(n / k, 2), stock_over_kernel=round(s / k, 3))
    print(json.dumps(dict(summary=summary)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(results=[v for v in res.values()], summary=summary), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
