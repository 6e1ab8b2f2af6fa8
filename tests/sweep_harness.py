"""What the sweep test files share (a plain module, not a conftest): the host-side attacker / wrapper builders of test_*sweep_host.py and the
product-run harness of test_gpu_*sweep.py on the setup of the reference-loop goldens (traj_ddp_k3s.npz, traj_ddp2_k3s.npz)."""
import importlib.util
import os
import random
import socket

import numpy as np
import torch

from conftest import ROOT
from roboticattack_amd import synthetic
from roboticattack_amd.attack import uada_ddp

DEV = "cuda:0"
ENV_SWITCHES = ("VAA_FULL_CE_EVERY_STEP", "VAA_HEAD_EVERY_STEP", "VAA_K3_ONE_PASS", "VAA_K3_CE_FOLD_WG", "VAA_FUSED_EPILOGUE", "VAA_FUSED_EMBED_GRAD",
                "VAA_FUSED_HEAD")


# ---- host side ----
def wrapper(name):
    """VLAAttacker/UADA_wrapper_ddp.py imported as a module of its own called `name`."""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "VLAAttacker", "UADA_wrapper_ddp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def attacker(monkeypatch, tmp_path, model="head", **kw):
    """A CPU attacker over a surrogate that exposes the fused path's hooks ("head") or does not ("plain")."""
    from roboticattack_amd.surrogate import SurrogateHeadVLA, SurrogateVLA

    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0").items():
        monkeypatch.setenv(k, v)
    factory = (lambda p, d: SurrogateHeadVLA(seed=1)) if model == "head" else (lambda p, d: SurrogateVLA(seed=1))
    args = dict(vla_path="x", dataset_name="synthetic", save_dir=str(tmp_path), patch_size=[3, 50, 50], bs=3, use_wandb=False, device="cpu",
                model_factory=factory, dataset_factory=lambda *a: (None, None))
    args.update(kw)
    return uada_ddp.OpenVLAAttacker(**args)


def fused(monkeypatch):
    """The fused path's availability without a GPU: decided by the model's hooks and resize_patch alone."""
    monkeypatch.delenv("VAA_FUSED_EPILOGUE", raising=False)
    monkeypatch.delenv("VAA_FUSED_EMBED_GRAD", raising=False)
    monkeypatch.setattr(uada_ddp.OpenVLAAttacker, "fused_ddp_available", lambda self: hasattr(self.vla, "hidden_rows")
                        and hasattr(self.vla, "patch_embed_params") and not self.randomPatchTransform.resize_patch)


# ---- product runs on the GPU ----
class Fresh:
    def __init__(self, seeds, b, kind="smooth"):
        self.seeds, self.b, self.kind = seeds, b, kind

    def __iter__(self):
        for s in self.seeds:
            yield synthetic.synth_batch(s, self.b, self.kind)


def seed():
    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def env(monkeypatch, gemm_head=False):
    """The environment of a one-rank run in this process; `gemm_head`: VAA_FUSED_HEAD=0."""
    for k, v in dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port())).items():
        monkeypatch.setenv(k, v)
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if gemm_head:
        monkeypatch.setenv("VAA_FUSED_HEAD", "0")


def worker_env(rank, world, port):
    """The environment of one rank of an mp.spawn worker (gloo: several ranks on one GPU)."""
    import sys

    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), VAA_DIST_BACKEND="gloo")
    for k in ENV_SWITCHES:
        os.environ.pop(k, None)


def spawn2(worker, *args):
    """`worker(rank, 2, port, *args)` on two ranks."""
    import torch.multiprocessing as mp

    mp.spawn(worker, args=(2, free_port()) + args, nprocs=2, join=True)


def run(d, save_dir, attack_type="UADA", rank=0, world=1, nval=None, **kw):
    """One product run of the data-parallel loop on the golden's setup (its sizes, seeds and schedule): a standalone run or, with one of the sweep
    parameters in `kw`, a sweep. Returns (the patches after every inner step [steps, P, 3, 50, 50] — behind the step itself where AdamW ran inside
    its epilogue, else behind K4 —, host logs per outer iteration, attacker, kernel names of the TRAINING steps, call counts of the training steps:
    the GEMM head's forward, the UPA sweep's K3, the head backward, K4 as a launch of its own)."""
    from roboticattack_amd import ops, optim
    from roboticattack_amd.surrogate import SurrogateHeadVLA

    n_it, inner, bs = int(d["num_iter"]), int(d["inner"]), int(d["bs"])
    nval = int(d["val_batches"]) if nval is None else nval
    snaps, logs, names = [], [], []
    counts = dict(head=0, k3=0, back=0, k4=0)

    def snap(patch):
        snaps.append(patch.detach().cpu().numpy().copy().reshape((-1, 3, 50, 50)))

    class Att(uada_ddp.OpenVLAAttacker):
        val_batches = 100

        def fused_ddp_step(self, pixel_values, patch, *a, **k):
            r = super().fused_ddp_step(pixel_values, patch, *a, **k)
            if world == 1:  # AdamW ran inside the epilogue
                snap(patch)
            return r

        def sweep_step(self, img, patches, *a, **k):
            r = super().sweep_step(img, patches, *a, **k)
            if world == 1 and self.sweep_kind.k4_in_epilogue:
                snap(patches)
            return r

        def assert_finite_state(self, patch, optimizer, host, where, **k):
            logs.append(np.array(host, dtype=np.float64).copy())
            return super().assert_finite_state(patch, optimizer, host, where, **k)

        def _val(self, f, *a):  # the kernel trace covers the training steps only
            names.extend(nm for nm, _ in ops.prof_collect())
            r = f(*a)
            ops.prof_start(8192)
            return r

        def validate(self, *a):
            return self._val(super().validate, *a)

        def validate_sweep(self, *a):
            return self._val(super().validate_sweep, *a)

    def k4(self, *a, **k):  # every step that goes through K4 as a launch of its own (world > 1; the unfused standalone loop; UPA's clip)
        r = orig["step"](self, *a, **k)
        counts["k4"] += 1
        snap(self.patch)
        return r

    def count(key):
        def g(*a, **k):
            counts[key] += 1
            return orig[key](*a, **k)

        return g

    orig = dict(step=optim.PatchOptimizer.step, head=ops._head_seg_forward, k3=ops.loss_rows_fwd_bwd_seg_upa, back=ops._loss_backward)
    optim.PatchOptimizer.step = k4
    ops._head_seg_forward, ops.loss_rows_fwd_bwd_seg_upa, ops._loss_backward = count("head"), count("k3"), count("back")
    try:
        args = dict(vla_path="x", dataset_name="synthetic", save_dir=save_dir, patch_size=[3, 50, 50], lr=float(d["lr"]), bs=bs, warmup=int(d["warmup"]),
                    num_iter=n_it, maskidx=[0], innerLoop=inner, geometry=True, use_wandb=False, MSE_weights=int(d["MSE_weights"]),
                    device=torch.device(DEV), attack_type=attack_type,
                    model_factory=lambda path, dev: SurrogateHeadVLA(seed=int(d["model_seed"])).to(dev),
                    dataset_factory=lambda name, b, r, w: (Fresh([int(d["train_seed0"]) + w * i + r for i in range(n_it)], bs),
                                                           Fresh([int(d["val_seed0"]) + w * i + r for i in range(nval)], bs)))
        args.update(kw)
        att = Att(**args)
        seed()
        ops.prof_start(8192)
        att.attack(rank, world)
        names.extend(nm for nm, _ in ops.prof_collect())
    finally:
        optim.PatchOptimizer.step = orig["step"]
        ops._head_seg_forward, ops.loss_rows_fwd_bwd_seg_upa, ops._loss_backward = orig["head"], orig["k3"], orig["back"]
    return np.stack(snaps), np.stack(logs), att, names, counts
