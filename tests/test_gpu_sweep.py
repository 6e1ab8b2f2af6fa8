"""GPU tests of the maskidx sweep (P patch groups optimised in one step of the data-parallel UADA loop).

Kernels: the segmented row map through K3s / K3h and the segmented step epilogue give every group the bits of the same calls on that group
alone; the segmented K4 the bits of P separate K4 launches. Loop: a sweep over SurrogateHeadVLA replays the reference-loop golden of the headline
loop in group 0, and every other group the standalone product run of its maskidx."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import c_oracle
from roboticattack_amd import synthetic
from sweep_harness import DEV, env, run, spawn2, worker_env

pytestmark = pytest.mark.gpu
V = 32064
SWEEP = [[0], [0, 1], [0, 1, 2, 3, 4, 5, 6]]


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _rows(labels):
    B, L = labels.shape
    return [(b, 256 + k) for b in range(B) for k in range(L - 1) if labels[b, k + 1] != -100]


def _slice_stats(ws, R, r0, r1):
    """Rows r0..r1 of the SliceStats ({alse, E, pred, pad}) in a K3 workspace laid out for R rows."""
    return ws[R * 4 * 16 : R * 4 * 16 + R * 16].view(torch.int32).view(R, 4)[r0:r1]


def _case(ops, Bp, D, seed):
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(seed, Bp)
    groups = [mask_labels(labels.clone(), m) for m in SWEEP]
    lab_all = torch.cat(groups).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    W = (torch.randn(V, D, device=DEV, generator=g) * (1.3 / np.sqrt(D))).to(torch.bfloat16)
    W[31744:32000] *= 2.0
    counts = [len(_rows(x.numpy())) for x in groups]
    r0 = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    h = torch.randn(int(r0[-1]), D, device=DEV, generator=g).to(torch.bfloat16)
    return groups, lab_all, W, h, r0


@pytest.mark.parametrize("Bp,D", [(4, 256), (3, 4096)])
def test_segmented_k3s_k3h_and_epilogue_bitwise_per_group(ops, Bp, D):
    P = len(SWEEP)
    groups, lab_all, W, h, r0 = _case(ops, Bp, D, 41 + Bp)
    R = int(r0[-1])
    L = lab_all.shape[1]
    seg = ops.LossRowMapSeg(lab_all, P)
    kw = dict(w=5.0)
    n = 3 * 50 * 50
    gen = torch.Generator(device=DEV).manual_seed(7)
    partials = torch.randn(P * Bp, n, device=DEV, generator=gen) * 1e-3
    patch0 = torch.rand(P * n, device=DEV, generator=gen)
    m0 = torch.randn(P * n, device=DEV, generator=gen) * 1e-4
    v0 = torch.rand(P * n, device=DEV, generator=gen) * 1e-7

    def k3(hh, rm, full_ce):
        o = ops.head_slice_fwd_bwd(hh, W, rm, ops.LOSS_UADA_DDP, want_dh=True, want_scalars=False, want_grad_slice=True, **kw)
        if full_ce:
            ops.head_loss_rows_stats(hh, W, rm, ops.LOSS_UADA_DDP, **kw)
        return o["dh"].clone(), o["grad_slice"].clone(), o["ws"].clone()

    def upd_args(patch, m, v, sp):
        return dict(patch=patch, m=m, v=v, mode=ops.OPT_ADAMW_HF, lr=2e-3, step=3, stat_part=sp)

    for full_ce in (False, True):
        dh, gs, ws = k3(h, seg, full_ce)
        nred = (n + 63) // 64
        # segmented epilogue: pass-through (zero tail), fold, fold + update
        msg_pt = torch.full((P * (n + 4),), 7.0, device=DEV)
        sc_pt = torch.full((P, 8), 3.0, device=DEV)
        ops.step_epilogue_seg(partials, msg_pt, sc_pt, P)
        msg = torch.zeros(P * (n + 4), device=DEV)
        sc = torch.zeros((P, 8), device=DEV)
        pred, pf = ops.step_epilogue_seg(partials, msg, sc, P, rowmap=seg, R=R, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws, **kw)
        pu, mu, vu = patch0.clone(), m0.clone(), v0.clone()
        spu = torch.zeros((P * nred, 2), dtype=torch.float64, device=DEV)
        msg_u = torch.zeros(P * (n + 4), device=DEV)
        sc_u = torch.zeros((P, 8), device=DEV)
        pred_u, _ = ops.step_epilogue_seg(partials, msg_u, sc_u, P, rowmap=seg, R=R, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws, update=upd_args(pu, mu, vu, spu), **kw)
        torch.cuda.synchronize()
        ops.async_error_check()
        assert torch.equal(msg_pt[P * n :], torch.zeros(4 * P, device=DEV)) and torch.equal(sc_pt, torch.full((P, 8), 3.0, device=DEV))
        assert torch.equal(msg_pt[: P * n], msg[: P * n]) and torch.equal(msg_u, msg) and torch.equal(sc_u, sc) and torch.equal(pred_u, pred)
        for g, m in enumerate(SWEEP):
            a, b = int(r0[g]), int(r0[g + 1])
            rm_g = ops.LossRowMap(groups[g].to(DEV))
            dh_g, gs_g, ws_g = k3(h[a:b].contiguous(), rm_g, full_ce)
            assert torch.equal(_bits(dh[a:b]), _bits(dh_g)) and torch.equal(_bits(gs[a:b]), _bits(gs_g)), (g, full_ce)
            assert torch.equal(_slice_stats(ws, R, a, b), _slice_stats(ws_g, b - a, 0, b - a))
            assert float(gs_g.float().abs().max()) > 0
            # the standalone epilogue on the group's partials and rows
            pg = partials[g * Bp : (g + 1) * Bp].contiguous()
            msg_g = torch.zeros(n + 4, device=DEV)
            sc_g = torch.zeros(8, device=DEV)
            pred_g, pf_g = ops.step_epilogue(pg, msg_g, sc_g, rowmap=rm_g, R=b - a, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws_g, **kw)
            p_g, m_g, v_g = patch0[g * n : (g + 1) * n].clone(), m0[g * n : (g + 1) * n].clone(), v0[g * n : (g + 1) * n].clone()
            sp_g = torch.zeros((nred, 2), dtype=torch.float64, device=DEV)
            msg_gu = torch.zeros(n + 4, device=DEV)
            ops.step_epilogue(pg, msg_gu, torch.zeros(8, device=DEV), rowmap=rm_g, R=b - a, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws_g,
                              update=upd_args(p_g, m_g, v_g, sp_g), **kw)
            torch.cuda.synchronize()
            assert torch.equal(msg[g * n : (g + 1) * n], msg_g[:n]) and torch.equal(msg[P * n + 4 * g : P * n + 4 * g + 4], msg_g[n:]), (g, full_ce)
            assert torch.equal(sc[g], sc_g), (g, sc[g], sc_g)
            assert torch.equal(pred[g * Bp : (g + 1) * Bp], pred_g) and torch.equal(pf[g * Bp : (g + 1) * Bp], pf_g)
            assert torch.equal(pu[g * n : (g + 1) * n], p_g) and torch.equal(mu[g * n : (g + 1) * n], m_g) and torch.equal(vu[g * n : (g + 1) * n], v_g)
            assert torch.equal(spu[g * nred : (g + 1) * nred], sp_g)
            assert float(sc_g[6]) == Bp * len(m) and (float(sc_g[1]) > 0) == full_ce
            if full_ce:  # the group's scalars against the C oracle on the group alone (the bf16 logits K3h made of its rows)
                _, _, _, _, lg = ops.head_loss_rows_fwd_bwd(h[a:b].contiguous(), W, rm_g, ops.LOSS_UADA_DDP, want_grad=False, want_logits=True, **kw)
                rows = _rows(groups[g].numpy())
                rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
                full = torch.zeros((Bp, 256 + L, V), dtype=torch.float32)
                full[torch.from_numpy(rb), torch.from_numpy(rp)] = lg.float().cpu()
                so, _ = c_oracle.loss(full.numpy(), groups[g].numpy(), c_oracle.MODE_UADA_DDP, **kw)
                got = sc_g.cpu().numpy()
                assert np.allclose(got[[0, 1, 2]], so[[0, 1, 2]], rtol=3e-5, atol=3e-5), (got, so)  # total, CE, w^2 MSE


def test_unsegmented_map_through_new_entry_points_gives_old_bits(ops):
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(5, 6)
    labels = mask_labels(labels, [0, 1, 2]).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    D = 512
    W = (torch.randn(V, D, device=DEV, generator=g) * (1.3 / np.sqrt(D))).to(torch.bfloat16)
    rm, seg1 = ops.LossRowMap(labels), ops.LossRowMapSeg(labels, 1)
    R = len(_rows(labels.cpu().numpy()))
    h = torch.randn(R, D, device=DEV, generator=g).to(torch.bfloat16)
    o1 = ops.head_slice_fwd_bwd(h, W, rm, ops.LOSS_UADA_DDP, want_dh=True, want_scalars=False, want_grad_slice=True)
    dh1, gs1, ws1 = o1["dh"].clone(), o1["grad_slice"].clone(), o1["ws"].clone()
    o2 = ops.head_slice_fwd_bwd(h, W, seg1, ops.LOSS_UADA_DDP, want_dh=True, want_scalars=False, want_grad_slice=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dh1), _bits(o2["dh"])) and torch.equal(_bits(gs1), _bits(o2["grad_slice"]))
    n = 7500
    parts = torch.randn(6, n, device=DEV, generator=g)
    for rowmap in (rm, seg1):  # an ordinary map with P = 1, and a one-group segmented map
        msg_a, sc_a = torch.zeros(n + 4, device=DEV), torch.zeros(8, device=DEV)
        pa, fa = ops.step_epilogue(parts, msg_a, sc_a, rowmap=rm, R=R, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws1)
        msg_b, sc_b = torch.zeros(n + 4, device=DEV), torch.zeros((1, 8), device=DEV)
        pb, fb = ops.step_epilogue_seg(parts, msg_b, sc_b, 1, rowmap=rowmap, R=R, V=V, mode=ops.LOSS_UADA_DDP, loss_ws=ws1)
        torch.cuda.synchronize()
        assert torch.equal(msg_a, msg_b) and torch.equal(sc_a, sc_b[0]) and torch.equal(pa, pb) and torch.equal(fa, fb)
    # K4 over P groups == P separate K4 launches (stats included), with the DDP mean and an L1 clip
    P, n = 3, 7500
    grad = torch.randn(P * n, device=DEV, generator=g) * 1e-3
    p0, m0, v0 = torch.rand(P * n, device=DEV, generator=g), torch.zeros(P * n, device=DEV), torch.zeros(P * n, device=DEV)
    for l1 in (0.0, 1e-3):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        st = ops.patch_update_seg(p, grad, m, v, P, ops.OPT_ADAMW_HF, 1e-2, 2, l1_clip=l1, grad_scale=0.5)
        for q in range(P):
            sl = slice(q * n, (q + 1) * n)
            pq, mq, vq = p0[sl].clone(), m0[sl].clone(), v0[sl].clone()
            sq = ops.patch_update(pq, grad[sl].contiguous(), mq, vq, ops.OPT_ADAMW_HF, 1e-2, 2, l1_clip=l1, grad_scale=0.5)
            torch.cuda.synchronize()
            assert torch.equal(p[sl], pq) and torch.equal(m[sl], mq) and torch.equal(v[sl], vq) and torch.equal(st[q], sq)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run(d, save_dir, maskidx=None, sweep=None, **kw):
    """One product run of the data-parallel UADA loop on the golden's setup (sweep_harness.run); returns (per-step patches [steps, P, ...], host
    logs, attacker, kernel names of the training steps)."""
    return run(d, save_dir, maskidx=maskidx if maskidx is not None else [int(v) for v in d["maskidx"]], maskidx_sweep=sweep, **kw)[:4]


def test_sweep_trajectory_vs_reference_loop_and_standalone_runs(tmp_path, monkeypatch):
    """maskidx_sweep=[[0,1], [0], [0,1,2]] over the golden setup of test_ddp_trajectory_k3s_vs_reference_loop (traj_ddp_k3s.npz, SurrogateHeadVLA,
    bs 3 per group): group 0 reproduces the reference loop's trajectory, saved patch, train log and validation averages; groups 1 and 2 their
    standalone product runs; K3s runs once per training step; a one-group sweep is bitwise the existing loop."""
    env(monkeypatch)
    d = np.load(os.path.join(GOLDEN, "traj_ddp_k3s.npz"))
    n_it, inner = int(d["num_iter"]), int(d["inner"])
    sweep = [[0, 1], [0], [0, 1, 2]]
    assert [int(v) for v in d["maskidx"]] == sweep[0]
    snaps, logs, att, names = _run(d, str(tmp_path / "sweep"), sweep=sweep)
    assert snaps.shape == (n_it * inner, 3, 3, 50, 50)
    assert sum("head_slice_kernel" in nm for nm in names) == n_it * inner  # ONE K3s per training step, not P
    assert sum("embed_dgrad" in nm for nm in names) == n_it * inner
    ref = d["patches"]
    err = np.abs(snaps[:, 0] - ref).reshape(len(ref), -1).max(1)
    print("group 0 per-step max |patch - reference|:", ["%.2e" % e for e in err])
    assert err.max() <= 1e-4, err
    assert np.abs(ref[-1] - ref[0]).max() > 5e-3
    last = torch.load(tmp_path / "sweep" / "maskidx0-1" / "last" / "patch.pt").numpy()
    assert np.abs(last - d["last_saved"]).max() <= 1e-4
    for tag in ("maskidx0", "maskidx0-1-2"):
        assert os.path.exists(tmp_path / "sweep" / tag / "last" / "patch.pt") and os.path.exists(tmp_path / "sweep" / tag / "0" / "patch.pt")
    assert logs.shape == (n_it, 3, 4)
    np.testing.assert_allclose(logs[:, 0, 0], d["train_ce"], rtol=3e-4)
    np.testing.assert_allclose(logs[:, 0, 1], d["train_mse"], rtol=2e-3)
    np.testing.assert_allclose(logs[:, 0, 2], d["train_uad"], atol=2e-4)
    np.testing.assert_allclose([att.val_MSE_Distance["maskidx0-1"][0]], d["val_mse"], rtol=2e-3)
    np.testing.assert_allclose([att.val_UAD["maskidx0-1"][0]], d["val_uad"], atol=2e-5)
    np.testing.assert_allclose([att.val_CE_loss["maskidx0-1"][0]], d["val_ce"], rtol=3e-4)
    assert set(att.last_train_log) == {"maskidx0-1", "maskidx0", "maskidx0-1-2"}
    # groups 1 and 2 against standalone product runs of their maskidx with the same seed
    for g in (1, 2):
        s_snaps, s_logs, s_att, _ = _run(d, str(tmp_path / f"solo{g}"), maskidx=sweep[g])
        e = np.abs(snaps[:, g] - s_snaps[:, 0]).reshape(len(ref), -1).max(1)
        print(f"group {g} per-step max |sweep - standalone|:", ["%.2e" % v for v in e])
        assert e.max() <= 1e-4, e
        assert np.abs(s_snaps[-1, 0] - s_snaps[0, 0]).max() > 1e-3
        np.testing.assert_allclose(logs[:, g, 1], s_logs[:, 1], rtol=2e-3)
        np.testing.assert_allclose(logs[:, g, 2], s_logs[:, 2], atol=2e-4)
        np.testing.assert_allclose([att.val_MSE_Distance[att.sweep_tags[g]][0]], [s_att.val_MSE_Distance[0]], rtol=2e-3)
    # a one-group sweep is bitwise the existing loop
    one, one_logs, one_att, _ = _run(d, str(tmp_path / "one"), sweep=[[0, 1]])
    base, base_logs, base_att, _ = _run(d, str(tmp_path / "base"))
    assert np.array_equal(one, base) and np.array_equal(one_logs.reshape(-1, 4), base_logs)
    assert one_att.last_train_log["maskidx0-1"] == base_att.last_train_log
    assert one_att.val_MSE_Distance["maskidx0-1"] == base_att.val_MSE_Distance


def _sweep2_worker(rank, world, port, out_dir, golden_path):
    worker_env(rank, world, port)
    d = np.load(golden_path)
    snaps, logs, att, names = _run(d, os.path.join(out_dir, f"rank{rank}"), sweep=[[0, 1], [0, 1, 2]], rank=rank, world=world)  # snaps: behind every K4
    np.savez(os.path.join(out_dir, f"sweep_r{rank}.npz"), snaps=snaps, logs=logs, n_slice=sum("head_slice_kernel" in n for n in names),
             val=np.array([att.val_MSE_Distance["maskidx0-1"][0], att.val_UAD["maskidx0-1"][0]] if rank == 0 else [0.0, 0.0]))


def test_sweep_two_ranks_group0_vs_reference_loop(tmp_path):
    """Two ranks (gloo on one GPU, as test_ddp_two_rank_trajectory_k3s_vs_reference_loop) of a sweep [[0,1], [0,1,2]]: ONE all-reduce of
    [2 gradients | 2 x 4 scalars] per step and the segmented K4; group 0 reproduces traj_ddp2_k3s.npz, the ranks are bit-identical."""
    golden = os.path.join(GOLDEN, "traj_ddp2_k3s.npz")
    d = np.load(golden)
    n_it, inner = int(d["num_iter"]), int(d["inner"])
    spawn2(_sweep2_worker, str(tmp_path), golden)
    r0, r1 = np.load(tmp_path / "sweep_r0.npz"), np.load(tmp_path / "sweep_r1.npz")
    assert np.array_equal(r0["snaps"], r1["snaps"]) and np.array_equal(r0["logs"], r1["logs"])
    assert int(r0["n_slice"]) == n_it * inner
    ref = d["patches"]
    assert r0["snaps"].shape == (n_it * inner, 2, 3, 50, 50)
    err = np.abs(r0["snaps"][:, 0] - ref).reshape(len(ref), -1).max(1)
    print("group 0 per-step max |patch - reference|:", ["%.2e" % e for e in err])
    assert err.max() <= 1e-4, err
    assert np.abs(r0["snaps"][-1, 1] - r0["snaps"][0, 1]).max() > 1e-3  # group 1 moves too
    np.testing.assert_allclose(r0["logs"][:, 0, 0], d["train_ce"], rtol=3e-4)
    np.testing.assert_allclose(r0["logs"][:, 0, 1], d["train_mse"], rtol=2e-3)
    np.testing.assert_allclose(r0["val"][0], d["val_mse"][0], rtol=2e-3)
    np.testing.assert_allclose(r0["val"][1], d["val_uad"][0], atol=2e-5)
    last = torch.load(tmp_path / "rank0" / "maskidx0-1" / "last" / "patch.pt").numpy()
    assert np.abs(last - d["last_saved"]).max() <= 1e-4 and not os.path.exists(tmp_path / "rank1" / "maskidx0-1")
