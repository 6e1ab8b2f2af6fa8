"""GPU tests of the UPA weight sweep (P (alpha, belta) groups optimised in one step of the data-parallel loop).

Kernels: K3 in LOSS_UPA mode over a segmented row map (vaa_loss_rows_fwd_bwd_seg_upa) gives every group the bits of vaa_loss_rows_fwd_bwd on that
group's rows alone with the group's (alpha, beta), the reference's recorded UPA losses / gradients (tests/golden/k3_upa_*.npz) and the C oracle's;
the pass-through epilogue followed by the segmented K4 with the L1 clip ends the step with the bits of P standalone sequences. Loop: a one-group
sweep is the existing data-parallel UPA loop bit for bit; every group of a three-group sweep over SurrogateHeadVLA follows its standalone run."""
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
PAIRS = [(0.8, 0.2), (0.2, 0.8), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (2.0, 0.05), (0.3, 0.7)]  # far apart, incl. one term switched off


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _rows(labels, S=None):
    B, L = labels.shape
    S = 256 + L if S is None else S
    return [(b, S - L + k) for b in range(B) for k in range(L - 1) if labels[b, k + 1] != -100]


def _logits(R, seed, dtype):
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((R, V)) * 2).astype(np.float32)
    z[:, 31744:32000] += (rs.standard_normal((R, 256)) * 3).astype(np.float32)
    z[::3, 1234] = 40.0  # rows whose top-1 token is not an action token
    return torch.from_numpy(z).to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel, bitwise per group
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("P,Bp", [(1, 5), (2, 4), (3, 6), (7, 3)])  # 40, 64, 144 and 168 labelled rows: two cases beyond K3s's 128
def test_segmented_upa_k3_bitwise_per_group(ops, P, Bp, dtype):
    _, labels, _ = synthetic.synth_text_batch(70 + P, Bp)  # unmasked: 7 action tokens + EOS per image
    L = labels.shape[1]
    Rg = len(_rows(labels.numpy()))
    assert Rg == 8 * Bp
    lab_all = labels.repeat(P, 1).contiguous().to(DEV)
    z = _logits(P * Rg, 100 + 10 * P + Bp, dtype)
    pairs = PAIRS[:P]
    seg = ops.LossRowMapSeg(lab_all, P)
    g = torch.full((P * Rg, 256), float("nan"), dtype=dtype, device=DEV)
    ops.prof_start(64)
    sc, pred, pf, g_out = ops.loss_rows_fwd_bwd_seg_upa(z, seg, P, pairs, w=5.0, grad=g)
    torch.cuda.synchronize()
    names = [nm for nm, _ in ops.prof_collect()]
    ops.async_error_check()
    assert g_out is g
    assert len(names) == 2 and "rows_stats_kernel" in names[0] and "false" in names[0] and "rows_finish_kernel" in names[1]  # two launches for all groups
    assert sc.shape == (P, 8) and torch.isfinite(g.float()).all() and torch.isfinite(sc).all()
    # evaluation only (no gradient): the same scalars and maps
    sc_e, pred_e, pf_e, g_e = ops.loss_rows_fwd_bwd_seg_upa(z, seg, P, pairs, w=5.0, want_grad=False)
    assert g_e is None and torch.equal(_bits(sc_e), _bits(sc)) and torch.equal(pred_e, pred) and torch.equal(pf_e, pf)
    rm_q = ops.LossRowMap(labels.to(DEV))
    for q, (al, be) in enumerate(pairs):
        a, b = q * Rg, (q + 1) * Rg
        zq = z[a:b].contiguous()
        sc_q, pred_q, pf_q, g_q = ops.loss_rows_fwd_bwd(zq, rm_q, ops.LOSS_UPA, w=5.0, alpha=al, beta=be, grad_kind=ops.GRAD_SLICE)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g[a:b]), _bits(g_q)), (q, float((g[a:b].float() - g_q.float()).abs().max()))
        assert torch.equal(_bits(sc[q]), _bits(sc_q)), (q, sc[q], sc_q)
        assert torch.equal(pred[q * Bp : (q + 1) * Bp], pred_q) and torch.equal(pf[q * Bp : (q + 1) * Bp], pf_q)
        assert float(sc_q[5]) == Rg and float(g_q.float().abs().max()) > 0
    if P > 1:  # the groups' weights acted: same labels, other logits and other weights -> other totals
        assert len({float(v) for v in sc[:, 0]}) == P
    ops.async_error_check()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ordinary_map_at_one_group_gives_the_old_call_its_bits(ops, dtype):
    _, labels, _ = synthetic.synth_text_batch(9, 6)
    labels = labels.to(DEV)
    R = len(_rows(labels.cpu().numpy()))
    z = _logits(R, 9, dtype)
    rm, seg1 = ops.LossRowMap(labels), ops.LossRowMapSeg(labels, 1)
    sc0, p0, f0, g0 = ops.loss_rows_fwd_bwd(z, rm, ops.LOSS_UPA, w=5.0, alpha=0.3, beta=0.7, grad_kind=ops.GRAD_SLICE)
    for rowmap in (rm, seg1):  # an ordinary map with P = 1, and a one-group segmented map
        sc1, p1, f1, g1 = ops.loss_rows_fwd_bwd_seg_upa(z, rowmap, 1, [(0.3, 0.7)], w=5.0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(g0), _bits(g1)) and torch.equal(_bits(sc0), _bits(sc1[0])) and torch.equal(p0, p1) and torch.equal(f0, f1)
    with pytest.raises(Exception, match="groups"):
        ops.loss_rows_fwd_bwd_seg_upa(z, seg1, 2, [(0.3, 0.7), (0.7, 0.3)])
    # rows are read and written in 16-byte pieces: a logits / gradient buffer off that alignment is refused, nothing is launched
    off = torch.zeros(R * V + 1, dtype=dtype, device=DEV)[1:].view(R, V)
    off.copy_(z)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    with pytest.raises(Exception, match="16-byte aligned"):
        ops.loss_rows_fwd_bwd_seg_upa(off, seg1, 1, [(0.3, 0.7)], w=5.0)
    goff = torch.zeros(R * 256 + 1, dtype=dtype, device=DEV)[1:].view(R, 256)
    with pytest.raises(Exception, match="16-byte aligned"):
        ops.loss_rows_fwd_bwd_seg_upa(z, seg1, 1, [(0.3, 0.7)], w=5.0, grad=goff)
    sc_e, _, _, _ = ops.loss_rows_fwd_bwd_seg_upa(z, seg1, 1, [(0.3, 0.7)], w=5.0, want_grad=False)
    assert torch.equal(_bits(sc_e[0]), _bits(sc0))
    with pytest.raises(Exception, match="VAA_LOSS_CE"):  # the target sweep's entry point is not widened
        ops.loss_rows_fwd_bwd_seg(z, seg1, 1, ops.LOSS_UPA)
    ops.async_error_check()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. against the reference's recorded values and the C oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_fixture_group(d, sc_g, g_slice):
    """A group's scalars / gradient slice against the reference's recorded UPA loss: the bounds of test_gpu_kernels.py::test_k3_upa_vs_reference_golden."""
    sc_g = sc_g.cpu().numpy()
    print("fixture scalars: total %.7f (%.7f) angle %.7f (%.7f) dist %.7f (%.7f)" % (sc_g[0], float(d["total"]), sc_g[3], float(d["angle"]), sc_g[4], float(d["dist"])))
    assert abs(sc_g[0] - float(d["total"])) < 3e-5 and abs(sc_g[3] - float(d["angle"])) < 3e-5 and abs(sc_g[4] - float(d["dist"])) < 3e-5
    gr = np.zeros((g_slice.shape[0], V), dtype=np.float32)  # slice storage: zero outside the action columns
    gr[:, 31744:32000] = g_slice.float().cpu().numpy()
    scale = max(np.abs(d["upa_g_action"]).max(), np.abs(d["upa_g_cols"]).max())
    e_a, e_c = np.abs(gr[:, 31744:32000] - d["upa_g_action"]).max(), np.abs(gr[:, d["upa_cols"]] - d["upa_g_cols"]).max()
    print("fixture gradient: max err action %.3e cols %.3e, bound %.3e" % (e_a, e_c, 2e-4 * scale))
    assert e_a <= 2e-4 * scale and e_c <= 2e-4 * scale


def _check_oracle_group(full, labels, al, be, sc_g, g_slice, rows):
    """... and against the C oracle's UPA loss with the group's own (alpha, beta): scalars to the rows-path bound of test_gpu_tma_sweep.py, the
    gradient to test_gpu_kernels.py's fp32 bound."""
    so, go = c_oracle.loss(full, labels, c_oracle.MODE_UPA, w=5.0, alpha=al, beta=be)
    got = sc_g.cpu().numpy()
    assert np.allclose(got[[0, 3, 4]], so[[0, 3, 4]], rtol=3e-5, atol=3e-5), (got, so)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    gor = go[rb, rp]
    assert np.abs(gor[:, :31744]).max() == 0 and np.abs(gor[:, 32000:]).max() == 0  # UPA's gradient lives in the action columns
    assert np.abs(g_slice.float().cpu().numpy() - gor[:, 31744:32000]).max() <= 2e-4 * np.abs(gor).max()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_fixture_through_the_segmented_call(ops, tag):
    """k3_upa_a (3 x 25 labels) and k3_upa_b (2 x 18) differ in B and L, so each goes through the new call at P = 1 and once more as group 1 beside a
    decoy group 0 (the same labels, other logits, other weights)."""
    d = np.load(os.path.join(GOLDEN, f"k3_upa_{tag}.npz"))
    B, S, seed = int(d["B"]), int(d["S"]), int(d["seed"])
    al, be = float(d["alpha"]), float(d["belta"])
    full = synthetic.synth_logits(seed + 1000, B, S, V)
    labels = torch.from_numpy(d["labels"])
    rows = _rows(d["labels"], S)
    assert np.array_equal(np.array(rows), d["upa_rows"])
    zr = full[torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])].contiguous().to(DEV)
    R = len(rows)
    # P = 1
    sc, _, _, g = ops.loss_rows_fwd_bwd_seg_upa(zr, ops.LossRowMapSeg(labels.to(DEV), 1), 1, [(al, be)], w=5.0)
    torch.cuda.synchronize()
    _check_fixture_group(d, sc[0], g)
    _check_oracle_group(full.numpy(), d["labels"], al, be, sc[0], g, rows)
    # group 1 beside a decoy
    decoy_full = synthetic.synth_logits(seed + 2000, B, S, V)
    zd = decoy_full[torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])].contiguous().to(DEV)
    dal, dbe = be + 0.45, al + 0.35
    lab2 = labels.repeat(2, 1).contiguous().to(DEV)
    sc2, _, _, g2 = ops.loss_rows_fwd_bwd_seg_upa(torch.cat([zd, zr]).contiguous(), ops.LossRowMapSeg(lab2, 2), 2, [(dal, dbe), (al, be)], w=5.0)
    torch.cuda.synchronize()
    ops.async_error_check()
    _check_fixture_group(d, sc2[1], g2[R:])
    _check_oracle_group(full.numpy(), d["labels"], al, be, sc2[1], g2[R:], rows)
    _check_oracle_group(decoy_full.numpy(), d["labels"], dal, dbe, sc2[0], g2[:R], rows)
    assert torch.equal(_bits(sc2[1]), _bits(sc[0])) and torch.equal(_bits(g2[R:]), _bits(g))  # the decoy does not reach group 1
    assert abs(float(sc2[0, 0]) - float(sc2[1, 0])) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. the step's ending: pass-through epilogue with the scalars in its tail, then the segmented K4 with the L1 clip
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_epilogue_tail_then_clipped_k4_is_bitwise_p_standalone_sequences(ops):
    P, Bp, n = 3, 4, 3 * 50 * 50
    clip = 1e-3
    gen = torch.Generator(device=DEV).manual_seed(12)
    partials = torch.randn(P * Bp, n, device=DEV, generator=gen) * 1e-3
    partials[Bp : 2 * Bp] *= 1e-6  # group 1: an L1 norm far below the clip; groups 0 and 2 far above it
    sc_in = torch.randn(P, 8, device=DEV, generator=gen)
    patch0 = torch.rand(P * n, device=DEV, generator=gen)
    m0 = torch.randn(P * n, device=DEV, generator=gen) * 1e-4
    v0 = torch.rand(P * n, device=DEV, generator=gen) * 1e-7
    hyper = dict(mode=ops.OPT_ADAMW_HF, lr=2e-3, step=3, l1_clip=clip, grad_scale=0.5)
    msg = torch.full((P * (n + 4),), 7.0, device=DEV)
    ops.step_epilogue_seg_tail(partials, msg, sc_in, P)
    p, m, v = patch0.clone(), m0.clone(), v0.clone()
    stats = ops.patch_update_seg(p, msg[: P * n], m, v, P, **hyper)
    torch.cuda.synchronize()
    ops.async_error_check()
    l1 = (msg[: P * n].view(P, n).double().abs().sum(1) * 0.5).cpu().numpy()  # the norm K4 clips: of the scaled gradient
    print("groups' L1 norms:", l1)
    assert l1[1] < clip / 10 and l1[0] > 10 * clip and l1[2] > 10 * clip
    assert torch.equal(msg[P * n :].view(P, 4), sc_in[:, [1, 2, 7, 0]]) and stats.shape == (P, 2)
    for q in range(P):
        sl = slice(q * n, (q + 1) * n)
        msg_g = torch.zeros(n + 4, device=DEV)
        ops.step_epilogue(partials[q * Bp : (q + 1) * Bp].contiguous(), msg_g, sc_in[q].contiguous())
        p_g, m_g, v_g = patch0[sl].clone(), m0[sl].clone(), v0[sl].clone()
        st_g = ops.patch_update(p_g, msg_g[:n].contiguous(), m_g, v_g, **hyper)
        torch.cuda.synchronize()
        assert torch.equal(msg[sl], msg_g[:n]) and torch.equal(msg[P * n + 4 * q : P * n + 4 * q + 4], msg_g[n:])
        assert torch.equal(p[sl], p_g) and torch.equal(m[sl], m_g) and torch.equal(v[sl], v_g) and torch.equal(_bits(stats[q]), _bits(st_g))
        assert not torch.equal(p_g, patch0[sl])
    ops.async_error_check()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _run(d, save_dir, pair=(0.8, 0.2), sweep=None, **kw):
    """One product UPA run of the data-parallel loop on the golden's setup (sweep_harness.run): a standalone run (alpha, belta) or a UPA sweep.
    Returns (per-step patches [steps, P, 3, 50, 50], host logs per outer iteration, attacker, kernel names of the TRAINING steps, call counts of
    the training steps)."""
    return run(d, save_dir, "UPA", alpha=pair[0], belta=pair[1], upa_sweep=sweep, **kw)


SWEEP3 = [(0.8, 0.2), (0.2, 0.8), (1.0, 0.0)]
TAGS3 = ["alpha0.8-belta0.2", "alpha0.2-belta0.8", "alpha1-belta0"]


def test_one_group_upa_sweep_is_the_existing_upa_loop_bit_for_bit(tmp_path, monkeypatch):
    """upa_sweep=[(a, b)] against the existing data-parallel UPA attacker at the same (a, b), both on the GEMM head (VAA_FUSED_HEAD=0): the patch
    after every inner step (4 outer x 3 inner), the train logs and the validation averages are bit for bit equal — K1 through the per-image
    descriptor pastes the same pixels, K2' leaves the same partial tiles, the pass-through epilogue reproduces K2's final sum and the message, and the
    segmented K4 with the clip is K4's one-group case."""
    env(monkeypatch, gemm_head=True)
    d = np.load(os.path.join(GOLDEN, "traj_ddp_k3s.npz"))
    n_it, inner = int(d["num_iter"]), int(d["inner"])
    assert n_it >= 3 and inner >= 3
    one, one_logs, one_att, one_names, _ = _run(d, str(tmp_path / "one"), sweep=[(0.35, 0.65)])
    base, base_logs, base_att, base_names, _ = _run(d, str(tmp_path / "base"), pair=(0.35, 0.65))
    assert one.shape == (n_it * inner, 1, 3, 50, 50) and base.shape == one.shape
    e = np.abs(one[:, 0] - base[:, 0]).reshape(n_it * inner, -1).max(1)
    print("one-group sweep per-step max |sweep - existing loop|:", ["%.2e" % v for v in e])
    assert np.array_equal(one, base) and np.array_equal(one_logs.reshape(-1, 4), base_logs)
    assert np.abs(base[-1, 0] - base[0, 0]).max() > 1e-4  # the patch really moved (clipped steps are about 0.1 lr each)
    tag = "alpha0.35-belta0.65"
    assert one_att.sweep_tags == [tag]
    assert one_att.val_MSE_Distance[tag] == base_att.val_MSE_Distance and one_att.val_CE_loss[tag] == base_att.val_CE_loss
    assert one_att.val_UAD[tag] == base_att.val_UAD and len(base_att.val_MSE_Distance) == 1
    assert one_att.last_train_log[tag] == base_att.last_train_log
    assert not any("head_slice_kernel" in nm for nm in one_names + base_names)  # both on the GEMM head
    assert torch.equal(torch.load(tmp_path / "one" / tag / "last" / "patch.pt"), torch.load(tmp_path / "base" / "last" / "patch.pt"))


def test_upa_sweep_trajectory_vs_standalone_upa_runs(tmp_path, monkeypatch):
    """upa_sweep=[(0.8, 0.2), (0.2, 0.8), (1, 0)] on the setup of traj_ddp_k3s.npz (SurrogateHeadVLA, its sizes, seeds and schedule; bs 3 per group):
    every group's per-inner-step patches are within 1e-4 of its standalone product run (attack_type="UPA", that alpha / belta, same seed) — the body
    runs at batch P*Bp, so the groups are not bit-equal; the groups' final patches differ from one another by at least 10x the largest deviation seen
    (the per-group weights acted; the tolerance hides no shared parameter); per step ONE head GEMM, ONE statistics, ONE finishing and ONE K4 launch
    for all groups; per-group files exist.

    Measured on one MI355X (12 steps): see DESIGN.md section 6a."""
    env(monkeypatch)
    d = np.load(os.path.join(GOLDEN, "traj_ddp_k3s.npz"))
    n_it, inner = int(d["num_iter"]), int(d["inner"])
    steps = n_it * inner
    snaps, logs, att, names, counts = _run(d, str(tmp_path / "sweep"), sweep=SWEEP3)
    assert snaps.shape == (steps, 3, 3, 50, 50) and logs.shape == (n_it, 3, 4)
    # call counts and the library's dispatch record: one head GEMM, one K3 (one statistics + one finishing launch), one backward GEMM and one K4 per step
    assert counts == dict(head=steps, k3=steps, back=steps, k4=steps), counts
    assert sum("rows_stats_kernel" in nm for nm in names) == steps and sum("rows_finish_kernel" in nm for nm in names) == steps
    assert sum("patch_update_kernel" in nm for nm in names) == steps and sum("step_epilogue_kernel" in nm for nm in names) == steps
    assert sum("embed_dgrad" in nm for nm in names) == steps and not any("head_slice_kernel" in nm for nm in names)
    assert att.sweep_tags == TAGS3 and set(att.last_train_log) == set(TAGS3)
    for tag in TAGS3:
        assert os.path.exists(tmp_path / "sweep" / tag / "last" / "patch.pt") and os.path.exists(tmp_path / "sweep" / tag / "0" / "patch.pt")
    worst = 0.0
    for g, pair in enumerate(SWEEP3):
        s_snaps, s_logs, s_att, _, _ = _run(d, str(tmp_path / f"solo{g}"), pair=pair)
        assert s_snaps.shape == (steps, 1, 3, 50, 50)
        e = np.abs(snaps[:, g] - s_snaps[:, 0]).reshape(steps, -1).max(1)
        print(f"group {g} per-step max |sweep - standalone|:", ["%.2e" % v for v in e])
        worst = max(worst, float(e.max()))
        assert e.max() <= 1e-4, e
        assert np.abs(s_snaps[-1, 0] - s_snaps[0, 0]).max() > 1e-4 and np.abs(snaps[-1, g] - snaps[0, g]).max() > 1e-4  # the patches really moved
        print(f"group {g} train total sweep / standalone:", logs[:, g, 3], s_logs[:, 3])
        np.testing.assert_allclose(logs[:, g, 3], s_logs[:, 3], rtol=3e-4)
        np.testing.assert_allclose([att.val_MSE_Distance[TAGS3[g]][0]], [s_att.val_MSE_Distance[0]], rtol=2e-3)  # the selection metric: scalar 0
        last = torch.load(tmp_path / "sweep" / TAGS3[g] / "last" / "patch.pt").numpy()
        assert np.abs(last - torch.load(tmp_path / f"solo{g}" / "last" / "patch.pt").numpy()).max() <= 1e-4
    apart = min(float(np.abs(snaps[-1, i] - snaps[-1, j]).max()) for i in range(3) for j in range(i + 1, 3))
    print("largest group-vs-standalone deviation %.3e, smallest distance between two groups' final patches %.3e" % (worst, apart))
    assert apart >= 10 * worst, (apart, worst)


def _sweep2_worker(rank, world, port, out_dir, golden_path, group):
    worker_env(rank, world, port)
    d = np.load(golden_path)
    if group < 0:  # the sweep
        snaps, logs, att, names, counts = _run(d, os.path.join(out_dir, f"rank{rank}"), sweep=SWEEP3, rank=rank, world=world)
        tag = "sweep"
    else:  # the standalone two-rank run of one group's pair
        snaps, logs, att, names, counts = _run(d, os.path.join(out_dir, f"solo{group}_{rank}"), pair=SWEEP3[group], rank=rank, world=world)
        tag = f"solo{group}"
    np.savez(os.path.join(out_dir, f"{tag}_r{rank}.npz"), snaps=snaps, logs=logs, n_stats=sum("rows_stats_kernel" in n for n in names),
             n_k4=sum("patch_update_kernel" in n for n in names))


def test_upa_sweep_two_ranks_vs_standalone_two_rank_runs(tmp_path):
    """Two ranks (gloo on one GPU, as test_target_sweep_two_ranks_group0_vs_standalone_two_rank_run) of the three-group UPA sweep: ONE all-reduce of
    [3 gradients | 3 x 4 scalars] per step and the segmented K4 with the clip; the ranks are bit-identical after every step; every group is within
    1e-4 of the standalone two-rank UPA run at its pair, and the groups are at least 10x further apart than the largest deviation."""
    golden = os.path.join(GOLDEN, "traj_ddp2_k3s.npz")
    d = np.load(golden)
    n_it, inner = int(d["num_iter"]), int(d["inner"])
    for group in (-1, 0, 1, 2):
        spawn2(_sweep2_worker, str(tmp_path), golden, group)
    r0, r1 = np.load(tmp_path / "sweep_r0.npz"), np.load(tmp_path / "sweep_r1.npz")
    assert r0["snaps"].shape == (n_it * inner, 3, 3, 50, 50) and r0["logs"].shape == (n_it, 3, 4)
    assert np.array_equal(r0["snaps"], r1["snaps"]) and np.array_equal(r0["logs"], r1["logs"])
    assert int(r0["n_stats"]) == n_it * inner and int(r0["n_k4"]) == n_it * inner
    worst = 0.0
    for g in range(3):
        s0, s1 = np.load(tmp_path / f"solo{g}_r0.npz"), np.load(tmp_path / f"solo{g}_r1.npz")
        assert np.array_equal(s0["snaps"], s1["snaps"])
        err = np.abs(r0["snaps"][:, g] - s0["snaps"][:, 0]).reshape(n_it * inner, -1).max(1)
        print(f"group {g} per-step max |sweep - standalone two-rank run|:", ["%.2e" % e for e in err])
        worst = max(worst, float(err.max()))
        assert err.max() <= 1e-4, err
        assert np.abs(r0["snaps"][-1, g] - r0["snaps"][0, g]).max() > 1e-4
        np.testing.assert_allclose(r0["logs"][:, g, 3], s0["logs"][:, 3], rtol=3e-4)
    apart = min(float(np.abs(r0["snaps"][-1, i] - r0["snaps"][-1, j]).max()) for i in range(3) for j in range(i + 1, 3))
    print("two ranks: largest deviation %.3e, smallest distance between two groups' final patches %.3e" % (worst, apart))
    assert apart >= 10 * worst
    assert os.path.exists(tmp_path / "rank0" / TAGS3[0] / "last" / "patch.pt") and os.path.exists(tmp_path / "rank0" / TAGS3[2] / "last" / "patch.pt")
    assert not os.path.exists(tmp_path / "rank1" / TAGS3[0])
