"""GPU parity tests: every call goes through the C-ABI (libvaa_hip.so) and is compared with
  (1) the golden vectors the REFERENCE produced (tests/golden, made by tools/gen_golden.py), and
  (2) the plain-C oracle on the same seeded inputs (oracle/vaa_oracle.c, itself pinned to the golden vectors).
Bars: paste/warp mask indices and the whole bf16 model input bit-exact; fp32 gradients/losses to the stated tolerance.
"""
import contextlib
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_files
from oracle import c_oracle, ref_port
from roboticattack_amd import synthetic

pytestmark = pytest.mark.gpu

K1K2 = golden_files("k1k2_")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _bits(t_bf16):
    return t_bf16.view(torch.int16).cpu().numpy().view(np.uint16)


def _keep_unpack(keep_bits):  # [B,3,6272] u8, bit p&7 of byte p>>3  ->  [B,3,50176] 0/1
    k = keep_bits.cpu().numpy()
    return np.unpackbits(k, axis=-1, bitorder="little")


def _run_k1(ops, imgs, patch, xy, theta, geometry, mm):
    out, keep = ops.patch_apply_fwd(_t(imgs), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), bool(geometry), mm)
    torch.cuda.synchronize()
    return out, keep


@pytest.mark.parametrize("f", K1K2, ids=[os.path.basename(f)[5:-4] for f in K1K2])
def test_k1_k2_vs_reference_golden(ops, f):
    d = np.load(f)
    B, geo = int(d["batch"]), int(d["geometry"])
    mm = 1 if str(d["fn"]) == "paste_patch_fix" else 0
    imgs = synthetic.synth_images(int(d["img_seed"]), B, str(d["img_kind"]))
    out, keep = _run_k1(ops, imgs, d["patch"], d["xy"], d["theta"], geo, mm)
    # mask indices: bit-exact against the reference's torch.where condition
    ref_keep = np.unpackbits(d["keep_bits"], axis=-1)[:, :, : 224 * 224]
    assert np.array_equal(_keep_unpack(keep), ref_keep)
    # the whole bf16 model input equals the reference's (CRC over all B*6*224*224 values)
    assert zlib.crc32(_bits(out).view(np.int16).tobytes()) == int(d["bf16_crc32"])
    # K2 against the reference's autograd patch gradient, with and without the stored mask
    g = synthetic.synth_upstream_grad(int(d["grad_seed"]), B).to(DEV)
    args = (_t(d["patch"]), _t(d["xy"], torch.int32), _t(d["theta"].reshape(-1, 6)))
    ref = d["patch_grad"]
    tol = 2e-6 * np.abs(ref).max()  # fp32 summation-order level (reference accumulates in fp32)
    g1 = ops.patch_grad_gather(g, *args, keep, bool(geo), mm).cpu().numpy()
    g2 = ops.patch_grad_gather(g, *args, None, bool(geo), mm).cpu().numpy()
    assert np.abs(g1 - ref).max() <= tol
    assert np.array_equal(g1, g2), "stored-mask and recomputed-mask paths must agree exactly"


def _random_case(rs, B, ph, pw, edge_frac=0.3, identity_frac=0.2):
    xy = np.stack([rs.randint(0, 224 - pw + 1, B), rs.randint(0, 224 - ph + 1, B)], 1).astype(np.int32)
    for b in range(B):
        if rs.rand() < edge_frac:
            xy[b, 0] = rs.choice([0, 224 - pw])
        if rs.rand() < edge_frac:
            xy[b, 1] = rs.choice([0, 224 - ph])
    theta = np.zeros((B, 2, 3), np.float32)
    for b in range(B):
        if rs.rand() < identity_frac:
            m = np.eye(3, dtype=np.float32)
        else:
            m = np.dot(ref_port.shear_matrix(rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2)), ref_port.rotation_matrix(rs.uniform(-30, 30)))
        theta[b] = m[:2]
    return xy, theta


@pytest.mark.parametrize("ph,pw,B,geo", [(50, 50, 16, 1), (50, 50, 8, 0), (22, 22, 8, 1), (37, 61, 6, 1), (100, 100, 6, 1),
                                         (139, 139, 3, 1), (61, 61, 5, 1), (1, 1, 4, 1), (224, 224, 2, 1)])
def test_k1_k2_random_sweep_vs_oracle(ops, ph, pw, B, geo):
    rs = np.random.RandomState(ph * 1000 + pw * 10 + B + geo)
    imgs = synthetic.synth_images(ph + pw + B, B, "noise")
    patch = rs.rand(3, ph, pw).astype(np.float32)
    xy, theta = _random_case(rs, B, ph, pw)
    out, keep = _run_k1(ops, imgs, patch, xy, theta, geo, 0)
    o_f32, o_bf16, o_keep = c_oracle.patch_apply_fwd(imgs, patch, xy, theta, geo, 0)
    assert np.array_equal(_keep_unpack(keep), o_keep)
    assert np.array_equal(_bits(out), o_bf16)
    g = synthetic.synth_upstream_grad(5 + B, B)
    og = c_oracle.patch_grad(_bits(g), patch, xy, theta, geo, 0)
    try:
        gg = ops.patch_grad_gather(g.to(DEV), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), keep, bool(geo), 0).cpu().numpy()
    except Exception as e:  # the only legal refusal: a patch whose accumulator tile exceeds the LDS
        assert ph * pw * 4 > 150 * 1024, e
        return
    assert np.abs(gg - og).max() <= 3e-6 * max(np.abs(og).max(), 1e-30)


def test_k1_empty_row_beyond_the_frame_regression(ops):
    """Patch on the right/bottom frame edge with a small rotation: far above/below the patch the conservative column interval of a row
    lies wholly BEYOND column 223 (the edge side is open to infinity). Such rows must be empty for both kernel roles — round 2 found
    the streaming role skipping items nobody wrote (seen at bs > 64, image 66 of the bench batch: xy=(174,108))."""
    xy = np.array([[174, 108], [174, 0], [100, 174], [0, 174], [174, 174]], np.int32)
    theta = np.array([[[0.9908992, -0.13735135, 0.0], [0.00398219, 1.0131141, 0.0]],
                      [[0.99, 0.01, 0.0], [-0.004, 1.01, 0.0]],
                      [[1.0, 0.004, 0.0], [0.14, 0.99, 0.0]],
                      [[1.01, -0.003, 0.0], [0.1, 0.98, 0.0]],
                      [[0.995, 0.002, 0.0], [0.003, 1.004, 0.0]]], np.float32)
    B = len(xy)
    imgs = synthetic.synth_images(66, B, "noise")
    patch = np.random.RandomState(1).rand(3, 50, 50).astype(np.float32)
    out, keep = _run_k1(ops, imgs, patch, xy, theta, 1, 0)
    _, o_bf16, o_keep = c_oracle.patch_apply_fwd(imgs, patch, xy, theta, 1, 0)
    assert np.array_equal(_bits(out), o_bf16) and np.array_equal(_keep_unpack(keep), o_keep)
    g = synthetic.synth_upstream_grad(2, B)
    og = c_oracle.patch_grad(_bits(g), patch, xy, theta, 1, 0)
    gg = ops.patch_grad_gather(g.to(DEV), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), keep, True, 0).cpu().numpy()
    assert np.abs(gg - og).max() <= 3e-6 * np.abs(og).max()


@pytest.mark.parametrize("B", [96, 200])
def test_k1_k2_bench_draws_beyond_bs64_vs_oracle(ops, B):
    """The seed-42 draws of the bench at batch sizes above 64 (different footprint split per image), every value against the oracle."""
    from roboticattack_amd.benchmarks import random_params

    imgs = synthetic.synth_images(1234, B, "noise")
    patch = np.random.RandomState(3).rand(3, 50, 50).astype(np.float32)
    xy, th = random_params(B, 50, 50, 42)
    theta = th.reshape(B, 2, 3)
    out, keep = _run_k1(ops, imgs, patch, xy, theta, 1, 0)
    out2, keep2 = _run_k1(ops, imgs, patch, xy, theta, 1, 0)
    assert torch.equal(out, out2) and torch.equal(keep, keep2)
    _, o_bf16, o_keep = c_oracle.patch_apply_fwd(imgs, patch, xy, theta, 1, 0)
    assert np.array_equal(_bits(out), o_bf16) and np.array_equal(_keep_unpack(keep), o_keep)
    g = synthetic.synth_upstream_grad(2, 64).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
    og = c_oracle.patch_grad(_bits(g), patch, xy, theta, 1, 0)
    gg = ops.patch_grad_gather(g.to(DEV), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), keep, True, 0).cpu().numpy()
    assert np.abs(gg - og).max() <= 3e-6 * np.abs(og).max()


def test_k1_general_affine_with_translation(ops):
    """The C-ABI takes any 2x3 theta (the reference only draws rotation+shear): scale, translation, near-singular."""
    rs = np.random.RandomState(77)
    B = 6
    imgs = synthetic.synth_images(9, B, "smooth")
    patch = rs.rand(3, 50, 50).astype(np.float32)
    xy = np.array([[10, 20], [0, 0], [174, 174], [100, 3], [60, 60], [5, 150]], np.int32)
    theta = np.array([[[1.3, 0.1, 0.2], [-0.2, 0.8, -0.1]], [[0.5, 0, 0.5], [0, 0.5, 0.5]], [[2.0, 0, -0.9], [0, 2.0, -0.9]],
                      [[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]], [[1e-7, 1.0, 0.0], [1.0, 1e-7, 0.0]], [[1, 0, 3.0], [0, 1, 3.0]]], np.float32)
    out, keep = _run_k1(ops, imgs, patch, xy, theta, 1, 0)
    _, o_bf16, o_keep = c_oracle.patch_apply_fwd(imgs, patch, xy, theta, 1, 0)
    assert np.array_equal(_keep_unpack(keep), o_keep)
    assert np.array_equal(_bits(out), o_bf16)
    g = synthetic.synth_upstream_grad(3, B)
    og = c_oracle.patch_grad(_bits(g), patch, xy, theta, 1, 0)
    gg = ops.patch_grad_gather(g.to(DEV), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), keep, True, 0).cpu().numpy()
    assert np.abs(gg - og).max() <= 3e-6 * np.abs(og).max()


def test_k2_full_size_properties_bs64(ops):
    """BASELINE size (bs=64, 3x50x50): linearity in the upstream gradient, bitwise repeatability, sum over sub-batches."""
    B = 64
    rs = np.random.RandomState(64)
    imgs = _t(synthetic.synth_images(640, B, "noise"))
    patch = _t(rs.rand(3, 50, 50).astype(np.float32))
    xy_n, th_n = _random_case(rs, B, 50, 50)
    xy, th = _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    out, keep = ops.patch_apply_fwd(imgs, patch, xy, th, True, 0)
    g1 = synthetic.synth_upstream_grad(1, B).to(DEV)
    g2 = synthetic.synth_upstream_grad(2, B).to(DEV)
    a = ops.patch_grad_gather(g1, patch, xy, th, keep, True, 0)
    b = ops.patch_grad_gather(g2, patch, xy, th, keep, True, 0)
    for _ in range(3):  # fp64 LDS accumulation + fixed-order partial sums -> run-to-run identical bits
        assert torch.equal(a, ops.patch_grad_gather(g1, patch, xy, th, keep, True, 0))
    # linearity: bf16(2*g) is exact, so K2(2 g1) == 2 K2(g1) bitwise; K2 of a sum within fp32 rounding
    assert torch.equal(ops.patch_grad_gather((g1.float() * 2).to(torch.bfloat16), patch, xy, th, keep, True, 0), a * 2)
    gs = (g1.float() + g2.float())
    exact = gs.to(torch.bfloat16).float().equal(gs)
    s = ops.patch_grad_gather(gs.to(torch.bfloat16), patch, xy, th, keep, True, 0)
    if exact:
        assert (s - (a + b)).abs().max() <= 1e-6 * (a.abs().max() + b.abs().max())
    # batch additivity: halves sum to the whole
    h1 = ops.patch_grad_gather(g1[:32].contiguous(), patch, xy[:32].contiguous(), th[:32].contiguous(), keep[:32].contiguous(), True, 0)
    h2 = ops.patch_grad_gather(g1[32:].contiguous(), patch, xy[32:].contiguous(), th[32:].contiguous(), keep[32:].contiguous(), True, 0)
    assert (h1 + h2 - a).abs().max() <= 1e-6 * a.abs().max()
    # and the oracle on the same 64 images
    og = c_oracle.patch_grad(_bits(g1), patch.cpu().numpy(), xy_n, th_n, 1, 0)
    assert np.abs(a.cpu().numpy() - og).max() <= 3e-6 * np.abs(og).max()
    # and against the EXACT sum of the reference's fp32 products (fp64 accumulation): the kernel adds exact integers, so only its
    # final fp32 rounding separates it from that sum — closer than the reference's own fp32 scan-order accumulation
    ex = c_oracle.patch_grad(_bits(g1), patch.cpu().numpy(), xy_n, th_n, 1, 0, f64=True)
    assert np.abs(a.cpu().numpy() - ex).max() <= 2e-7 * np.abs(ex).max()
    assert np.abs(a.cpu().numpy() - ex).max() <= np.abs(og - ex).max()
    _, o_bf16, _ = c_oracle.patch_apply_fwd(imgs.cpu().numpy(), patch.cpu().numpy(), xy_n, th_n, 1, 0)
    assert np.array_equal(_bits(out), o_bf16)


def test_k1_k2_empty_and_large_batch(ops):
    patch = _t(np.random.RandomState(0).rand(3, 50, 50).astype(np.float32))
    e_out, e_keep = ops.patch_apply_fwd(torch.empty((0, 224, 224, 3), dtype=torch.uint8, device=DEV), patch,
                                        torch.empty((0, 2), dtype=torch.int32, device=DEV), torch.empty((0, 6), device=DEV), True, 0)
    assert e_out.shape == (0, 6, 224, 224)
    gz = ops.patch_grad_gather(torch.empty((0, 6, 224, 224), dtype=torch.bfloat16, device=DEV), patch,
                               torch.empty((0, 2), dtype=torch.int32, device=DEV), torch.empty((0, 6), device=DEV), None, True, 0)
    assert torch.count_nonzero(gz) == 0
    # more images than persistent workgroups (B > 512): every image must still be accumulated exactly once
    B = 700
    rs = np.random.RandomState(700)
    xy_n, th_n = _random_case(rs, B, 50, 50)
    xy, th = _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    imgs = torch.zeros((B, 224, 224, 3), dtype=torch.uint8, device=DEV)
    _, keep = ops.patch_apply_fwd(imgs, patch, xy, th, True, 0)
    g = torch.ones((B, 6, 224, 224), dtype=torch.bfloat16, device=DEV)
    whole = ops.patch_grad_gather(g, patch, xy, th, keep, True, 0)
    parts = sum(ops.patch_grad_gather(g[s:e].contiguous(), patch, xy[s:e].contiguous(), th[s:e].contiguous(), keep[s:e].contiguous(), True, 0)
                for s, e in ((0, 300), (300, 700)))
    assert (whole - parts).abs().max() <= 1e-6 * whole.abs().max()


@pytest.mark.parametrize("ph,pw,B", [(50, 50, 64), (100, 100, 8), (139, 139, 4), (195, 200, 2), (224, 224, 2)])
def test_k2_bitwise_repeatable_every_size(ops, ph, pw, B):
    """Integer (fixed-point) LDS accumulation + fixed-order partial sums: identical bits run after run for every patch size,
    including the row-banded sizes whose int64 plane exceeds the LDS (> 135 px) — and still the oracle's numbers."""
    rs = np.random.RandomState(ph + B)
    imgs = _t(synthetic.synth_images(3, B, "noise"))
    patch_n = rs.rand(3, ph, pw).astype(np.float32)
    xy_n, th_n = _random_case(rs, B, ph, pw)
    patch, xy, th = _t(patch_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    _, keep = ops.patch_apply_fwd(imgs, patch, xy, th, True, 0)
    g = synthetic.synth_upstream_grad(11, B)
    a = ops.patch_grad_gather(g.to(DEV), patch, xy, th, keep, True, 0)
    for _ in range(4):
        assert torch.equal(a, ops.patch_grad_gather(g.to(DEV), patch, xy, th, keep, True, 0))
    og = c_oracle.patch_grad(_bits(g), patch_n, xy_n, th_n, 1, 0)
    assert np.abs(a.cpu().numpy() - og).max() <= 3e-6 * np.abs(og).max()


def test_k2_gradient_scale_range_and_nonfinite(ops):
    """The fixed-point format follows the data: images whose gradients differ by 2^40 in one batch (forces the lazy re-scale),
    tiny (1e-27 after the 1e-3 of the generator; the format bottoms out at 2^-100) and huge (1e27) gradients keep fp32-level relative accuracy; an inf/nan upstream gradient poisons (NaN) at least the texels autograd would."""
    B, rs = 12, np.random.RandomState(5)
    imgs = _t(synthetic.synth_images(4, B, "smooth"))
    patch_n = rs.rand(3, 50, 50).astype(np.float32)
    xy_n, th_n = _random_case(rs, B, 50, 50)
    patch, xy, th = _t(patch_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    _, keep = ops.patch_apply_fwd(imgs, patch, xy, th, True, 0)
    g = synthetic.synth_upstream_grad(21, B).float()
    for scales in ([2.0 ** (-20 + 4 * b) for b in range(B)], [1e-24] * B, [1e30] * B, [2.0 ** (24 - 4 * b) for b in range(B)]):
        gs = (g * torch.tensor(scales).view(B, 1, 1, 1)).to(torch.bfloat16)
        og = c_oracle.patch_grad(_bits(gs), patch_n, xy_n, th_n, 1, 0)
        got = ops.patch_grad_gather(gs.to(DEV), patch, xy, th, keep, True, 0).cpu().numpy()
        assert np.isfinite(got).all()
        assert np.abs(got - og).max() <= 3e-6 * np.abs(og).max(), scales[:2]
    gbad = g.clone()
    ys, xs = np.nonzero(_keep_unpack(keep)[3, 0].reshape(224, 224))
    gbad[3, 0, ys[0], xs[0]] = float("inf")
    gb16 = gbad.to(torch.bfloat16)
    got = ops.patch_grad_gather(gb16.to(DEV), patch, xy, th, keep, True, 0).cpu().numpy()
    bad_ref = ~np.isfinite(c_oracle.patch_grad(_bits(gb16), patch_n, xy_n, th_n, 1, 0))  # the texels autograd would make inf / nan
    assert bad_ref.any() and np.isnan(got[bad_ref]).all()  # a superset is poisoned (the whole row band of the workgroup that met the value)
    assert np.isnan(got).all() or np.isfinite(got[~np.isnan(got)]).all()


def test_k2_int64_tile_flush_huge_batch(ops):
    """A workgroup flushes its int64 tile into its fp32 partial before the tile could overflow (2^17 footprint pixels). 16,000 images =
    the same 64 placements / gradients 250 times (9.6 GB of bf16 gradient, 32 images per workgroup -> one flush each): the result is
    250 x the 64-image result, which the oracle provides."""
    B0, rep = 64, 250
    rs = np.random.RandomState(11)
    imgs = _t(synthetic.synth_images(5, B0, "noise"))
    patch_n = rs.rand(3, 50, 50).astype(np.float32)
    xy_n, th_n = _random_case(rs, B0, 50, 50)
    patch = _t(patch_n)
    _, keep0 = ops.patch_apply_fwd(imgs, patch, _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6)), True, 0)
    g0 = synthetic.synth_upstream_grad(9, B0)
    og = c_oracle.patch_grad(_bits(g0), patch_n, xy_n, th_n, 1, 0)
    g = g0.to(DEV).repeat(rep, 1, 1, 1).contiguous()
    xy, th, keep = _t(xy_n, torch.int32).repeat(rep, 1).contiguous(), _t(th_n.reshape(-1, 6)).repeat(rep, 1).contiguous(), keep0.repeat(rep, 1, 1).contiguous()
    got = ops.patch_grad_gather(g, patch, xy, th, keep, True, 0)
    assert torch.equal(got, ops.patch_grad_gather(g, patch, xy, th, keep, True, 0))
    del g
    assert np.abs(got.cpu().numpy() / rep - og).max() <= 3e-6 * np.abs(og).max()


def test_k1_k2_multi_row_banded_sizes_vs_oracle(ops):
    """Per-image patches up to 139x139 (config 5's largest scale): the int64 plane of the largest image exceeds the LDS, so K2 `_multi`
    runs in row bands; smaller images of the same batch fit a single band's worth of rows. Against the oracle, stored and recomputed mask."""
    sizes = np.array([[139, 139], [61, 61], [100, 139], [139, 70], [224, 3]], np.int32)
    B = len(sizes)
    rs = np.random.RandomState(139)
    imgs = synthetic.synth_images(13, B, "smooth")
    pdesc_n, total = ops.make_pdesc(sizes)
    packed_n = rs.rand(total).astype(np.float32)
    xy_n = np.array([[rs.randint(0, 224 - w + 1), rs.randint(0, 224 - h + 1)] for h, w in sizes], np.int32)
    xy_n[0] = (85, 0)  # the largest patch on the top edge
    _, th_n = _random_case(rs, B, 50, 50)
    pdesc, packed, xy, th = _t(pdesc_n), _t(packed_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    max_hw = (int(sizes[:, 0].max()), int(sizes[:, 1].max()))
    out, keep = ops.patch_apply_fwd_multi(_t(imgs), packed, pdesc, max_hw, xy, th, True, 0)
    _, o_bf16, o_keep = c_oracle.patch_apply_fwd_multi(imgs, packed_n, pdesc_n, xy_n, th_n, 1, 0)
    assert np.array_equal(_bits(out), o_bf16) and np.array_equal(_keep_unpack(keep), o_keep)
    g = synthetic.synth_upstream_grad(4, B)
    o_gp = c_oracle.patch_grad_multi(_bits(g), packed_n, pdesc_n, xy_n, th_n, 1, 0)
    for kp in (keep, None):
        gp = ops.patch_grad_gather_multi(g.to(DEV), packed, pdesc, max_hw, xy, th, kp, True, 0)
        for (h, w, off, _z) in pdesc_n:  # per image: its own gradient scale
            a, b = gp.cpu().numpy()[off : off + 3 * h * w], o_gp[off : off + 3 * h * w]
            assert np.abs(a - b).max() <= 3e-6 * max(np.abs(b).max(), 1e-30), (h, w)
    assert torch.equal(gp, ops.patch_grad_gather_multi(g.to(DEV), packed, pdesc, max_hw, xy, th, None, True, 0))


def test_k3_rowmap_large_batch(ops):
    """vaa_loss_rowmap_build beyond one pass of its 1024 threads (B = 1500): header counts and every {b, k, label, ord} entry."""
    from roboticattack_amd.labels import mask_labels

    B = 1500
    _, labels, _ = synthetic.synth_text_batch(3, B)
    labels = mask_labels(labels, [0, 3])
    labels[7] = -100  # a sample without any labelled position
    rm = ops.LossRowMap(labels.to(DEV))
    raw = rm.buf.cpu().numpy().view(np.int32)
    lab = labels.numpy()
    bk = np.argwhere(lab[:, 1:] != -100)
    R = len(bk)
    assert raw[0] == R and raw[1] == int((lab[:, 1:] > 2).sum())
    ent = raw[4 : 4 + 4 * R].reshape(R, 4)
    assert np.array_equal(ent[:, 0], bk[:, 0]) and np.array_equal(ent[:, 1], bk[:, 1])
    assert np.array_equal(ent[:, 2], lab[bk[:, 0], bk[:, 1] + 1])
    first = np.r_[True, bk[1:, 0] != bk[:-1, 0]]
    ordv = np.arange(R) - np.maximum.accumulate(np.where(first, np.arange(R), 0))
    assert np.array_equal(ent[:, 3], ordv)


RESIZE = golden_files("resize_")


@pytest.mark.parametrize("f", RESIZE, ids=[os.path.basename(f)[:-4] for f in RESIZE])
def test_resize_patch_config5_vs_reference_golden(ops, f):
    """BASELINE config 5 (resize_patch=True) against what the REFERENCE computed (A-D2 repair, tools/gen_golden.py:gen_resize):
    draws, RNG consumption, mask bits and the whole bf16 tensor bit-exact; gradient to the base patch <= 2e-6; every stage against
    the C oracle; launches do not depend on B."""
    import random

    from roboticattack_amd import ops as O
    from roboticattack_amd.transform import RandomPatchTransform

    d = np.load(f)
    B = int(d["batch"])
    imgs = synthetic.synth_images(int(d["img_seed"]), B, str(d["img_kind"]))
    g = synthetic.synth_upstream_grad(int(d["grad_seed"]), B)
    patch_n = d["patch"]
    ph, pw = patch_n.shape[1:]
    # ---- the operator as the attack loops call it ----
    t = RandomPatchTransform(DEV, resize_patch=True)
    random.seed(int(d["rng_seed"]))
    np.random.seed(int(d["rng_seed"]))
    patch = _t(patch_n).requires_grad_(True)
    O.TIMER = []
    out = t.apply_random_patch_batch(synthetic.to_pil_list(imgs), patch, ref_port.MEAN, ref_port.STD, True)
    assert (random.random(), float(np.random.rand())) == tuple(d["rng_after"]), "RNG consumption differs from the reference"
    assert np.array_equal(t.last_sizes, d["sizes"]) and np.array_equal(t.last_params[0], d["xy"])
    assert np.array_equal(t.last_params[1].reshape(B, 2, 3), d["theta"])
    assert zlib.crc32(_bits(out).view(np.int16).tobytes()) == int(d["bf16_crc32"]), "whole bf16 model input identical to the reference's"
    si = d["sample_idx"].astype(int)
    assert np.array_equal(out.detach().float().cpu().numpy()[si[:, 0], si[:, 1], si[:, 2], si[:, 3]],
                          torch.from_numpy(d["samples"]).to(torch.bfloat16).float().numpy())
    out.backward(gradient=g.to(DEV))
    torch.cuda.synchronize()
    launches = [n for (n, *_r) in O.TIMER]
    O.TIMER = None
    assert launches == ["K0_patch_resize_fwd", "K1_patch_apply_fwd_multi", "K2_patch_grad_gather_multi", "K0_patch_resize_bwd"], launches
    ref = d["patch_grad"]
    assert np.abs(patch.grad.cpu().numpy() - ref).max() <= 2e-6 * np.abs(ref).max()
    # ---- stage by stage against the C oracle ----
    pdesc_n, total = O.make_pdesc(d["sizes"])
    o_pdesc, o_total = c_oracle.make_pdesc(d["sizes"])
    assert np.array_equal(pdesc_n, o_pdesc) and total == o_total
    pdesc = _t(pdesc_n)
    packed = O.patch_resize_fwd(_t(patch_n), pdesc, total)
    o_packed = c_oracle.patch_resize_fwd(patch_n, pdesc_n, total)
    assert np.array_equal(packed.cpu().numpy(), o_packed), "antialias-bilinear resize must equal torch's CPU kernel bit for bit"
    max_hw = (int(pdesc_n[:, 0].max()), int(pdesc_n[:, 1].max()))
    xy, th = _t(d["xy"], torch.int32), _t(d["theta"].reshape(-1, 6))
    o2, keep = O.patch_apply_fwd_multi(_t(imgs), packed, pdesc, max_hw, xy, th, True, 0)
    kb = np.unpackbits(d["keep_bits"], axis=-1)[:, :, : 224 * 224]
    assert np.array_equal(_keep_unpack(keep), kb), "paste/warp mask indices must be bit-exact"
    assert torch.equal(o2, out.detach())
    for kp in (keep, None):  # stored mask / mask recomputed from the resized patches
        gp = O.patch_grad_gather_multi(g.to(DEV), packed, pdesc, max_hw, xy, th, kp, True, 0)
        o_gp = c_oracle.patch_grad_multi(_bits(g), o_packed, pdesc_n, d["xy"], d["theta"], 1, 0)
        assert np.abs(gp.cpu().numpy() - o_gp).max() <= 3e-6 * np.abs(o_gp).max()
    assert torch.equal(gp, O.patch_grad_gather_multi(g.to(DEV), packed, pdesc, max_hw, xy, th, keep, True, 0))  # bitwise repeatable
    gb = O.patch_resize_bwd(_t(o_gp), pdesc, ph, pw).cpu().numpy()
    o_gb = c_oracle.patch_resize_bwd(o_gp, pdesc_n, ph, pw)
    assert np.abs(gb - o_gb).max() <= 1e-6 * np.abs(o_gb).max()


@pytest.mark.parametrize("ph,pw,sizes", [(100, 100, [(61, 61), (139, 139), (100, 100), (100, 61), (139, 100), (1, 1), (224, 224)]),
                                         (50, 50, [(30, 69), (50, 50), (19, 19), (69, 69)]), (37, 61, [(22, 84), (51, 37)]),
                                         # K0_CASES "r20" / "r20mix" of patch_grad_ref.py: the direct form (more than kTapMax taps)
                                         (20, 20, [(5, 5), (5, 20), (20, 5), (6, 40), (4, 7)]), (20, 20, [(5, 5), (20, 20), (27, 13)])])
def test_patch_resize_kernel_vs_torch_cpu(ops, ph, pw, sizes):
    """The HIP resize equals torch's CPU antialias-bilinear kernel bit for bit (up- and down-scaling, unchanged axes, extremes);
    its adjoint equals torch autograd to fp32 summation order."""
    torch.manual_seed(ph + pw)
    x = torch.rand(3, ph, pw)
    pdesc_n, total = ops.make_pdesc(sizes)
    pdesc = _t(pdesc_n)
    packed = ops.patch_resize_fwd(x.to(DEV), pdesc, total).cpu().numpy()
    gy = torch.rand(total)
    xg = x.clone().requires_grad_(True)
    acc = 0
    for (h, w, off, _z) in pdesc_n:
        ref = ref_port.resize_patch(xg, int(h), int(w))
        assert np.array_equal(packed[off : off + 3 * h * w].reshape(3, h, w), ref.detach().numpy()), (h, w)
        acc = acc + (ref * gy[off : off + 3 * h * w].view(3, h, w)).sum()
    acc.backward()
    gb = ops.patch_resize_bwd(gy.to(DEV), pdesc, ph, pw).cpu().numpy()
    assert np.abs(gb - xg.grad.numpy()).max() <= 2e-6 * np.abs(xg.grad.numpy()).max()


def test_resize_patch_config5_upa_step_vs_ref_port(ops):
    """Config 5 as a workload: 3x100x100 base patch, B=4, geometry on, UPA loss (maskidx sweep) through the fp32 surrogate.
    The product path (RandomPatchTransform(resize_patch=True) -> model -> K3 UPA -> K2 multi -> resize adjoint) against the
    restated reference ops (oracle/ref_port.py + autograd on CPU) driven by the same draws."""
    import random

    from roboticattack_amd.surrogate import SurrogateVLA
    from roboticattack_amd.transform import RandomPatchTransform

    B = 4
    imgs = synthetic.synth_images(505, B, "smooth")
    input_ids, labels, attn = synthetic.synth_text_batch(55, B)
    torch.manual_seed(42)
    patch0 = torch.rand(3, 100, 100)
    cpu_model, gpu_model = SurrogateVLA(seed=9), SurrogateVLA(seed=9).to(DEV)
    # ---- reference ops on CPU ----
    random.seed(7)
    np.random.seed(7)
    sizes, xy, theta = ref_port.draw_params_resized(B, 100, 100, True)
    after = (random.random(), float(np.random.rand()))
    pc = patch0.clone().requires_grad_(True)
    pix_c = ref_port.apply_random_patch_batch_resized(imgs, pc, sizes, xy, theta, True).to(torch.bfloat16)
    pix_c.retain_grad()
    logits_c = cpu_model(input_ids, attn, pix_c, labels).logits
    loss_c, _, _ = ref_port.upa_weighted_loss(logits_c, labels, 0.8, 0.2)
    loss_c.backward()
    # ---- product path on the GPU ----
    random.seed(7)
    np.random.seed(7)
    t = RandomPatchTransform(DEV, resize_patch=True)
    pg = patch0.clone().to(DEV).requires_grad_(True)
    pix_g = t.apply_random_patch_batch(synthetic.to_pil_list(imgs), pg, ref_port.MEAN, ref_port.STD, True)
    assert (random.random(), float(np.random.rand())) == after, "RNG consumption"
    assert np.array_equal(t.last_sizes, sizes) and np.array_equal(t.last_params[0], xy)
    # bit-exact against the C oracle (pinned to the reference's own output by the resize_* goldens). torch's CPU grid_sample on the
    # test host can differ from the golden-producing host in the last fp32 bit (MKL / vector path; a `canvas < -20` flip at a
    # boundary pixel is then possible), so against ref_port-on-this-host only the fraction of differing values is bounded.
    pdesc_n, total = c_oracle.make_pdesc(sizes)
    o_packed = c_oracle.patch_resize_fwd(patch0.numpy(), pdesc_n, total)
    _, o_bf16, _ = c_oracle.patch_apply_fwd_multi(imgs, o_packed, pdesc_n, xy, theta, 1, 0)
    assert np.array_equal(_bits(pix_g.detach()), o_bf16), "model input identical to the oracle's"
    assert float((pix_g.detach().float().cpu() != pix_c.detach().float()).float().mean()) < 1e-3
    # the whole step on the GPU: surrogate model + K3 (UPA) + K2 with per-image patches + resize adjoint
    pix_g.retain_grad()
    out = gpu_model(input_ids.to(DEV), attn.to(DEV), pix_g, labels.to(DEV))
    total_l, sc, _, _ = ops.DiscrepancyLoss.apply(out.logits, labels.to(DEV), ops.LOSS_UPA, 5.0, 0.8, 0.2, 1.0, ops.LAYOUT_FULL)
    total_l.backward()
    # K3 against the restated UPA loss on the very same logits
    l_ref, a_ref, d_ref = ref_port.upa_weighted_loss(out.logits.detach().float().cpu(), labels, 0.8, 0.2)
    assert abs(float(total_l) - float(l_ref)) <= 3e-5 * abs(float(l_ref))
    assert abs(float(sc[3]) - float(a_ref)) <= 3e-5 and abs(float(sc[4]) - float(d_ref)) <= 3e-5 * float(d_ref)
    # K2 (per-image gradients) + resize adjoint against the oracle chain fed with the same upstream bf16 gradient
    gup = pix_g.grad.detach()
    o_gp = c_oracle.patch_grad_multi(_bits(gup), o_packed, pdesc_n, xy, theta, 1, 0)
    o_g = c_oracle.patch_resize_bwd(o_gp, pdesc_n, 100, 100)
    assert np.abs(pg.grad.cpu().numpy() - o_g).max() <= 3e-6 * np.abs(o_g).max()
    # and the complete CPU autograd of the restated reference ops (different GEMM order in the model, possible mask flips): direction
    ref = pc.grad.numpy().ravel()
    got = pg.grad.cpu().numpy().ravel()
    assert abs(float(total_l) - float(loss_c)) <= 1e-3 * abs(float(loss_c))
    assert float(np.dot(ref, got) / (np.linalg.norm(ref) * np.linalg.norm(got))) > 0.999


def test_patch_apply_autograd_function(ops):
    """PyTorch-ROCm autograd drives K2 through PatchApply.backward exactly like the attack loop does."""
    d = np.load(os.path.join(GOLDEN, "k1k2_geo50_rand.npz"))
    B = int(d["batch"])
    imgs = _t(synthetic.synth_images(int(d["img_seed"]), B, str(d["img_kind"])))
    patch = _t(d["patch"]).requires_grad_(True)
    out = ops.PatchApply.apply(patch, imgs, _t(d["xy"], torch.int32), _t(d["theta"].reshape(-1, 6)), True, 0)
    assert out.dtype == torch.bfloat16 and out.requires_grad
    g = synthetic.synth_upstream_grad(int(d["grad_seed"]), B).to(DEV)
    out.backward(gradient=g)
    assert np.abs(patch.grad.cpu().numpy() - d["patch_grad"]).max() <= 2e-6 * np.abs(d["patch_grad"]).max()


# ----------------------------------------------------------------------------------------------------------
# K3
# ----------------------------------------------------------------------------------------------------------
def _rows(labels):
    B, L = labels.shape
    S = 256 + L
    return [(b, S - L + k) for b in range(B) for k in range(L - 1) if labels[b, k + 1] != -100]


def _check_rows(g_full, labels, d, pfx, rtol):
    rows = _rows(labels)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    gr = g_full[rb, rp]
    scale = max(np.abs(d[f"{pfx}_g_action"]).max(), np.abs(d[f"{pfx}_g_cols"]).max())
    assert np.abs(gr[:, 31744:32000] - d[f"{pfx}_g_action"]).max() <= rtol * scale
    assert np.abs(gr[:, d[f"{pfx}_cols"]] - d[f"{pfx}_g_cols"]).max() <= rtol * scale
    assert abs(np.abs(g_full).sum() - np.abs(gr).sum()) <= 1e-6 * np.abs(gr).sum() + 1e-12  # unlabelled rows untouched (zero)
    return gr


def _check_fp64(g_full, labels, logits, mode, **kw):
    """The fp32 gradient of the labelled rows element by element against the fp64 reference's bound (tests/loss_ref.py), beside the max-norm checks."""
    import loss_ref

    rows = _rows(np.asarray(labels))
    rb, rp = torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])
    loss_ref.compare(loss_ref.loss_ref(logits[rb, rp].cpu(), torch.as_tensor(np.asarray(labels)), mode, **kw), grad=g_full[rb, rp], layout="ROWS", tag=mode)


@pytest.mark.parametrize("tag", ["m0", "m012", "m6", "mall"])
def test_k3_uada_vs_reference_golden(ops, tag):
    d = np.load(os.path.join(GOLDEN, f"k3_uada_{tag}.npz"))
    B, S, seed = int(d["B"]), int(d["S"]), int(d["seed"])
    logits = synthetic.synth_logits(seed + 1000, B, S, 32064).to(DEV)
    labels = _t(d["masked"])
    sc, pred, g = ops.loss_fwd_bwd(logits, labels, ops.LOSS_UADA, w=5.0)
    sc = sc.cpu().numpy()
    assert abs(sc[0] - float(d["total"])) < 3e-5 and abs(sc[1] - float(d["ce"])) < 3e-5 and abs(sc[2] - float(d["mse"])) < 3e-5
    assert abs(sc[7] - float(d["uad"])) < 1e-6
    gr = _check_rows(g.cpu().numpy(), d["masked"], d, "uada", 2e-4)
    _check_fp64(g, d["masked"], logits, "UADA", w=5.0)
    # DDP mode (no 1/CE term) with --MSE_weights
    sc2, _, g2 = ops.loss_fwd_bwd(logits, labels, ops.LOSS_UADA_DDP, w=float(d["ddp_w"]))
    assert abs(sc2.cpu().numpy()[0] - float(d["ddp_mse"])) < 3e-5
    _check_rows(g2.cpu().numpy(), d["masked"], d, "ddp", 2e-4)
    _check_fp64(g2, d["masked"], logits, "UADA_DDP", w=float(d["ddp_w"]))
    # ROWS layout on the compacted labelled rows gives the same numbers
    rows = _rows(d["masked"])
    compact = logits[torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])].contiguous()
    sc3, pred3, g3 = ops.loss_fwd_bwd(compact, labels, ops.LOSS_UADA, w=5.0, layout=ops.LAYOUT_ROWS)
    assert torch.equal(sc3, sc_t(sc, DEV)) or np.allclose(sc3.cpu().numpy(), sc, rtol=0, atol=1e-6)
    assert np.allclose(g3.cpu().numpy(), gr, rtol=0, atol=1e-9)
    assert torch.equal(pred, pred3)
    # argmax tokens equal the oracle's
    op, _ = c_oracle.action_argmax(logits.cpu().numpy(), d["masked"])
    assert np.array_equal(pred.cpu().numpy()[pred.cpu().numpy() >= 0], op)
    # bf16 logits: same loss to bf16-level tolerance, gradient in bf16
    lb = logits.to(torch.bfloat16)
    scb, _, gb = ops.loss_fwd_bwd(lb, labels, ops.LOSS_UADA, w=5.0)
    so, go = c_oracle.loss(lb.float().cpu().numpy(), d["masked"], c_oracle.MODE_UADA, w=5.0)
    assert np.allclose(scb.cpu().numpy()[:3], so[:3], rtol=1e-5, atol=1e-5)
    assert gb.dtype == torch.bfloat16
    assert np.abs(gb.float().cpu().numpy() - go).max() <= 1e-2 * np.abs(go).max()


def sc_t(sc, dev):
    return torch.from_numpy(np.asarray(sc)).to(dev)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_k3_upa_vs_reference_golden(ops, tag):
    d = np.load(os.path.join(GOLDEN, f"k3_upa_{tag}.npz"))
    B, S, seed = int(d["B"]), int(d["S"]), int(d["seed"])
    logits = synthetic.synth_logits(seed + 1000, B, S, 32064).to(DEV)
    sc, _, g = ops.loss_fwd_bwd(logits, _t(d["labels"]), ops.LOSS_UPA, alpha=float(d["alpha"]), beta=float(d["belta"]))
    sc = sc.cpu().numpy()
    assert abs(sc[0] - float(d["total"])) < 3e-5 and abs(sc[3] - float(d["angle"])) < 3e-5 and abs(sc[4] - float(d["dist"])) < 3e-5
    _check_rows(g.cpu().numpy(), d["labels"], d, "upa", 2e-4)
    _check_fp64(g, d["labels"], logits, "UPA", alpha=float(d["alpha"]), beta=float(d["belta"]))


@pytest.mark.parametrize("tag", ["t0", "t012"])
def test_k3_tma_vs_reference_golden(ops, tag):
    d = np.load(os.path.join(GOLDEN, f"k3_tma_{tag}.npz"))
    B, S, seed = int(d["B"]), int(d["S"]), int(d["seed"])
    logits = synthetic.synth_logits(seed + 1000, B, S, 32064).to(DEV)
    sc, _, g = ops.loss_fwd_bwd(logits, _t(d["newlabels"]), ops.LOSS_CE, scale=1.0)
    assert abs(sc.cpu().numpy()[0] - float(d["ce"])) < 3e-5
    _check_rows(g.cpu().numpy(), d["newlabels"], d, "tma", 2e-4)
    _check_fp64(g, d["newlabels"], logits, "CE", scale=1.0)
    sc2, _, g2 = ops.loss_fwd_bwd(logits, _t(d["newlabels"]), ops.LOSS_CE, scale=0.25)  # accumulate_steps = 4
    assert abs(sc2.cpu().numpy()[0] - 0.25 * float(d["ce"])) < 1e-5
    assert np.allclose(g2.cpu().numpy(), 0.25 * g.cpu().numpy(), rtol=1e-6, atol=1e-12)


def test_k3_bs64_vs_oracle(ops):
    """BASELINE size: B=64, maskidx=[0] -> 128 labelled rows of 32064 logits."""
    B = 64
    _, labels, _ = synthetic.synth_text_batch(4242, B)
    masked = ref_port.mask_labels(labels.clone(), [0])
    L = labels.shape[1]
    S = 256 + L
    rs = np.random.RandomState(1)
    logits = torch.zeros((B, S, 32064), dtype=torch.float32)
    rows = _rows(masked.numpy())
    for (b, p) in rows:
        logits[b, p] = torch.from_numpy((rs.standard_normal(32064) * 2).astype(np.float32))
    sc, pred, g = ops.loss_fwd_bwd(logits.to(DEV), masked.to(DEV), ops.LOSS_UADA, w=5.0)
    so, go = c_oracle.loss(logits.numpy(), masked.numpy(), c_oracle.MODE_UADA, w=5.0)
    assert np.allclose(sc.cpu().numpy()[:7], so[:7], rtol=2e-5, atol=2e-5)
    assert np.abs(g.cpu().numpy() - go).max() <= 2e-4 * np.abs(go).max()
    dsc = DiscrepancyCheck(ops, logits.to(DEV), masked.to(DEV))
    assert abs(dsc - so[0]) < 3e-5


def DiscrepancyCheck(ops, logits, labels):
    lg = logits.clone().requires_grad_(True)
    total, scalars, pred, _ = ops.DiscrepancyLoss.apply(lg, labels, ops.LOSS_UADA, 5.0, 0.8, 0.2, 1.0, ops.LAYOUT_FULL)
    (total * 2.0).backward()
    _, _, g = ops.loss_fwd_bwd(logits, labels, ops.LOSS_UADA, w=5.0)
    assert torch.allclose(lg.grad, 2.0 * g)
    return float(total)


# ----------------------------------------------------------------------------------------------------------
# K4
# ----------------------------------------------------------------------------------------------------------
def test_k4_adamw_pgd_clip_vs_oracle(ops):
    rs = np.random.RandomState(4)
    n_shape = (3, 50, 50)
    p0 = rs.rand(*n_shape).astype(np.float32)
    p = _t(p0)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    pc, mc, vc = p0.copy().ravel(), np.zeros(7500, np.float32), np.zeros(7500, np.float32)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = ref_port.HFAdamW([pt], lr=1e-3)
    for t in range(1, 7):
        lr = 1e-3 * ref_port.cosine_lambda(t, 2, 10)
        g = (rs.randn(*n_shape) * 10.0 ** rs.uniform(-7, -1, n_shape)).astype(np.float32)
        st = ops.patch_update(p, _t(g), m, v, ops.OPT_ADAMW_HF, lr, t)
        l1 = c_oracle.patch_update(pc, g.ravel(), mc, vc, 0, lr, t)
        opt.param_groups[0]["lr"] = lr
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        pt.data = pt.data.clamp(0, 1)
        assert np.abs(p.cpu().numpy().ravel() - pc).max() < 1e-6
        assert np.abs(p.cpu().numpy() - pt.detach().numpy()).max() < 1e-6
        s = st.cpu().numpy()
        assert abs(s[0] - l1) <= 1e-5 * l1 and abs(s[1] - g.mean()) <= 1e-6 * abs(g).mean() + 1e-9
    assert p.min() >= 0 and p.max() <= 1
    # DDP: sum of ranks' gradients with grad_scale = 1/world == mean gradient
    pa, pb = _t(p0), _t(p0)
    ma, va, mb, vb = (torch.zeros_like(pa) for _ in range(4))
    g = rs.randn(*n_shape).astype(np.float32)
    ops.patch_update(pa, _t(g * 4), ma, va, ops.OPT_ADAMW_HF, 1e-3, 1, grad_scale=0.25)
    ops.patch_update(pb, _t(g), mb, vb, ops.OPT_ADAMW_HF, 1e-3, 1)
    assert torch.equal(pa, pb)
    # UPA: L1 grad-norm clip 1e-3 before the step (UPA.py:157)
    pq, mq, vq = _t(p0), torch.zeros_like(pa), torch.zeros_like(pa)
    ops.patch_update(pq, _t(g), mq, vq, ops.OPT_ADAMW_HF, 2e-3, 1, l1_clip=1e-3)
    pcq, mcq, vcq = p0.copy().ravel(), np.zeros(7500, np.float32), np.zeros(7500, np.float32)
    c_oracle.patch_update(pcq, g.ravel(), mcq, vcq, 0, 2e-3, 1, l1_clip=1e-3)
    assert np.abs(pq.cpu().numpy().ravel() - pcq).max() < 1e-6
    # PGD sign step (TMA.py:171-175)
    pg = _t(p0)
    ops.patch_update(pg, _t(g), None, None, ops.OPT_PGD_SIGN, 0.05, 1)
    assert np.allclose(pg.cpu().numpy(), ref_port.pgd_step(torch.from_numpy(p0), torch.from_numpy(g), 0.05).numpy(), atol=1e-7)


@pytest.mark.parametrize("shape", [(3, 1, 1), (3, 17, 31), (3, 52, 52), (2, 64, 64), (3, 53, 53), (3, 100, 100), (2, 128, 128), (3, 105, 105), (3, 139, 139)])
@pytest.mark.parametrize("mode", ["adamw_clip", "adamw", "pgd"])
def test_k4_every_form_vs_oracle(ops, shape, mode):
    """K4 in its three forms — 4 workgroups (n <= 8,192, incl. the exact boundary 2x64x64), 16 workgroups (n <= 32,768: UPA's 3x100x100 base patch, boundary 2x128x128)
    and the one-workgroup stream beyond — against the C oracle over three steps: patch / moments <= 1e-6, the logged statistics, and rows that straddle a
    workgroup's share. Every workgroup of the first two forms computes the whole gradient's statistics itself; the clip coefficient must come out the same in all."""
    rs = np.random.RandomState(sum(shape) + len(mode))
    n = int(np.prod(shape))
    p0 = rs.rand(*shape).astype(np.float32)
    p, m, v = _t(p0), torch.zeros(shape, device=DEV), torch.zeros(shape, device=DEV)
    pc, mc, vc = p0.copy().ravel(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(1, 4):
        g = (rs.randn(*shape) * 10.0 ** rs.uniform(-6, -2, shape)).astype(np.float32)
        if mode == "pgd":
            st = ops.patch_update(p, _t(g), None, None, ops.OPT_PGD_SIGN, 0.01, t)
            l1 = c_oracle.patch_update(pc, g.ravel(), mc, vc, 1, 0.01, t)
        else:
            clip = 1e-3 if mode == "adamw_clip" else 0.0
            st = ops.patch_update(p, _t(g), m, v, ops.OPT_ADAMW_HF, 2e-3, t, l1_clip=clip, grad_scale=0.5)
            l1 = c_oracle.patch_update(pc, (g * np.float32(0.5)).ravel(), mc, vc, 0, 2e-3, t, l1_clip=clip)
        assert np.abs(p.cpu().numpy().ravel() - pc).max() < 1e-6
        if mode != "pgd":
            assert np.abs(m.cpu().numpy().ravel() - mc).max() <= 1e-6 * max(np.abs(mc).max(), 1e-30) + 1e-12
            assert np.abs(v.cpu().numpy().ravel() - vc).max() <= 1e-6 * max(np.abs(vc).max(), 1e-30) + 1e-15
        s = st.cpu().numpy()
        scale = 0.5 if mode != "pgd" else 1.0
        assert abs(s[0] - l1) <= 1e-5 * l1 and abs(s[1] - scale * g.mean()) <= 1e-6 * abs(g).mean() + 1e-9
    with pytest.raises(Exception, match="overlap"):
        ops.patch_update(p, p, m, v, ops.OPT_ADAMW_HF, 1e-3, 1)
    # ... and a gradient that only PARTLY overlaps a buffer it is not pointer-equal to (views into one flat buffer: ADVICE r5)
    flat = torch.zeros(2 * n, device=DEV)
    pv, gv = flat[:n].view(shape), flat[n // 2 : n // 2 + n].view(shape)
    with pytest.raises(Exception, match="overlap"):
        ops.patch_update(pv, gv, m, v, ops.OPT_ADAMW_HF if mode != "pgd" else ops.OPT_PGD_SIGN, 1e-3, 1)
    ops.patch_update(pv, flat[n:].view(shape), m, v, ops.OPT_ADAMW_HF if mode != "pgd" else ops.OPT_PGD_SIGN, 1e-3, 1)  # adjacent, not overlapping: fine


@pytest.mark.parametrize("mode,maskidx,dtype", [("UADA_DDP", [0], torch.bfloat16), ("UADA_DDP", [0, 1, 2], torch.float32), ("UADA", [0], torch.float32),
                                                ("UPA", None, torch.float32), ("UPA", None, torch.bfloat16), ("CE", [0, 2, 5], torch.float32),
                                                ("CE", list(range(7)), torch.bfloat16)])
@pytest.mark.parametrize("B", [3, 64])
def test_k3_rows_path_vs_oracle(ops, mode, maskidx, dtype, B):
    """K3 on the labelled rows with a prebuilt row map (what the attack loops run): rows split over 2-4 workgroups, gradient confined
    to the action slice for UADA_DDP / UPA, slice argmax AND full-vocabulary argmax — all against the C oracle on the same logits."""
    from roboticattack_amd.labels import mask_labels, tma_target_labels, tma_target_tokens

    rs = np.random.RandomState(B * 7 + len(mode))
    _, labels, _ = synthetic.synth_text_batch(77 + B, B)
    if mode == "CE":
        labels = tma_target_labels(labels, tma_target_tokens(np.zeros(7), maskidx))
    elif mode != "UPA":
        labels = mask_labels(labels, maskidx)
    L = labels.shape[1]
    rows = _rows(labels.numpy())
    R = len(rows)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    z = (rs.standard_normal((R, 32064)) * 2).astype(np.float32)
    z[:, 31744:32000] += (rs.standard_normal((R, 256)) * 3).astype(np.float32)
    z[::3, 1234] = 40.0  # rows whose top-1 token is NOT an action token: slice argmax and full argmax must differ there
    zt = torch.from_numpy(z).to(dtype)
    full = torch.zeros((B, 256 + L, 32064), dtype=torch.float32)
    full[torch.from_numpy(rb), torch.from_numpy(rp)] = zt.float()
    omode = {"UADA": c_oracle.MODE_UADA, "UADA_DDP": c_oracle.MODE_UADA_DDP, "CE": c_oracle.MODE_CE, "UPA": c_oracle.MODE_UPA}[mode]
    kmode = {"UADA": ops.LOSS_UADA, "UADA_DDP": ops.LOSS_UADA_DDP, "CE": ops.LOSS_CE, "UPA": ops.LOSS_UPA}[mode]
    so, go = c_oracle.loss(full.numpy(), labels.numpy(), omode, w=5.0)
    gor = go[rb, rp]
    rm = ops.LossRowMap(labels.to(DEV))
    hdr = rm.buf[:16].view(torch.int32).cpu().numpy()
    assert hdr[0] == R and hdr[1] == int((labels[:, 1:] > 2).sum())
    gtol = (1e-2 if dtype == torch.bfloat16 else 2e-4) * max(np.abs(gor).max(), 1e-30)
    sliced = mode in ("UADA_DDP", "UPA")
    for kind in ([ops.GRAD_SLICE, ops.GRAD_FULL] if sliced else [ops.GRAD_FULL]):
        sc, pred, pred_full, g = ops.loss_rows_fwd_bwd(zt.to(DEV), rm, kmode, w=5.0, grad_kind=kind)
        assert np.allclose(sc.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5), (sc.cpu().numpy(), so)
        gg = g.float().cpu().numpy()
        if kind == ops.GRAD_SLICE:
            assert gg.shape == (R, 256)
            assert np.abs(gg - gor[:, 31744:32000]).max() <= gtol
            assert np.abs(np.delete(gor, np.s_[31744:32000], axis=1)).max() == 0.0  # the oracle agrees: nothing outside the slice
        else:
            assert np.abs(gg - gor).max() <= gtol
    # predictions: slice argmax (feeds UAD) and full-vocabulary argmax (UADA.py:165-167), -1 on positions without a label
    zf = zt.float().numpy()
    pf = pred_full.cpu().numpy().reshape(B, L - 1)
    ps = pred.cpu().numpy().reshape(B, L - 1)
    exp_full = np.full((B, L - 1), -1)
    exp_slice = np.full((B, L - 1), -1)
    for i, (b, p) in enumerate(rows):
        k = p - 256
        exp_full[b, k] = int(zf[i].argmax())
        if labels[b, k + 1] > 2:
            exp_slice[b, k] = 31744 + int(zf[i, 31744:32000].argmax())
    assert np.array_equal(pf, exp_full) and np.array_equal(ps, exp_slice)
    assert (pf[exp_slice >= 0] != ps[exp_slice >= 0]).any()
    # the generic entry point with LAYOUT_ROWS builds the map itself and must agree bit for bit
    sc2, pred2, g2, pf2 = ops.loss_fwd_bwd(zt.to(DEV), labels.to(DEV), kmode, w=5.0, layout=ops.LAYOUT_ROWS, want_pred_full=True)
    assert torch.equal(sc2, sc) and torch.equal(pred2, pred) and torch.equal(pf2, pred_full) and torch.equal(g2, g)
    # and the FULL layout (black-box model path) reports the same full-vocabulary argmax
    sc3, pred3, _, pf3 = ops.loss_fwd_bwd(full.to(DEV), labels.to(DEV), kmode, w=5.0, want_grad=False, want_pred_full=True)
    if dtype == torch.float32:
        assert torch.equal(pf3, pred_full) and torch.equal(pred3, pred)
        assert np.allclose(sc3.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("mode", ["UADA", "UADA_DDP"])
def test_k3_rows_path_wide_vocabulary(ops, mode):
    """A vocabulary beyond 32,768 columns takes the 512-thread instantiation of the row kernels (OpenVLA's 32,064 takes the 256-thread
    one): same checks against the C oracle."""
    from roboticattack_amd.labels import mask_labels

    B, V = 3, 40064
    rs = np.random.RandomState(5)
    _, labels, _ = synthetic.synth_text_batch(91, B)
    labels = mask_labels(labels, [0, 3])
    L = labels.shape[1]
    rows = _rows(labels.numpy())
    R = len(rows)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    z = (rs.standard_normal((R, V)) * 2).astype(np.float32)
    z[:, 31744:32000] += (rs.standard_normal((R, 256)) * 3).astype(np.float32)
    z[::2, 39000] = 35.0
    full = torch.zeros((B, 256 + L, V), dtype=torch.float32)
    full[torch.from_numpy(rb), torch.from_numpy(rp)] = torch.from_numpy(z)
    omode = {"UADA": c_oracle.MODE_UADA, "UADA_DDP": c_oracle.MODE_UADA_DDP}[mode]
    kmode = {"UADA": ops.LOSS_UADA, "UADA_DDP": ops.LOSS_UADA_DDP}[mode]
    so, go = c_oracle.loss(full.numpy(), labels.numpy(), omode, w=5.0)
    gor = go[rb, rp]
    rm = ops.LossRowMap(labels.to(DEV))
    sc, pred, pred_full, g = ops.loss_rows_fwd_bwd(torch.from_numpy(z).to(DEV), rm, kmode, w=5.0, grad_kind=ops.GRAD_FULL)
    assert np.allclose(sc.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5)
    assert np.abs(g.float().cpu().numpy() - gor).max() <= 2e-4 * max(np.abs(gor).max(), 1e-30)
    pf = pred_full.cpu().numpy().reshape(B, L - 1)
    for i, (b, p) in enumerate(rows):
        assert pf[b, p - 256] == int(z[i].argmax())


def test_head_loss_rows_matches_generic_head_backward(ops):
    """LM head + loss on the labelled rows with the backward contracting over the 256 action columns (UADA_DDP / UPA)
    equals the generic path (full [R,V] gradient @ W) to bf16 GEMM rounding; CE modes take the full-row route inside the same op."""
    from roboticattack_amd.labels import mask_labels

    B, D = 8, 512
    g = torch.Generator(device=DEV).manual_seed(3)
    W = (torch.randn(32064, D, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    _, labels, _ = synthetic.synth_text_batch(5, B)
    for mode, lab in ((ops.LOSS_UADA_DDP, mask_labels(labels.clone(), [0, 1])), (ops.LOSS_UPA, labels), (ops.LOSS_UADA, mask_labels(labels.clone(), [0]))):
        lab = lab.to(DEV)
        rm = ops.LossRowMap(lab)
        R = int((lab[:, 1:] != -100).sum())
        h = (torch.randn(R, D, device=DEV, generator=g)).to(torch.bfloat16)
        h1 = h.clone().requires_grad_(True)
        t1, s1, _, _ = ops.HeadLossRows.apply(h1, W, rm, mode, 5.0, 0.8, 0.2, 1.0)
        t1.backward()
        h2 = h.clone().requires_grad_(True)
        t2, s2, _, _ = ops.DiscrepancyLossRows.apply(torch.nn.functional.linear(h2, W), rm, mode, 5.0, 0.8, 0.2, 1.0)
        t2.backward()
        assert torch.equal(s1, s2)
        assert (h1.grad.float() - h2.grad.float()).abs().max() <= 2e-2 * h2.grad.float().abs().max() + 1e-12


def test_two_streams_overlap_k2_and_k3(ops):
    """include/vaa.h: re-entrant per stream, scratch is the caller's. The binding keys its scratch by (device, stream, operator), so
    the loss of one step and the gather of another can overlap on two streams; results equal the serial ones bit for bit."""
    from roboticattack_amd.labels import mask_labels

    B = 64
    rs = np.random.RandomState(2)
    imgs = _t(synthetic.synth_images(8, B, "noise"))
    patch = _t(rs.rand(3, 50, 50).astype(np.float32))
    xy_n, th_n = _random_case(rs, B, 50, 50)
    xy, th = _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    _, keep = ops.patch_apply_fwd(imgs, patch, xy, th, True, 0)
    g = synthetic.synth_upstream_grad(3, B).to(DEV)
    _, labels, _ = synthetic.synth_text_batch(12, B)
    labels = mask_labels(labels, [0]).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    logits = (torch.randn(R, 32064, device=DEV) * 2).to(torch.bfloat16)
    rm = ops.LossRowMap(labels)
    ref_g = ops.patch_grad_gather(g, patch, xy, th, keep, True, 0)
    ref_sc, _, _, ref_gl = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(20):
        with torch.cuda.stream(s1):
            g1 = ops.patch_grad_gather(g, patch, xy, th, keep, True, 0)
        with torch.cuda.stream(s2):
            sc2, _, _, gl2 = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0)
        torch.cuda.synchronize()
        assert torch.equal(g1, ref_g) and torch.equal(sc2, ref_sc) and torch.equal(gl2, ref_gl)
    assert len({k for k in ops._ws_cache if k[1] in (s1.cuda_stream, s2.cuda_stream)}) == 2  # one scratch buffer per (stream, operator)


def test_capi_error_paths_on_gpu(ops):
    from roboticattack_amd import _lib

    L = _lib.lib()
    p = torch.zeros((3, 50, 50), device=DEV)
    g = torch.zeros((2, 6, 224, 224), dtype=torch.bfloat16, device=DEV)
    xy = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    th = torch.zeros((2, 6), device=DEV)
    out = torch.zeros((3, 50, 50), device=DEV)
    ws = torch.zeros(16, dtype=torch.uint8, device=DEV)
    rc = L.vaa_patch_grad_gather(g.data_ptr(), p.data_ptr(), xy.data_ptr(), th.data_ptr(), None, 2, 50, 50, 1, 0, _lib.f32x([1] * 6),
                                 out.data_ptr(), ws.data_ptr(), 16, None)
    assert rc == -4 and b"workspace" in L.vaa_last_error()
    rc = L.vaa_patch_apply_fwd(g.data_ptr(), p.data_ptr(), xy.data_ptr(), th.data_ptr(), 2, 300, 50, 1, 0, _lib.f32x([0] * 6),
                               _lib.f32x([1] * 6), g.data_ptr(), None, None)
    assert rc == -2
    rc = L.vaa_loss_fwd_bwd(g.data_ptr(), 7, 0, xy.data_ptr(), 2, 300, 40, 32064, 0, _lib.f32x([5, 0, 0, 1]), out.data_ptr(), None, None,
                            ws.data_ptr(), 16, None)
    assert rc == -1


def test_eval_paste_vs_reference_and_oracle(ops):
    """K5 (simulation_random_patch): byte-exact frames vs the reference's golden and vs the C oracle on a random batch."""
    from roboticattack_amd.transform import RandomPatchTransform

    d = np.load(os.path.join(GOLDEN, "sim_patch.npz"))
    n = len(d["crc"])
    imgs = synthetic.synth_images(int(d["img_seed"]), n, "smooth")
    t = RandomPatchTransform(DEV)
    patch = torch.from_numpy(d["patch"])
    out = t.simulation_patch_batch(imgs, patch, list(d["geometry"]), list(d["angle"]), list(d["shx"]), list(d["shy"]), d["xy"]).cpu().numpy()
    assert [zlib.crc32(o.tobytes()) for o in out] == [int(c) for c in d["crc"]]
    one = t.simulation_random_patch(imgs[0], patch, geometry=bool(d["geometry"][0]), angle=float(d["angle"][0]), shx=float(d["shx"][0]),
                                    shy=float(d["shy"][0]), position=tuple(int(v) for v in d["xy"][0]))
    assert isinstance(one, np.ndarray) and one.dtype == np.uint8 and np.array_equal(one, out[0])
    rs = np.random.RandomState(5)
    B = 24
    imgs2 = synthetic.synth_images(3, B, "noise")
    p2 = rs.rand(3, 61, 37).astype(np.float32)
    xy, th = _random_case(rs, B, 61, 37)
    geo = rs.rand(B) < 0.7
    got = ops.patch_apply_eval(_t(imgs2), _t(p2), _t(xy, torch.int32), _t(th.reshape(-1, 6)), _t(geo.astype(np.int32))).cpu().numpy()
    assert np.array_equal(got, c_oracle.patch_apply_eval(imgs2, p2, xy, th, geo))


@pytest.mark.parametrize("name,B,ph,pw,geo,maskidx,mode", [
    ("cfg1_uada_bs1", 1, 50, 50, 1, [0], "UADA"),                 # BASELINE.json configs[0]: bs=1 plumbing case
    ("cfg2_uada_bs16_nogeo", 16, 50, 50, 0, [0], "UADA"),         # configs[1]: bs=16, geometry=False
    ("cfg3_ddp_rank_bs8", 8, 50, 50, 1, [0], "UADA_DDP"),         # configs[2]: 64 over 8 ranks -> 8 per rank
    ("cfg4_tma_rank_bs8", 8, 50, 50, 1, [0, 1, 2, 3, 4, 5, 6], "CE"),   # configs[3]: TMA, 32 over 4 ranks
    ("cfg5_upa_rank_bs4_100", 4, 100, 100, 1, [0, 1, 2], "UPA"),  # configs[4]: UPA, 3x100x100, 32 over 8 ranks
])
def test_baseline_config_shapes_one_step_vs_oracle(ops, name, B, ph, pw, geo, maskidx, mode):
    """One hot-path step (K1 -> K3 -> K2 -> K4) at the per-GPU shapes of every BASELINE.json config, each op against the oracle."""
    from roboticattack_amd.labels import mask_labels, tma_target_labels, tma_target_tokens

    rs = np.random.RandomState(len(name) + B)
    imgs = synthetic.synth_images(B + ph, B, "smooth")
    patch = rs.rand(3, ph, pw).astype(np.float32)
    xy, theta = _random_case(rs, B, ph, pw)
    out, keep = _run_k1(ops, imgs, patch, xy, theta, geo, 0)
    _, o_bf16, o_keep = c_oracle.patch_apply_fwd(imgs, patch, xy, theta, geo, 0)
    assert np.array_equal(_bits(out), o_bf16) and np.array_equal(_keep_unpack(keep), o_keep)
    # K3 on bf16 rows, as the attack loops feed it
    _, labels, _ = synthetic.synth_text_batch(31 + B, B)
    if mode == "CE":
        labels = tma_target_labels(labels, tma_target_tokens(np.zeros(7), maskidx))
    elif mode != "UPA":
        labels = mask_labels(labels, maskidx)
    L = labels.shape[1]
    rows = _rows(labels.numpy())
    full = torch.zeros((B, 256 + L, 32064), dtype=torch.float32)
    for (b, p) in rows:
        full[b, p] = torch.from_numpy((rs.standard_normal(32064) * 2).astype(np.float32)).to(torch.bfloat16).float()
    compact = full[torch.tensor([r[0] for r in rows]), torch.tensor([r[1] for r in rows])].to(torch.bfloat16).contiguous().to(DEV)
    kmode = {"UADA": ops.LOSS_UADA, "UADA_DDP": ops.LOSS_UADA_DDP, "CE": ops.LOSS_CE, "UPA": ops.LOSS_UPA}[mode]
    omode = {"UADA": c_oracle.MODE_UADA, "UADA_DDP": c_oracle.MODE_UADA_DDP, "CE": c_oracle.MODE_CE, "UPA": c_oracle.MODE_UPA}[mode]
    sc, _, g = ops.loss_fwd_bwd(compact, labels.to(DEV), kmode, w=5.0, layout=ops.LAYOUT_ROWS)
    so, go = c_oracle.loss(full.numpy(), labels.numpy(), omode, w=5.0)
    assert np.allclose(sc.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5)
    gor = go[np.array([r[0] for r in rows]), np.array([r[1] for r in rows])]
    assert np.abs(g.float().cpu().numpy() - gor).max() <= 1e-2 * max(np.abs(gor).max(), 1e-30)  # bf16 gradient storage
    # K2 + K4
    gup = synthetic.synth_upstream_grad(17, B)
    og = c_oracle.patch_grad(_bits(gup), patch, xy, theta, geo, 0)
    gg = ops.patch_grad_gather(gup.to(DEV), _t(patch), _t(xy, torch.int32), _t(theta.reshape(-1, 6)), keep, bool(geo), 0)
    assert np.abs(gg.cpu().numpy() - og).max() <= 3e-6 * np.abs(og).max()
    p = _t(patch)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ops.patch_update(p, gg, m, v, ops.OPT_ADAMW_HF, 2e-3, 1, l1_clip=1e-3 if mode == "UPA" else 0.0)
    pc, mc, vc = patch.copy().ravel(), np.zeros(patch.size, np.float32), np.zeros(patch.size, np.float32)
    c_oracle.patch_update(pc, og.ravel().copy(), mc, vc, 0, 2e-3, 1, l1_clip=1e-3 if mode == "UPA" else 0.0)
    assert np.abs(p.cpu().numpy().ravel() - pc).max() <= 1e-4  # north-star tolerance on the updated pixels


def test_patch_embed_grad_gather_vs_torch_conv_autograd(ops):
    """K2' against plain PyTorch-CPU autograd through the REAL formulation it replaces: the reference's paste/warp/normalise forward
    (oracle/ref_port.py, appply_random_transform.py:104-136), `.to(bfloat16)` (UADA.py:142), then timm's PatchEmbed of both towers as
    F.conv2d(x, W[D,3,14,14], stride=14) (modeling_prismatic.py:120-123) with tokens flattened row-major, and an upstream gradient on the
    conv OUTPUTS. Pins the (c, y, x) column order of the flattened conv weight, the token order and the tower / channel split; the
    remaining difference is the bf16 rounding point of the pixel gradient (the CPU chain rounds it once per tower as well)."""
    B, ph, pw, D0, D1 = 3, 50, 50, 64, 128
    rs = np.random.RandomState(31)
    imgs = synthetic.synth_images(8, B, "noise")
    patch_n = rs.rand(3, ph, pw).astype(np.float32)
    xy_n, th_n = _random_case(rs, B, ph, pw)
    gen = torch.Generator().manual_seed(3)
    w = [(torch.randn(D, 3, 14, 14, generator=gen) * 0.05).to(torch.bfloat16) for D in (D0, D1)]
    dy = [(torch.randn(B, D, 16, 16, generator=gen) * 0.1).to(torch.bfloat16) for D in (D0, D1)]  # gradient w.r.t. the conv outputs [B,D,16,16]
    # ---- reference chain on the CPU ----
    p = torch.from_numpy(patch_n).clone().requires_grad_(True)
    x = ref_port.apply_random_patch_batch(list(imgs), p, xy_n, th_n, True).to(torch.bfloat16)
    e0 = torch.nn.functional.conv2d(x[:, :3], w[0], stride=14)
    e1 = torch.nn.functional.conv2d(x[:, 3:], w[1], stride=14)
    torch.autograd.backward([e0, e1], [dy[0], dy[1]])
    want = p.grad.numpy()
    # ---- K2' ----
    patch, xy, th = _t(patch_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    _, keep = ops.patch_apply_fwd(_t(imgs), patch, xy, th, True, 0)
    wp = [ops.pack_embed_weights(ww.reshape(ww.shape[0], 588).t().contiguous().to(DEV)) for ww in w]
    tok = [d.flatten(2).transpose(1, 2).contiguous().to(DEV) for d in dy]  # [B,256,D], token t = ty*16 + tx (timm: x.flatten(2).transpose(1, 2))
    got = ops.patch_embed_grad_gather(tok[0], tok[1], wp[0], wp[1], patch, xy, th, keep, True).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-2 * np.abs(want).max()  # bf16 conv backward on the CPU vs fp32-accumulated MFMA rounded to bf16
    assert np.corrcoef(got.ravel(), want.ravel())[0, 1] > 0.99999


def test_patch_embed_grad_gather_multi_vs_oracle(ops):
    """K2' with one patch per image (resize_patch=True): per-image gradients against the oracle fed by an fp32 host matmul, folded to
    pixel layout and rounded to bf16 per tower (image by image through vaa_oracle_patch_grad_multi)."""
    B, D0, D1 = 5, 128, 64
    rs = np.random.RandomState(17)
    imgs = synthetic.synth_images(6, B, "noise")
    sizes = np.array([[61, 61], [139, 139], [100, 80], [30, 120], [75, 75]], np.int32)  # 139x139: more than one row band
    pdesc_n, total = ops.make_pdesc(sizes)
    packed_n = rs.rand(total).astype(np.float32)
    xy_n = np.stack([[rs.randint(0, 224 - w + 1), rs.randint(0, 224 - h + 1)] for h, w in sizes]).astype(np.int32)
    _, th_n = _random_case(rs, B, 50, 50)
    gen = torch.Generator(device=DEV).manual_seed(4)
    dy = [(torch.randn(B, 256, D, device=DEV, generator=gen) * 0.1).to(torch.bfloat16) for D in (D0, D1)]
    w = [(torch.randn(D, 588, device=DEV, generator=gen) * 0.05).to(torch.bfloat16) for D in (D0, D1)]
    packed, pdesc, xy, th = _t(packed_n), _t(pdesc_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    mh = (int(sizes[:, 0].max()), int(sizes[:, 1].max()))
    _, keep = ops.patch_apply_fwd_multi(_t(imgs), packed, pdesc, mh, xy, th, True, 0)
    got = ops.patch_embed_grad_gather_multi(dy[0], dy[1], ops.pack_embed_weights(w[0].t().contiguous()), ops.pack_embed_weights(w[1].t().contiguous()),
                                            packed, pdesc, mh, xy, th, keep, True).cpu().numpy()
    fold = lambda d, ww: (d.float().cpu() @ ww.float().cpu()).to(torch.bfloat16).view(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)
    gcat = torch.cat([fold(dy[0], w[0]), fold(dy[1], w[1])], dim=1).contiguous()
    want = c_oracle.patch_grad_multi(_bits(gcat), packed_n, pdesc_n, xy_n, th_n, 1, 0)
    for (h, ww_, off, _z) in pdesc_n:
        a, b = got[off : off + 3 * h * ww_], want[off : off + 3 * h * ww_]
        assert np.abs(a - b).max() <= 5e-3 * np.abs(b).max() + 1e-9  # one bf16 ulp of a tile gradient: per-image results have few terms per texel
    unf = ops.patch_grad_gather_multi(gcat.to(DEV), packed, pdesc, mh, xy, th, keep, True).cpu().numpy()  # the unfused HIP path on the same bf16 gradient
    assert np.abs(unf - want).max() <= 3e-6 * np.abs(want).max()


def test_patch_embed_tile_kernel_tower_split_matches_unsplit(ops):
    """Small batches run the tile kernel with one tower per workgroup and let the gather add the two towers' tile gradients; larger ones
    keep both towers in one workgroup. Same fp32 add either way: the per-image gradients of the same 8 images agree to the last bits
    whether they are a batch of 8 (split) or the head of a batch of 48 (unsplit) — not bitwise, only because the gather cuts the patch into a
    different number of row bands for the two batch sizes (each band rounds to its own 2^-30 fixed-point quantum)."""
    Bs, Bl, D0, D1 = 8, 48, 128, 192
    rs = np.random.RandomState(41)
    imgs = synthetic.synth_images(9, Bl, "noise")
    sizes = np.full((Bl, 2), 50, np.int32)
    pdesc_n, total = ops.make_pdesc(sizes)
    packed = _t(rs.rand(total).astype(np.float32))
    xy_n, th_n = _random_case(rs, Bl, 50, 50)
    gen = torch.Generator(device=DEV).manual_seed(8)
    dy = [(torch.randn(Bl, 256, D, device=DEV, generator=gen) * 0.1).to(torch.bfloat16) for D in (D0, D1)]
    wp = [ops.pack_embed_weights((torch.randn(588, D, device=DEV, generator=gen) * 0.05).to(torch.bfloat16)) for D in (D0, D1)]
    pdesc, xy, th = _t(pdesc_n), _t(xy_n, torch.int32), _t(th_n.reshape(-1, 6))
    _, keep = ops.patch_apply_fwd_multi(_t(imgs), packed, pdesc, (50, 50), xy, th, True, 0)
    big = ops.patch_embed_grad_gather_multi(dy[0], dy[1], wp[0], wp[1], packed, pdesc, (50, 50), xy, th, keep, True)
    n8 = 8 * 3 * 50 * 50
    small = ops.patch_embed_grad_gather_multi(dy[0][:Bs].contiguous(), dy[1][:Bs].contiguous(), wp[0], wp[1], packed[:n8].contiguous(), pdesc[:Bs].contiguous(),
                                              (50, 50), xy[:Bs].contiguous(), th[:Bs].contiguous(), keep[:Bs].contiguous(), True)
    assert float((small - big[:n8]).abs().max()) <= 2e-7 * float(big[:n8].abs().max()) and float(small.abs().max()) > 0


def test_patch_embed_pack_weights_layout_and_errors(ops):
    """vaa_patch_embed_pack_weights writes the layout include/vaa.h / vaa_patch_grad.hip document:
    packed[(((nb*nchunk + kc)*2 + h)*64 + lane)*8 + e] = W^T[nb*16 + (lane & 15)][kc*64 + (lane >> 4)*16 + h*8 + e], zero for columns >= 588."""
    D = 192
    wt = (torch.randn(588, D, device=DEV) * 0.1).to(torch.bfloat16)
    packed = ops.pack_embed_weights(wt).view(37, D // 64, 2, 64, 8).cpu()
    full = torch.zeros(592, D, dtype=torch.bfloat16)
    full[:588] = wt.cpu()
    nb, kc, h, lane, e = torch.meshgrid(torch.arange(37), torch.arange(D // 64), torch.arange(2), torch.arange(64), torch.arange(8), indexing="ij")
    want = full[nb * 16 + (lane & 15), kc * 64 + (lane >> 4) * 16 + h * 8 + e]
    assert torch.equal(packed.view(torch.int16), want.view(torch.int16))
    with pytest.raises(ValueError):
        ops.pack_embed_weights((torch.randn(588, 96, device=DEV)).to(torch.bfloat16))  # not a multiple of 64
    from roboticattack_amd import _lib

    L = _lib.lib()
    d = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    rc = L.vaa_patch_embed_grad_gather(d.data_ptr(), 96, d.data_ptr(), 64, d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(), d.data_ptr(),
                                       1, 50, 50, 1, 0, _lib.f32x([0.5] * 6), 1, d.data_ptr(), d.data_ptr(), 1 << 30, None)
    assert rc == -1 and b"64" in L.vaa_last_error()  # VAA_E_INVALID: tower widths must be multiples of 64


@pytest.mark.parametrize("B,ph,pw,geo,D0,D1", [(6, 50, 50, 1, 64, 192), (3, 22, 31, 0, 64, 64), (4, 100, 100, 1, 128, 64), (64, 50, 50, 1, 1024, 1152),
                                                (2, 50, 50, 1, 1216, 64)])  # the last one: a tower too wide for the LDS-resident variant
def test_patch_embed_grad_gather_vs_unfused(ops, B, ph, pw, geo, D0, D1):
    """K2' (8f-3): patch-embed backward restricted to the kept tiles + gather == K2 on the dense pixel gradient dY @ W (folded back to
    pixel layout and rounded to bf16 like the model's own backward hands it over)."""
    from roboticattack_amd import benchmarks, synthetic

    g = torch.Generator(device=DEV).manual_seed(B * 7 + ph)
    img = torch.from_numpy(synthetic.synth_images(77, B, "noise")).to(DEV)
    patch = torch.rand(3, ph, pw, device=DEV, generator=g)
    xy_n, th_n = benchmarks.random_params(B, ph, pw, 5)
    xy, th = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    _, keep = ops.patch_apply_fwd(img, patch, xy, th if geo else None, bool(geo), ops.MASK_LT_M20, want_keep=True)
    dy0 = (torch.randn(B, 256, D0, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    dy1 = (torch.randn(B, 256, D1, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    w0 = (torch.randn(D0, 588, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    w1 = (torch.randn(D1, 588, device=DEV, generator=g) * 0.05).to(torch.bfloat16)

    def fold(dy, w):  # [B,256,D] @ [D,588] -> [B,3,224,224] (inverse of the unfold in Vit.forward)
        t = (dy.float() @ w.float()).to(torch.bfloat16)
        return t.view(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)

    gout = torch.cat([fold(dy0, w0), fold(dy1, w1)], dim=1).contiguous()
    ref = ops.patch_grad_gather(gout, patch, xy, th if geo else None, keep, bool(geo))
    got = ops.patch_embed_grad_gather(dy0, dy1, ops.pack_embed_weights(w0.t().contiguous()), ops.pack_embed_weights(w1.t().contiguous()), patch, xy, th if geo else None, keep, bool(geo))
    # same bf16 rounding point; the only difference is the fp32 summation order inside the two GEMMs (rare 1-ulp bf16 flips)
    assert (got - ref).abs().max() <= 2e-3 * ref.abs().max() + 1e-7
    exact = ops.patch_embed_grad_gather(dy0, dy1, ops.pack_embed_weights(w0.t().contiguous()), ops.pack_embed_weights(w1.t().contiguous()), patch, xy, th if geo else None, keep, bool(geo),
                                        round_bf16=False)
    assert (exact - ref).abs().max() <= 1e-2 * ref.abs().max() + 1e-7
    # ORACLE leg (no HIP code on this side): the patch-embed backward as an fp32 matmul on the host, folded to pixel layout, rounded to
    # bf16 per tower like the model's own backward hands it over, then the plain-C gather (oracle/vaa_oracle.c:vaa_oracle_patch_grad)
    def fold_cpu(dy, w):
        t = (dy.float().cpu() @ w.float().cpu()).to(torch.bfloat16)
        return t.view(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)

    gout_cpu = torch.cat([fold_cpu(dy0, w0), fold_cpu(dy1, w1)], dim=1).contiguous()
    theta_o = th_n.reshape(B, 2, 3) if geo else np.tile(np.eye(3, dtype=np.float32)[:2], (B, 1, 1))
    og = c_oracle.patch_grad(_bits(gout_cpu), patch.cpu().numpy(), xy_n, theta_o, int(geo), 0)
    assert np.abs(got.cpu().numpy() - og).max() <= 2e-3 * np.abs(og).max() + 1e-7  # bf16 rounding flips of the tile gradients (GEMM order)
    assert np.abs(ref.cpu().numpy() - og).max() <= 2e-3 * np.abs(og).max() + 1e-7


@pytest.mark.parametrize("tool,seconds,seed", [("soak_parity.py", 45, 101), ("soak_loss.py", 20, 102), ("soak_loss.py --head", 20, 103)])
def test_randomised_soak_leg(tool, seconds, seed):
    """A fixed-seed, time-boxed leg of the randomised parity soaks (tools/soak_parity.py: K0/K1/K2/K2'/K5 against the plain-C oracle over
    random patch sizes 1..224, batches, edge-biased placements, general affines, per-image patches; tools/soak_loss.py: K3 in all modes,
    layouts and dtypes; `--head`: K3h over row counts 1..128, head widths, ties across workgroups) inside the driver's own `pytest -m gpu` run — the K1 hole at bs > 64 of round 2 was found by exactly this tool."""
    import subprocess
    import sys

    from conftest import ROOT

    tool, *flags = tool.split()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), *flags, "--seconds", str(seconds), "--seed", str(seed)],
                         capture_output=True, text=True, cwd=ROOT, timeout=seconds * 6 + 300)
    tail = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and " 0 failures" in tail, (out.stdout[-3000:], out.stderr[-2000:])
    n_cases = int(tail.split(":")[1].split("cases")[0])
    assert n_cases >= 20, tail  # the leg really ran


def test_patch_embed_grad_updated_pixels_bench_shape(ops):
    """What production runs (K2' feeding K4) at the bench shape — 64 images, 3x50x50, towers 1024 / 1152 — measured where the north-star
    tolerance is stated: on the UPDATED PIXELS. Ten AdamW steps (fresh placements and upstream gradients every step) are taken twice from the
    same start: once with K2' gradients, once with the oracle's (fp32 host matmul of the SAME bf16 operands, bf16 rounding per tower like
    the model's own backward, plain-C gather, oracle AdamW). Pixels must agree <= 1e-4 after the first and after the tenth step; the
    distribution of the gradient differences |dg| / max|g| is printed so the 2e-3 bound of the op-level tests is characterised."""
    from roboticattack_amd import benchmarks, synthetic

    B, ph, pw, D0, D1 = 64, 50, 50, 1024, 1152
    g = torch.Generator(device=DEV).manual_seed(2024)
    img = torch.from_numpy(synthetic.synth_images(77, B, "noise")).to(DEV)
    w0 = (torch.randn(D0, 588, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    w1 = (torch.randn(D1, 588, device=DEV, generator=g) * 0.02).to(torch.bfloat16)
    wp0, wp1 = ops.pack_embed_weights(w0.t().contiguous()), ops.pack_embed_weights(w1.t().contiguous())
    patch_h = torch.rand(3, ph, pw, device=DEV, generator=g)
    patch_o = patch_h.cpu().numpy().copy().ravel()
    m_h, v_h = torch.zeros_like(patch_h), torch.zeros_like(patch_h)
    m_o, v_o = np.zeros(3 * ph * pw, np.float32), np.zeros(3 * ph * pw, np.float32)
    lr = 2e-3  # the peak learning rate of the shipped UADA script is 2e-3 (scripts/run_UADA.sh); AdamW moves a pixel by <= ~lr per step
    rel = []
    pix_err, pix_over = [], []
    for step in range(1, 11):
        xy_n, th_n = benchmarks.random_params(B, ph, pw, 100 + step)
        xy, th = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
        # both trajectories paste the HIP trajectory's patch: the masks (keep bits) then coincide and the test isolates the gradient path
        _, keep = ops.patch_apply_fwd(img, patch_h, xy, th, True, ops.MASK_LT_M20, want_keep=True)
        dy0 = (torch.randn(B, 256, D0, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
        dy1 = (torch.randn(B, 256, D1, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
        got = ops.patch_embed_grad_gather(dy0, dy1, wp0, wp1, patch_h, xy, th, keep, True)

        def fold_cpu(dy, w):
            t = (dy.float().cpu() @ w.float().cpu()).to(torch.bfloat16)
            return t.view(B, 16, 16, 3, 14, 14).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, 224, 224)

        gout_cpu = torch.cat([fold_cpu(dy0, w0), fold_cpu(dy1, w1)], dim=1).contiguous()
        og = c_oracle.patch_grad(_bits(gout_cpu), patch_h.cpu().numpy(), xy_n, th_n.reshape(B, 2, 3), 1, 0)
        d = np.abs(got.cpu().numpy() - og).ravel() / np.abs(og).max()
        rel.append(d)
        ops.patch_update(patch_h, got, m_h, v_h, ops.OPT_ADAMW_HF, lr, step)
        c_oracle.patch_update(patch_o, og.ravel().copy(), m_o, v_o, 0, lr, step)
        dp = np.abs(patch_h.cpu().numpy().ravel() - patch_o)
        pix_err.append(float(dp.max()))
        pix_over.append(int((dp > 1e-4).sum()))
    rel = np.concatenate(rel)
    q = np.quantile(rel, [0.5, 0.9, 0.99, 0.999, 1.0])
    print(f"\nK2' vs oracle gradient, |dg|/max|g| over {rel.size} texel-channels x steps: median {q[0]:.2e}  p90 {q[1]:.2e}  p99 {q[2]:.2e}  "
          f"p99.9 {q[3]:.2e}  max {q[4]:.2e};  share above 1e-4: {float((rel > 1e-4).mean()):.4f}, above 1e-3: {float((rel > 1e-3).mean()):.5f}")
    print("updated-pixel max |dp| after steps 1..10:", " ".join(f"{e:.2e}" for e in pix_err), "| pixels above 1e-4:", pix_over)
    assert q[4] <= 2e-3
    assert pix_err[0] <= 1e-4 and pix_err[-1] <= 1e-4 and max(pix_err) <= 1e-4


def _planar_keep_to_tiles(keep_u8, B):
    """[B,3,6272] keep bytes (bit p&7 of byte p>>3) -> [B,3,256,14] u16 words (bit x of word (c, tile, y))."""
    bits = np.unpackbits(keep_u8.reshape(B, 3, -1), axis=2, bitorder="little").reshape(B, 3, 16, 14, 16, 14)  # [b,c,ty,y,tx,x]
    w = (bits.astype(np.uint32) << np.arange(14, dtype=np.uint32)).sum(axis=5)                                   # [b,c,ty,y,tx]
    return w.transpose(0, 1, 2, 4, 3).reshape(B, 3, 256, 14).astype(np.uint16)


@pytest.mark.parametrize("B,ph,pw,geo,mask", [(5, 50, 50, 1, 0), (3, 22, 31, 0, 0), (2, 100, 100, 1, 0), (96, 50, 50, 1, 0), (4, 50, 50, 0, 1),
                                              (3, 224, 224, 1, 0), (2, 1, 1, 1, 0)])
def test_patch_apply_tiles_equals_planar_k1(ops, B, ph, pw, geo, mask):
    """K1 in tile-major form (vaa_patch_apply_fwd_tiles) against the golden-pinned planar K1 on the same inputs: every bf16 value of both
    GEMM operands BIT-EXACT (== im2col of the planar tensor), keep words == the planar keep bits, tile flags == "any kept pixel in the
    tile"; placements include the frame edges and corners (the ownership rule of the two roles is per tile here)."""
    rs = np.random.RandomState(B * 131 + ph)
    imgs = _t(synthetic.synth_images(3 + B, B, "noise"))
    patch = _t(rs.rand(3, ph, pw).astype(np.float32))
    xy_n, th_n = _random_case(rs, B, ph, pw, edge_frac=0.5)
    xy, th = _t(xy_n, torch.int32), _t(th_n.reshape(B, 6))
    out, keep = ops.patch_apply_fwd(imgs, patch, xy, th if geo else None, bool(geo), mask)
    t0, t1, keep_t, flags = ops.patch_apply_fwd_tiles(imgs, patch, xy, th if geo else None, bool(geo), mask)
    want0, want1 = ops.unfold_tiles(out[:, :3]).contiguous(), ops.unfold_tiles(out[:, 3:]).contiguous()
    assert torch.equal(t0.view(torch.int16), want0.view(torch.int16)) and torch.equal(t1.view(torch.int16), want1.view(torch.int16))
    kt = _planar_keep_to_tiles(keep.cpu().numpy(), B)
    assert np.array_equal(keep_t.cpu().numpy().view(np.uint16), kt)
    assert np.array_equal(flags.cpu().numpy() != 0, (kt != 0).any(axis=(1, 3)))
    if geo or mask == 0:
        assert int(flags.sum()) > 0


def test_patch_apply_tiles_per_image_patches(ops):
    """The tile-major K1 with one patch per image (pdesc; resize_patch=True) against the planar per-image K1."""
    rs = np.random.RandomState(17)
    B = 5
    sizes = np.stack([rs.randint(30, 140, B), rs.randint(30, 140, B)], axis=1).astype(np.int32)
    pdesc_n, total = ops.make_pdesc(sizes)
    packed = _t(rs.rand(total).astype(np.float32))
    imgs = _t(synthetic.synth_images(23, B, "noise"))
    xy_n = np.stack([[rs.randint(0, 225 - w), rs.randint(0, 225 - h)] for h, w in sizes]).astype(np.int32)
    _, th_n = _random_case(rs, B, 50, 50)
    pdesc, xy, th = _t(pdesc_n), _t(xy_n, torch.int32), _t(th_n.reshape(B, 6))
    max_hw = (int(sizes[:, 0].max()), int(sizes[:, 1].max()))
    out, keep = ops.patch_apply_fwd_multi(imgs, packed, pdesc, max_hw, xy, th, True, 0)
    t0, t1, keep_t, flags = ops.patch_apply_fwd_tiles(imgs, packed, xy, th, True, 0, pdesc=pdesc, max_hw=max_hw)
    assert torch.equal(t0.view(torch.int16), ops.unfold_tiles(out[:, :3]).contiguous().view(torch.int16))
    assert torch.equal(t1.view(torch.int16), ops.unfold_tiles(out[:, 3:]).contiguous().view(torch.int16))
    kt = _planar_keep_to_tiles(keep.cpu().numpy(), B)
    assert np.array_equal(keep_t.cpu().numpy().view(np.uint16), kt) and np.array_equal(flags.cpu().numpy() != 0, (kt != 0).any(axis=(1, 3)))


@pytest.mark.parametrize("B,ph,pw,geo,D0,D1", [(6, 50, 50, 1, 64, 192), (64, 50, 50, 1, 1024, 1152), (3, 22, 31, 0, 64, 64), (40, 50, 50, 1, 128, 64)])
def test_patch_embed_grad_gather_tiles_equals_planar_mask_form(ops, B, ph, pw, geo, D0, D1):
    """K2' fed by the tile-major mask (keep words + tile flags of vaa_patch_apply_fwd_tiles) == K2' fed by the planar keep bits, BITWISE:
    the tile list, the MFMA products and the integer scatter are the same, only the mask's memory layout differs. Also with the final
    fixed-order sum left to the caller (gpatch == NULL: partial tiles in the workspace)."""
    from roboticattack_amd import benchmarks

    g = torch.Generator(device=DEV).manual_seed(B * 7 + ph)
    img = torch.from_numpy(synthetic.synth_images(77, B, "noise")).to(DEV)
    patch = torch.rand(3, ph, pw, device=DEV, generator=g)
    xy_n, th_n = benchmarks.random_params(B, ph, pw, 5)
    xy, th = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    _, keep = ops.patch_apply_fwd(img, patch, xy, th if geo else None, bool(geo), ops.MASK_LT_M20, want_keep=True)
    _, _, keep_t, flags = ops.patch_apply_fwd_tiles(img, patch, xy, th if geo else None, bool(geo), ops.MASK_LT_M20)
    dy0 = (torch.randn(B, 256, D0, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    dy1 = (torch.randn(B, 256, D1, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    wp0 = ops.pack_embed_weights((torch.randn(588, D0, device=DEV, generator=g) * 0.05).to(torch.bfloat16))
    wp1 = ops.pack_embed_weights((torch.randn(588, D1, device=DEV, generator=g) * 0.05).to(torch.bfloat16))
    ref = ops.patch_embed_grad_gather(dy0, dy1, wp0, wp1, patch, xy, th if geo else None, keep, bool(geo))
    got = ops.patch_embed_grad_gather_tiles(dy0, dy1, wp0, wp1, patch, xy, th if geo else None, keep_t, flags, bool(geo))
    assert torch.equal(ref, got) and float(ref.abs().max()) > 0
    parts = ops.patch_embed_grad_gather_tiles(dy0, dy1, wp0, wp1, patch, xy, th if geo else None, keep_t, flags, bool(geo), defer_reduce=True)
    assert parts.shape == (min(B, 512), 3 * ph * pw)
    assert torch.allclose(parts.double().sum(0).float().view_as(ref), ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("B,dtype", [(64, torch.bfloat16), (5, torch.float32)])
def test_step_epilogue_equals_separate_launches(ops, B, dtype):
    """vaa_step_epilogue (one launch: K2's final fixed-order sum + K3's fold + the DDP message) against the launches it replaces:
    msg[0..n) BITWISE the gradient of the un-deferred K2', scalars / prediction maps / gradient slice BITWISE those of
    vaa_loss_rows_fwd_bwd, msg[n..n+4) = {CE, w^2*MSE, UAD, total}; and the pass-through form (rowmap == NULL)."""
    from roboticattack_amd import benchmarks
    from roboticattack_amd.labels import mask_labels

    g = torch.Generator(device=DEV).manual_seed(B)
    img = torch.from_numpy(synthetic.synth_images(7, B, "noise")).to(DEV)
    patch = torch.rand(3, 50, 50, device=DEV, generator=g)
    xy_n, th_n = benchmarks.random_params(B, 50, 50, 9)
    xy, th = torch.from_numpy(xy_n).to(DEV), torch.from_numpy(th_n).to(DEV)
    _, _, keep_t, flags = ops.patch_apply_fwd_tiles(img, patch, xy, th, True)
    D0, D1 = 128, 64
    dy0 = (torch.randn(B, 256, D0, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    dy1 = (torch.randn(B, 256, D1, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    wp0 = ops.pack_embed_weights((torch.randn(588, D0, device=DEV, generator=g) * 0.05).to(torch.bfloat16))
    wp1 = ops.pack_embed_weights((torch.randn(588, D1, device=DEV, generator=g) * 0.05).to(torch.bfloat16))
    want_g = ops.patch_embed_grad_gather_tiles(dy0, dy1, wp0, wp1, patch, xy, th, keep_t, flags, True)
    _, labels, _ = synthetic.synth_text_batch(31, B)
    labels = mask_labels(labels, [0, 3]).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    logits = (torch.randn(R, 32064, device=DEV, generator=g) * 2).to(dtype)
    rm = ops.LossRowMap(labels)
    want_s, want_p, want_pf, want_gs = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA_DDP, w=5.0, grad_kind=ops.GRAD_SLICE)
    want_s, want_gs = want_s.clone(), want_gs.clone()
    # the split form
    n = 3 * 50 * 50
    gsl = torch.full((R, 256), float("nan"), dtype=dtype, device=DEV)
    ws = ops.loss_rows_stats(logits, rm, ops.LOSS_UADA_DDP, w=5.0, grad=gsl)
    parts = ops.patch_embed_grad_gather_tiles(dy0, dy1, wp0, wp1, patch, xy, th, keep_t, flags, True, defer_reduce=True)
    msg = torch.full((n + 4,), float("nan"), device=DEV)
    scal = torch.full((8,), float("nan"), device=DEV)
    pred, pred_full = ops.step_epilogue(parts, msg, scal, rowmap=rm, R=R, V=32064, mode=ops.LOSS_UADA_DDP, w=5.0, loss_ws=ws)
    assert torch.equal(msg[:n].view_as(want_g), want_g)
    assert torch.equal(scal, want_s) and torch.equal(pred, want_p) and torch.equal(pred_full, want_pf)
    assert torch.equal(gsl.view(torch.int16) if dtype == torch.bfloat16 else gsl, want_gs.view(torch.int16) if dtype == torch.bfloat16 else want_gs)
    assert torch.equal(msg[n:], want_s[[1, 2, 7, 0]])
    # a caller's R other than the map's row count: a NaN total in the scalars and the message; the rows both know are folded as ever
    msg_r, scal_r = torch.zeros(n + 4, device=DEV), torch.zeros(8, device=DEV)
    ops.step_epilogue(parts, msg_r, scal_r, rowmap=rm, R=R - 1, V=32064, mode=ops.LOSS_UADA_DDP, w=5.0, loss_ws=ws)
    assert torch.isnan(scal_r[0]) and torch.isnan(msg_r[n + 3]) and float(scal_r[5]) == R - 1 and torch.equal(msg_r[:n], msg[:n])
    # pass-through form: the scalars are final already (modes whose gradient needs them ran vaa_loss_rows_fwd_bwd), only the message is built
    msg2 = torch.zeros(n + 4, device=DEV)
    ops.step_epilogue(parts, msg2, want_s)
    assert torch.equal(msg2[:n], msg[:n]) and torch.equal(msg2[n:], want_s[[1, 2, 7, 0]])
    # the single-GPU form: K4 applied inside the epilogue == vaa_patch_update on the same gradient, bitwise in patch / m / v
    for opt_mode in (ops.OPT_ADAMW_HF, ops.OPT_PGD_SIGN):
        p_a, p_b = patch.clone(), patch.clone()
        m_a, v_a = torch.rand_like(patch) * 1e-3, torch.rand_like(patch) * 1e-6
        m_b, v_b = m_a.clone(), v_a.clone()
        st = ops.patch_update(p_a, want_g, m_a, v_a, opt_mode, 2e-3, 7).clone()
        sp = torch.zeros(((n + 63) // 64, 2), dtype=torch.float64, device=DEV)
        msg3 = torch.zeros(n + 4, device=DEV)
        ops.step_epilogue(parts, msg3, want_s, update=dict(patch=p_b, m=m_b, v=v_b, mode=opt_mode, lr=2e-3, step=7, stat_part=sp))
        assert torch.equal(p_a, p_b) and torch.equal(msg3[:n], msg[:n]) and float((p_b - patch).abs().max()) > 0
        if opt_mode == ops.OPT_ADAMW_HF:
            assert torch.equal(m_a, m_b) and torch.equal(v_a, v_b)
        tot = sp.sum(0)
        assert torch.allclose(torch.stack([tot[0], tot[1] / n]).float(), st, rtol=1e-6, atol=0)
    # vaa_loss_rows_stats refuses modes whose gradient depends on the folded scalars
    from roboticattack_amd import _lib

    with pytest.raises(_lib.VaaError):
        ops.loss_rows_stats(logits, rm, ops.LOSS_UPA, grad=gsl)


def test_patch_embed_grad_gather_multi_tiles_equals_planar_mask_form(ops):
    """K2' with one patch per image (resize_patch=True) fed by the tile-major mask == the planar-mask form, bitwise."""
    rs = np.random.RandomState(4)
    B, D0, D1 = 5, 64, 128
    sizes = np.stack([rs.randint(40, 140, B), rs.randint(40, 140, B)], axis=1).astype(np.int32)
    pdesc_n, total = ops.make_pdesc(sizes)
    packed = _t(rs.rand(total).astype(np.float32))
    imgs = _t(synthetic.synth_images(29, B, "noise"))
    xy_n = np.stack([[rs.randint(0, 225 - w), rs.randint(0, 225 - h)] for h, w in sizes]).astype(np.int32)
    _, th_n = _random_case(rs, B, 50, 50)
    pdesc, xy, th = _t(pdesc_n), _t(xy_n, torch.int32), _t(th_n.reshape(B, 6))
    max_hw = (int(sizes[:, 0].max()), int(sizes[:, 1].max()))
    gen = torch.Generator(device=DEV).manual_seed(8)
    dy = [(torch.randn(B, 256, D, device=DEV, generator=gen) * 0.1).to(torch.bfloat16) for D in (D0, D1)]
    wp = [ops.pack_embed_weights((torch.randn(588, D, device=DEV, generator=gen) * 0.05).to(torch.bfloat16)) for D in (D0, D1)]
    _, keep = ops.patch_apply_fwd_multi(imgs, packed, pdesc, max_hw, xy, th, True, 0)
    _, _, keep_t, flags = ops.patch_apply_fwd_tiles(imgs, packed, xy, th, True, 0, pdesc=pdesc, max_hw=max_hw)
    ref = ops.patch_embed_grad_gather_multi(dy[0], dy[1], wp[0], wp[1], packed, pdesc, max_hw, xy, th, keep, True)
    got = ops.patch_embed_grad_gather_multi_tiles(dy[0], dy[1], wp[0], wp[1], packed, pdesc, max_hw, xy, th, keep_t, flags, True)
    assert torch.equal(ref, got) and float(ref.abs().max()) > 0


def test_round3_entry_points_error_paths_and_empty_batches(ops):
    """Argument checking of the round-3 entry points through the C-ABI: null pointers, bad sizes, the un-warped mask rule with a warp,
    workspace too small, modes the split K3 form does not cover, empty batches (no-ops), and the per-dispatch timer's bookkeeping."""
    import ctypes as C

    from roboticattack_amd import _lib

    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    d = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    p = d.data_ptr()
    f6 = _lib.f32x([0.5] * 6)
    # K1 tile-major
    assert L.vaa_patch_apply_fwd_tiles(p, p, None, p, p, 0, 50, 50, 1, 0, f6, f6, p, p, p, p, st) == 0                      # empty batch
    assert L.vaa_patch_apply_fwd_tiles(None, p, None, p, p, 2, 50, 50, 1, 0, f6, f6, p, p, p, p, st) == -1                   # null image
    assert L.vaa_patch_apply_fwd_tiles(p, p, None, p, None, 2, 50, 50, 1, 0, f6, f6, p, p, p, p, st) == -1                   # geometry without theta
    assert L.vaa_patch_apply_fwd_tiles(p, p, None, p, p, 2, 225, 50, 1, 0, f6, f6, p, p, p, p, st) == -2                     # patch larger than the frame
    assert L.vaa_patch_apply_fwd_tiles(p, p, None, p, p, 2, 50, 50, 1, 1, f6, f6, p, p, p, p, st) == -2 and b"geometry=0" in L.vaa_last_error()
    # K2' tile-major: keep words without flags, widths, workspace
    a = (p, 64, p, 64, p, p, p, p, p)
    assert L.vaa_patch_embed_grad_gather_tiles(*a, p, None, 2, 50, 50, 1, 0, f6, 1, p, p, 1 << 30, st) == -1
    assert L.vaa_patch_embed_grad_gather_tiles(p, 96, p, 64, p, p, p, p, p, p, p, 2, 50, 50, 1, 0, f6, 1, p, p, 1 << 30, st) == -1
    assert L.vaa_patch_embed_grad_gather_tiles(*a, p, p, 2, 50, 50, 1, 0, f6, 1, p, p, 1024, st) == -4 and b"workspace" in L.vaa_last_error()
    assert L.vaa_patch_grad_partials(0) == 0 and L.vaa_patch_grad_partials(64) == 64 and L.vaa_patch_grad_partials(5000) == 512
    # split K3 form + epilogue
    prm = _lib.f32x([5.0, 0.8, 0.2, 1.0])
    assert L.vaa_loss_rows_stats(p, 1, p, 8, 4, 10, 32064, ops.LOSS_UPA, prm, p, 1, p, 1 << 20, st) == -1 and b"VAA_LOSS_UADA_DDP" in L.vaa_last_error()
    assert L.vaa_loss_rows_stats(p, 1, p, 8, 4, 10, 32064, ops.LOSS_UADA_DDP, prm, p, 1, p, 16, st) == -4
    assert L.vaa_loss_rows_stats(p, 1, p, 100, 4, 10, 32064, ops.LOSS_UADA_DDP, prm, p, 1, p, 1 << 20, st) == -1             # R > B*(L-1)
    assert L.vaa_step_epilogue(None, 4, 7500, None, 0, 0, 0, 0, 0, prm, None, 0, p, None, None, p, st) == -1
    assert L.vaa_step_epilogue(p, 0, 7500, None, 0, 0, 0, 0, 0, prm, None, 0, p, None, None, p, st) == -1
    assert L.vaa_step_epilogue_update(p, 4, 100, None, 0, 0, 0, 0, 0, prm, None, 0, p, None, None, p, None, p, p, 0, 1e-3, 0.9, 0.999, 1e-6, 1, None, st) == -1
    assert L.vaa_step_epilogue_update(p, 4, 100, None, 0, 0, 0, 0, 0, prm, None, 0, p, None, None, p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-6, 0, None, st) == -1  # AdamW step 0
    assert L.vaa_step_epilogue_update(p, 4, 100, None, 0, 0, 0, 0, 0, prm, None, 0, p, None, None, p, p, p, p, 7, 1e-3, 0.9, 0.999, 1e-6, 1, None, st) == -1  # unknown mode
    # per-dispatch timer: records exactly the launches made while armed, capacity respected, names are the kernels'
    patch = torch.rand(3, 8, 8, device=DEV)
    g = torch.rand_like(patch)
    m, v = torch.zeros_like(patch), torch.zeros_like(patch)
    ops.prof_start(2)
    for t in range(1, 4):
        ops.patch_update(patch, g, m, v, ops.OPT_ADAMW_HF, 1e-3, t)
    recs = ops.prof_collect()
    assert len(recs) == 2 and all("patch_update_kernel" in n and 0.5 < us < 500 for n, us in recs)
    ops.patch_update(patch, g, m, v, ops.OPT_ADAMW_HF, 1e-3, 4)   # disarmed: nothing recorded
    assert L.vaa_prof_stop() == 2 and L.vaa_prof_get(5, None, C.byref(C.c_float())) == -1 and L.vaa_prof_start(-1) == -1
    ops.prof_start(0)
    assert ops.prof_collect() == []
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("B,maskidx,mode,dtype", [(64, [0], "UADA", torch.bfloat16), (16, [0, 3], "UADA", torch.float32), (8, list(range(7)), "CE", torch.bfloat16),
                                                  (3, [0], "UADA", torch.bfloat16)])
def test_k3_one_pass_equals_two_launches(ops, monkeypatch, B, maskidx, mode, dtype):
    """K3 full-row gradients (single-GPU UADA: 1/CE, UADA.py:145-148; TMA's CE, TMA.py:148) as ONE launch — statistics, grid-wide hand-over,
    gradient from the registers — are bit for bit the two-launch form's: scalars, both prediction maps, the gradient; repeated launches on one
    stream (the hand-over words re-arm themselves) and launches on a second stream (its own words) included."""
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(4242 + B, B)
    labels = mask_labels(labels, maskidx).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    g0 = torch.Generator(device=DEV).manual_seed(B)
    logits = (torch.randn(R, 32064, device=DEV, generator=g0) * 2).to(dtype)
    rm = ops.LossRowMap(labels)
    kmode = {"UADA": ops.LOSS_UADA, "CE": ops.LOSS_CE}[mode]

    def run(stream=None):
        g = torch.full_like(logits, float("nan"))
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            sc, pred, pred_full, _ = ops.loss_rows_fwd_bwd(logits, rm, kmode, w=5.0, grad_kind=ops.GRAD_FULL, grad=g)
        torch.cuda.synchronize()
        return [t.clone() for t in (sc, pred, pred_full, g)]

    def same(a, b):
        return all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y) or
                   (x.is_floating_point() and torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x.float()), torch.nan_to_num(y.float())))
                   for x, y in zip(a, b))

    monkeypatch.setenv("VAA_K3_ONE_PASS", "0")
    ref = run()
    assert torch.isfinite(ref[3].float()).all()
    monkeypatch.setenv("VAA_K3_ONE_PASS", "1")
    ops.prof_start(16)
    one = run()
    names = [n for n, _ in ops.prof_collect()]
    assert len(names) == 1 and "rows_stats_kernel" in names[0], names  # really one launch
    assert same(ref, one)
    for _ in range(5):
        assert same(ref, run())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    assert same(ref, run(side))
    assert same(ref, run())


@pytest.mark.gpu
def test_k3_full_rows_under_capture_and_beyond_half_residency(ops):
    """The one-launch form of K3's full-row gradient is admitted only outside stream capture (its hand-over generation is a launch argument) and
    for grids of at most half the resident slots: a captured graph and an fp32 launch of 1,024 workgroups take the two launches — same bits."""
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(99, 16)
    labels = mask_labels(labels, [0, 1]).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    g0 = torch.Generator(device=DEV).manual_seed(5)
    logits = (torch.randn(R, 32064, device=DEV, generator=g0) * 2).to(torch.bfloat16)
    rm = ops.LossRowMap(labels)
    grad = torch.zeros_like(logits)
    sc, pred, pred_full, _ = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=grad)
    torch.cuda.synchronize()
    ref = [t.clone() for t in (sc, pred, pred_full, grad)]
    # captured: the launch sequence inside the graph is statistics + finishing launch; replays reproduce the eager (one-launch) result
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    gout = torch.zeros_like(logits)
    with torch.cuda.stream(side):
        ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=gout)  # warm-up on the capture stream
        with torch.cuda.graph(g, stream=side):
            out = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=gout)
    torch.cuda.synchronize()
    for _ in range(3):
        gout.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])
        assert torch.equal(gout.view(torch.int16), ref[3].view(torch.int16))
    # 1,024 workgroups (fp32, R' = 256, four parts per row) exceed half of the device's resident slots: two launches, checked against the oracle elsewhere;
    # here: the launch count and the agreement of its scalars with the bf16-free recomputation in fp64
    _, lab2, _ = synthetic.synth_text_batch(7, 64)
    lab2 = mask_labels(lab2, [0, 1, 2, 3]).to(DEV)
    R2 = int((lab2[:, 1:] != -100).sum())
    z2 = torch.randn(R2, 32064, device=DEV, generator=g0) * 2
    rm2 = ops.LossRowMap(lab2)
    ops.prof_start(16)
    sc2, _, _, g2 = ops.loss_rows_fwd_bwd(z2, rm2, ops.LOSS_CE, w=5.0, grad_kind=ops.GRAD_FULL)
    torch.cuda.synchronize()
    names = [n for n, _ in ops.prof_collect()]
    if R2 * 4 * 2 > 1024:  # the admission rule on this part (256 CUs x 4 resident workgroups of this kernel)
        assert len(names) == 2, names
    tgt = lab2[:, 1:][lab2[:, 1:] != -100]
    ce = torch.nn.functional.cross_entropy(z2.double(), tgt, reduction="mean")
    assert abs(float(sc2[1]) - float(ce)) <= 3e-5 * max(1.0, abs(float(ce)))
    assert torch.isfinite(g2).all()


@pytest.mark.gpu
def test_k3_one_pass_handover_timeout_fails_loudly(ops, monkeypatch):
    """Fail loud, never NaN: the opt-in one-launch K3 whose grid-wide hand-over runs out of polls (forced here with
    VAA_K3_HANDOVER_POLLS=0: every waiting workgroup gives up at once) NaN-poisons the gradient AND raises the library's failure word — the NEXT
    library call of the process returns VAA_E_LAUNCH with the reason, and so does every later one (the word is sticky) until vaa_async_error(), the
    explicit poll, reports and clears it. The default form (two launches)
    has no hand-over and is unaffected."""
    from roboticattack_amd import _lib
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(11, 64)
    labels = mask_labels(labels, [0]).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    logits = (torch.randn(R, 32064, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 2).to(torch.bfloat16)
    rm = ops.LossRowMap(labels)
    ops.async_error_check()  # clean before
    monkeypatch.delenv("VAA_K3_ONE_PASS", raising=False)
    ops.prof_start(8)
    _, _, _, g_ref = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL)
    torch.cuda.synchronize()
    assert len(ops.prof_collect()) == 2 and torch.isfinite(g_ref.float()).all()  # two launches by default
    monkeypatch.setenv("VAA_K3_ONE_PASS", "1")
    monkeypatch.setenv("VAA_K3_HANDOVER_POLLS", "0")
    g = torch.zeros_like(logits)
    try:  # with 0 polls the kernel may give up before the call's own launch check reads the (sticky) word: the call itself may then raise
        ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=g)
    except _lib.VaaError as e:
        assert "hand-over timed out" in str(e)
    torch.cuda.synchronize()
    assert torch.isnan(g.float()).any()  # poisoned, never stale or silently partial
    patch = torch.rand(3, 8, 8, device=DEV)
    for _ in range(2):  # every later library call, whatever it is, reports the failure: the word is sticky, no call consumes it ...
        with pytest.raises(_lib.VaaError, match="hand-over timed out"):
            ops.patch_update(patch, torch.rand_like(patch), torch.zeros_like(patch), torch.zeros_like(patch), ops.OPT_ADAMW_HF, 1e-3, 1)
    with pytest.raises(_lib.VaaError, match="vaa_async_error"):       # ... until the explicit poll reports and clears it
        ops.async_error_check()
    ops.async_error_check()                                           # clean again
    ops.patch_update(patch, torch.rand_like(patch), torch.zeros_like(patch), torch.zeros_like(patch), ops.OPT_ADAMW_HF, 1e-3, 1)
    with pytest.raises(_lib.VaaError, match="hand-over timed out"):  # the failing call itself already sees its own failure if the kernel has run by its check;
        ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=g)  # (it has not: launches are asynchronous) ...
        torch.cuda.synchronize()
        ops.async_error_check()                                       # ... so the poll behind the synchronisation is what raises
    monkeypatch.delenv("VAA_K3_HANDOVER_POLLS")
    g2 = torch.zeros_like(logits)
    ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_UADA, w=5.0, grad_kind=ops.GRAD_FULL, grad=g2)  # un-forced: the one-launch form works and agrees
    torch.cuda.synchronize()
    ops.async_error_check()
    assert torch.equal(g2.view(torch.int16), g_ref.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("B,maskidx,D", [(8, [0], 4096), (32, [0], 4096), (64, [0], 4096), (5, [0, 3], 192), (13, [0, 1, 2], 320), (3, [6], 64)])
def test_head_loss_rows_stats_vs_oracle_and_gemm_path(ops, B, maskidx, D):
    """SURVEY.md 8f-2 as written: LM head FUSED with K3's statistics (vaa_head_loss_rows_stats; the attack step uses it up to 128 labelled rows). Checked three ways on the same hidden rows and head weight:
      * its bf16 logits (test-only dump) == the hipBLASLt head's bf16 logits on > 99 % of them, and within half a bf16 step + the fp32 accumulation
        error of the exact (fp64) products everywhere;
      * the C ORACLE fed with those very logits: loss scalars <= 3e-5, gradient slice <= 1e-2 of its scale (bf16 storage), both argmax maps exact;
      * vaa_loss_rows_stats fed with those very logits: gradient slice and slice statistics BIT FOR BIT, CE to fp32 summation order.
    Shapes: OpenVLA's head (D = 4096) at bs = 8 / 32 / 64 and small towers incl. D not a multiple of 256 (padded k-steps) and ragged row counts."""
    from roboticattack_amd.labels import mask_labels

    V = 32064
    rs = np.random.RandomState(B * 11 + D)
    _, labels, _ = synthetic.synth_text_batch(500 + B, B)
    labels = mask_labels(labels, maskidx)
    L = labels.shape[1]
    rows = _rows(labels.numpy())
    R = len(rows)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    g = torch.Generator(device=DEV).manual_seed(B + D)
    W = (torch.randn(V, D, device=DEV, generator=g) * (1.3 / np.sqrt(D))).to(torch.bfloat16)
    W[31744:32000] *= 2.0  # spread the action logits
    h = torch.randn(R, D, device=DEV, generator=g).to(torch.bfloat16)
    rm = ops.LossRowMap(labels.to(DEV))
    assert ops.head_loss_rows_applies(R, D, V)
    gs = torch.full((R, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    ws, lg = ops.head_loss_rows_stats(h, W, rm, ops.LOSS_UADA_DDP, 5.0, grad=gs, want_logits=True)
    n = 7500
    parts, msg = torch.zeros((4, n), device=DEV), torch.zeros(n + 4, device=DEV)
    sc = torch.zeros(8, device=DEV)
    pred, pred_full = ops.step_epilogue(parts, msg, sc, rowmap=rm, R=R, V=V, mode=ops.LOSS_UADA_DDP, w=5.0, loss_ws=ws)
    torch.cuda.synchronize()
    # (1) the logits are the head's
    ref_lg = torch.nn.functional.linear(h, W)
    assert float((lg != ref_lg).float().mean()) < 0.01
    # ... and against the exact products: half a bf16 step at the value + what an fp32 accumulation of D terms may carry (2e-6 of the sum of
    # the terms' magnitudes — a near-zero logit is a sum of large cancelling terms, and the GEMM library's own summation order is not fixed)
    ref64, mag = h.double() @ W.double().t(), h.double().abs() @ W.double().abs().t()
    assert bool(((lg.double() - ref64).abs() <= 0.5 * torch.maximum(ref64.abs(), lg.double().abs()) * 2.0 ** -7 + 2e-6 * mag + 1e-30).all())
    del ref64, mag
    # (2) the oracle on the kernel's own logits
    full = torch.zeros((B, 256 + L, V), dtype=torch.float32)
    full[torch.from_numpy(rb), torch.from_numpy(rp)] = lg.float().cpu()
    so, go = c_oracle.loss(full.numpy(), labels.numpy(), c_oracle.MODE_UADA_DDP, w=5.0)
    gor = go[rb, rp][:, 31744:32000]
    assert np.allclose(sc.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5), (sc.cpu().numpy(), so)
    assert float(sc[5]) == R  # (UAD, scalars[7], is checked through the product's statistics kernel below: the oracle reports it elsewhere)
    assert np.abs(gs.float().cpu().numpy() - gor).max() <= 1e-2 * max(np.abs(gor).max(), 1e-30) and np.abs(gor).max() > 0
    zf = lg.float().cpu().numpy()
    pf, ps = pred_full.cpu().numpy().reshape(B, L - 1), pred.cpu().numpy().reshape(B, L - 1)
    for i, (b, p) in enumerate(rows):
        k = p - 256
        assert pf[b, k] == int(zf[i].argmax())
        if labels[b, k + 1] > 2:
            assert ps[b, k] == 31744 + int(zf[i, 31744:32000].argmax())
    assert int((pf >= 0).sum()) == R
    # (3) the product's statistics kernel on the same logits: same bits where the arithmetic is the same
    gs2 = torch.empty_like(gs)
    sc2 = torch.zeros(8, device=DEV)
    ws2 = ops.loss_rows_stats(lg, rm, ops.LOSS_UADA_DDP, 5.0, grad=gs2)
    pred2, pred_full2 = ops.step_epilogue(parts, msg, sc2, rowmap=rm, R=R, V=V, mode=ops.LOSS_UADA_DDP, w=5.0, loss_ws=ws2)
    assert torch.equal(gs2.view(torch.int16), gs.view(torch.int16)) and torch.equal(pred2, pred) and torch.equal(pred_full2, pred_full)
    assert torch.equal(sc2[[2, 6, 7]], sc[[2, 6, 7]]) and abs(float(sc2[1]) - float(sc[1])) <= 2e-6 * abs(float(sc2[1]))
    # bitwise repeatable
    gs3 = torch.empty_like(gs)
    ops.head_loss_rows_stats(h, W, rm, ops.LOSS_UADA_DDP, 5.0, grad=gs3)
    sc3 = torch.zeros(8, device=DEV)
    ops.step_epilogue(parts, msg, sc3, rowmap=rm, R=R, V=V, mode=ops.LOSS_UADA_DDP, w=5.0, loss_ws=ws)
    assert torch.equal(gs3.view(torch.int16), gs.view(torch.int16)) and torch.equal(sc3, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("B,maskidx", [(64, [0]), (32, [0]), (8, [0, 1, 2])])
def test_head_stats_production_launch_equals_dumping_launch(ops, B, maskidx):
    """K3h's oracle check goes through the test-only logits dump (`logits_dbg`) — so the PRODUCTION launch (no dump) is tied
    to the dumping launch directly: at OpenVLA's head (D = 4096) and 128 / 64 / 32 labelled rows both launches leave the SAME bytes in the
    head's workspace (every workgroup's PartStat of every row + the bf16 action-slice logits) and in K3's workspace (the folded per-row
    statistics head_finish_kernel writes), and the same gradient slice. Both workspaces are filled with a byte pattern before each launch, so
    a part one launch wrote and the other did not would differ."""
    from roboticattack_amd import _lib
    from roboticattack_amd.labels import mask_labels

    V, D = 32064, 4096
    _, labels, _ = synthetic.synth_text_batch(700 + B, B)
    labels = mask_labels(labels, maskidx)
    R = int((labels[:, 1:] != -100).sum())
    assert R == B * (len(maskidx) + 1)
    g = torch.Generator(device=DEV).manual_seed(3 * B + 1)
    W = (torch.randn(V, D, device=DEV, generator=g) * (1.3 / np.sqrt(D))).to(torch.bfloat16)
    h = torch.randn(R, D, device=DEV, generator=g).to(torch.bfloat16)
    rm = ops.LossRowMap(labels.to(DEV))
    L = _lib.lib()
    n_ws, n_hws = L.vaa_loss_rows_ws_bytes(R), L.vaa_head_loss_ws_bytes(R, V)
    got = []
    for dump in (False, True):
        for kind, nb in (("k3", n_ws), ("k3h", n_hws)):
            ops._workspace(torch.device(DEV), nb, kind).fill_(0xAB)
        gs = torch.full((R, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
        ws, hws, lg = ops._head_stats(h, W, rm, ops.LOSS_UADA_DDP, 5.0, 0.8, 0.2, 1.0, gs, dump)
        torch.cuda.synchronize()
        assert (lg is not None) == dump
        got.append((ws[:n_ws].clone(), hws[:n_hws].clone(), gs.view(torch.int16).clone()))
    (ws0, hws0, g0), (ws1, hws1, g1) = got
    assert torch.equal(hws0, hws1), "per-workgroup PartStats / slice logits differ between the production and the dumping launch"
    assert torch.equal(ws0, ws1) and torch.equal(g0, g1)
    assert int((hws0 != 0xAB).sum()) > R * 251 * 8 and not bool(torch.isnan(got[0][2].view(torch.bfloat16).float()).any())  # ... and they were written


@pytest.mark.gpu
@pytest.mark.parametrize("mode_name", ["UPA", "UADA_DDP", "UADA", "CE"])
@pytest.mark.parametrize("B,maskidx,D", [(13, [0, 1, 2], 192), (32, [0, 1, 2], 4096), (16, [0, 1, 2, 3, 4, 5, 6], 256)])
def test_head_loss_rows_fwd_bwd_without_logits(ops, mode_name, B, maskidx, D):
    """Every K3 mode evaluated WITHOUT logits in memory: vaa_head_loss_rows_stats + vaa_head_loss_rows_finish (UPA and UADA_DDP with their gradient
    slice; UADA / CE evaluation only, their gradients need every logit) against
      * vaa_loss_rows_fwd_bwd on the kernel's own bf16 logits: predictions, slice statistics, UAD and the gradient slice BIT FOR BIT (the finishing pass
        is the same kernel reading the same 256 action logits from the head's buffer), CE / total to fp32 summation order;
      * the C ORACLE on those logits: scalars <= 3e-5, gradient slice <= 1e-2 of its scale (bf16 storage)."""
    from roboticattack_amd.labels import mask_labels

    V = 32064
    mode = {"UPA": ops.LOSS_UPA, "UADA_DDP": ops.LOSS_UADA_DDP, "UADA": ops.LOSS_UADA, "CE": ops.LOSS_CE}[mode_name]
    om = {"UPA": c_oracle.MODE_UPA, "UADA_DDP": c_oracle.MODE_UADA_DDP, "UADA": c_oracle.MODE_UADA, "CE": c_oracle.MODE_CE}[mode_name]
    _, labels, _ = synthetic.synth_text_batch(900 + B, B)
    labels = mask_labels(labels, maskidx)
    L = labels.shape[1]
    rows = _rows(labels.numpy())
    R = len(rows)
    rb, rp = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    g = torch.Generator(device=DEV).manual_seed(B * 7 + D)
    W = (torch.randn(V, D, device=DEV, generator=g) * (1.3 / np.sqrt(D))).to(torch.bfloat16)
    W[31744:32000] *= 2.0
    h = torch.randn(R, D, device=DEV, generator=g).to(torch.bfloat16)
    rm = ops.LossRowMap(labels.to(DEV))
    want_grad = mode in ops.SLICE_MODES
    kw = dict(w=4.0, alpha=0.7, beta=0.3, scale=1.0)
    sc, pred, pf, gs, lg = ops.head_loss_rows_fwd_bwd(h, W, rm, mode, want_grad=want_grad, want_logits=True, **kw)
    sc2, pred2, pf2, gs2 = ops.loss_rows_fwd_bwd(lg, rm, mode, want_grad=want_grad, grad_kind=ops.GRAD_SLICE, **kw)
    torch.cuda.synchronize()
    assert torch.equal(pred, pred2) and torch.equal(pf, pf2)
    assert torch.equal(sc[[2, 5, 6, 7]], sc2[[2, 5, 6, 7]]) and torch.allclose(sc, sc2, rtol=3e-6, atol=1e-7), (sc, sc2)
    if want_grad:
        assert torch.equal(gs.view(torch.int16), gs2.view(torch.int16)) and float(gs.float().abs().max()) > 0
    else:
        assert gs is None
        with pytest.raises(Exception, match="cross-entropy"):
            ops.head_loss_rows_fwd_bwd(h, W, rm, mode, want_grad=True, **kw)
    full = torch.zeros((B, 256 + L, V), dtype=torch.float32)
    full[torch.from_numpy(rb), torch.from_numpy(rp)] = lg.float().cpu()
    so, go = c_oracle.loss(full.numpy(), labels.numpy(), om, **kw)
    assert np.allclose(sc.cpu().numpy()[:5], so[:5], rtol=3e-5, atol=3e-5), (sc.cpu().numpy(), so)
    if want_grad:
        gor = go[rb, rp][:, 31744:32000]
        assert np.abs(gs.float().cpu().numpy() - gor).max() <= 1e-2 * max(np.abs(gor).max(), 1e-30)


@pytest.mark.gpu
def test_head_loss_rows_stats_argument_checks(ops):
    import ctypes as C

    from roboticattack_amd import _lib

    L = _lib.lib()
    p, st = C.c_void_p(0x1000), None
    prm = _lib.f32x([5.0, 0.8, 0.2, 1.0])
    assert L.vaa_head_loss_rows_applies(128, 4096, 32064) == 1 and L.vaa_head_loss_rows_applies(129, 4096, 32064) == 0
    assert L.vaa_head_loss_rows_applies(16, 4100, 32064) == 0 and L.vaa_head_loss_rows_applies(16, 4096, 30000) == 0
    assert L.vaa_head_loss_ws_bytes(0, 32064) == 0 and L.vaa_head_loss_ws_bytes(16, 32064) >= 16 * 251 * 16 + 16 * 256 * 2
    a = (p, p, 4096, p, 16, 8, 30, 32064)
    assert L.vaa_head_loss_rows_stats(None, p, 4096, p, 16, 8, 30, 32064, ops.LOSS_UADA_DDP, prm, p, p, 1 << 20, p, 1 << 24, None, st) == -1
    assert L.vaa_head_loss_rows_stats(p, p, 4096, p, 200, 100, 30, 32064, ops.LOSS_UADA_DDP, prm, p, p, 1 << 20, p, 1 << 24, None, st) == -2 and b"GEMM" in L.vaa_last_error()
    assert L.vaa_head_loss_rows_stats(*a, ops.LOSS_UPA, prm, p, p, 1 << 20, p, 1 << 24, None, st) == -1 and b"UADA_DDP" in L.vaa_last_error()
    assert L.vaa_head_loss_rows_stats(C.c_void_p(0x1008), p, 4096, p, 16, 8, 30, 32064, ops.LOSS_UADA_DDP, prm, p, p, 1 << 20, p, 1 << 24, None, st) == -1 and b"aligned" in L.vaa_last_error()
    assert L.vaa_head_loss_rows_stats(*a, ops.LOSS_UADA_DDP, prm, p, p, 16, p, 1 << 24, None, st) == -4
    assert L.vaa_head_loss_rows_stats(*a, ops.LOSS_UADA_DDP, prm, p, p, 1 << 20, p, 16, None, st) == -4 and b"workspace" in L.vaa_last_error()
    assert L.vaa_head_loss_rows_stats(p, p, 4096, p, 100, 8, 10, 32064, ops.LOSS_UADA_DDP, prm, p, p, 1 << 20, p, 1 << 24, None, st) == -2  # R > B*(L-1)
    # the finishing pass: a gradient slice only for UPA (UADA_DDP's is written by the statistics call, CE terms need the [R,V] logits)
    f = (p, 16, 8, 30, 32064)
    assert L.vaa_head_loss_rows_finish(*f, ops.LOSS_UADA, prm, p, 1 << 20, p, 1 << 24, p, None, None, p, st) == -2 and b"GEMM" in L.vaa_last_error()
    assert L.vaa_head_loss_rows_finish(*f, ops.LOSS_UADA_DDP, prm, p, 1 << 20, p, 1 << 24, p, None, None, p, st) == -1
    assert L.vaa_head_loss_rows_finish(*f, ops.LOSS_UPA, prm, p, 1 << 20, p, 16, p, None, None, p, st) == -4
    assert L.vaa_head_loss_rows_finish(*f, ops.LOSS_UPA, prm, p, 16, p, 1 << 24, p, None, None, p, st) == -4
    assert L.vaa_head_loss_rows_finish(*f, ops.LOSS_UPA, prm, p, 1 << 20, p, 1 << 24, None, None, None, None, st) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("B,maskidx,dtype", [(8, list(range(7)), torch.bfloat16), (64, [0], torch.bfloat16), (16, [0, 1], torch.float32)])
def test_k3_ce_gradient_with_the_fold_in_its_own_workgroup(ops, monkeypatch, B, maskidx, dtype):
    """TMA's CE gradient (TMA.py:148): the finishing launch with the fold moved to one extra workgroup (the gradient workgroups need the row's own
    parts and the row count only) gives the bits of the form in which every workgroup folds — scalars, prediction maps, gradient."""
    from roboticattack_amd.labels import mask_labels

    _, labels, _ = synthetic.synth_text_batch(777 + B, B)
    labels = mask_labels(labels, maskidx).to(DEV)
    R = int((labels[:, 1:] != -100).sum())
    g0 = torch.Generator(device=DEV).manual_seed(B)
    logits = (torch.randn(R, 32064, device=DEV, generator=g0) * 2).to(dtype)
    rm = ops.LossRowMap(labels)
    outs = []
    for mode in ("0", "1"):
        monkeypatch.setenv("VAA_K3_CE_FOLD_WG", mode)
        g = torch.full_like(logits, float("nan"))
        sc, pred, pred_full, _ = ops.loss_rows_fwd_bwd(logits, rm, ops.LOSS_CE, w=5.0, scale=0.25, grad_kind=ops.GRAD_FULL, grad=g)
        torch.cuda.synchronize()
        assert torch.isfinite(g.float()).all() and torch.isfinite(sc).all()
        outs.append((sc.clone(), pred.clone(), pred_full.clone(), g.clone()))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
