"""K12 (vaa_jpeg_roundtrip) on the GPU: byte for byte against the NumPy integer restatement of include/vaa.h (jpeg_ref.roundtrip) on every
frame and quality of tests/golden/jpeg_pillow.npz, against the recorded codec itself, its buffer discipline and refusals, and eval_frames /
evaluate_patch with the JPEG step against the same steps composed by hand. No tolerance anywhere: both sides are integer arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _k12(frames, qt, rot180=False):
    from roboticattack_amd import ops

    fr = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    out = ops.jpeg_roundtrip(fr, qt, rot180)
    assert out.dtype == torch.uint8 and out.shape == fr.shape
    return out.cpu().numpy()


def test_kernel_is_the_integer_restatement_on_every_fixture_frame_and_quality():
    g = jpeg_ref.golden()
    z = g["z"]
    for n, q in g["cases"]:
        f, qt = z["in_" + n], z["qt_q%d" % q]
        got = _k12(f[None], qt)[0]
        bad = got != g["ref"][(n, q)]
        assert not bad.any(), "%s q=%d: %d bytes differ, first at %s" % (n, q, int(bad.sum()), np.argwhere(bad)[0].tolist())
        got = _k12(f[None], qt, rot180=True)[0]
        bad = got != jpeg_ref.roundtrip(f, qt, rot180=True)
        assert not bad.any(), "%s q=%d rot180: %d bytes differ, first at %s" % (n, q, int(bad.sum()), np.argwhere(bad)[0].tolist())


def test_kernel_statistics_against_the_recorded_codec():
    """The distance to the recorded Pillow / libjpeg-turbo output that tests/test_jpeg_host.py measured for jpeg_ref — (0, 0, 0) in every
    case — holds for the kernel, from the fixture alone."""
    g = jpeg_ref.golden()
    z = g["z"]
    for n, q in g["cases"]:
        got = _k12(z["in_" + n][None], z["qt_q%d" % q])[0]
        assert jpeg_ref.stats(got, z["out_%s_q%d" % (n, q)]) == jpeg_ref.stats(g["ref"][(n, q)], z["out_%s_q%d" % (n, q)]) == (0.0, 0.0, 0), (n, q)


@pytest.mark.parametrize("rot", [False, True])
def test_batch_rows_equal_single_frames(rot):
    g = jpeg_ref.golden()
    z = g["z"]
    batch = np.stack([z["in_ramp"], z["in_noise"], z["in_sines"]])
    for q in (95, 50):
        qt = z["qt_q%d" % q]
        got = _k12(batch, qt, rot)
        for i, n in enumerate(("ramp", "noise", "sines")):
            assert np.array_equal(got[i], _k12(batch[i:i + 1], qt, rot)[0])
            assert np.array_equal(got[i], g["ref"][(n, q)] if not rot else jpeg_ref.roundtrip(batch[i], qt, rot180=True))


def test_more_than_one_workgroup_per_mcu_row():
    """64 x 264: 17 MCUs per row (two chroma workgroups, three luminance workgroups per MCU row, the last ones partly empty), W % 4 == 0 and
    W % 16 != 0; 40 x 130: the byte-store path (W % 4 != 0) across a workgroup boundary."""
    rng = np.random.default_rng(5)
    qt = jpeg_ref.qtables(90)
    for H, W in ((64, 264), (40, 130)):
        yy, xx = np.mgrid[0:H, 0:W]
        f = np.clip(np.stack([xx, 2 * yy, xx + yy], -1) + rng.integers(0, 60, (H, W, 3)), 0, 255).astype(np.uint8)
        for rot in (False, True):
            assert np.array_equal(_k12(f[None], qt, rot)[0], jpeg_ref.roundtrip(f, qt, rot180=rot)), (H, W, rot)


def test_buffer_discipline():
    from roboticattack_amd import _lib, ops

    z = jpeg_ref.golden()["z"]
    f, qt = z["in_odd17x33"], ops.jpeg_qtables(75)
    n, guard = f.size, 64
    src = torch.from_numpy(f).to(DEV)
    keep = src.clone()
    buf = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    dev_qt = torch.from_numpy(qt.view(np.int16).copy()).to(DEV)
    L = _lib.lib()
    nws = L.vaa_jpeg_roundtrip_ws_bytes(1, 17, 33)
    wsb = torch.full((guard + nws + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 8 == 0 and wsb.data_ptr() % 8 == 0

    def run():
        rc = L.vaa_jpeg_roundtrip(src.data_ptr(), 1, 17, 33, 0, qt.ctypes.data, dev_qt.data_ptr(), buf.data_ptr() + guard, wsb.data_ptr() + guard, nws,
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.vaa_last_error()
        torch.cuda.synchronize()
        return buf.cpu().numpy().copy()

    # a canary that the round trip of this frame cannot produce everywhere: check against the restatement, which covers every byte
    first = run()
    want = jpeg_ref.roundtrip(f, qt)
    assert np.array_equal(first[guard:guard + n].reshape(f.shape), want)          # every byte written (equal to the restatement)
    buf[guard:guard + n] = 0x3C                                                    # a second canary value: no byte survives either
    second = run()
    assert np.array_equal(second, first)                                           # same bits; guards included
    assert (first[:guard] == 0xA5).all() and (first[guard + n:] == 0xA5).all()
    w = wsb.cpu().numpy()
    assert (w[:guard] == 0x5A).all() and (w[guard + nws:] == 0x5A).all()
    assert torch.equal(src, keep)
    assert L.vaa_async_error() == 0


def test_refusals_return_their_codes_and_launch_nothing():
    from roboticattack_amd import _lib, ops

    L = _lib.lib()
    H, W = 32, 40
    src = torch.zeros((2, H, W, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((2, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    qt = ops.jpeg_qtables(95)
    dq = torch.from_numpy(qt.view(np.int16).copy()).to(DEV)
    nws = L.vaa_jpeg_roundtrip_ws_bytes(2, H, W)
    ws = torch.zeros(nws + 64, dtype=torch.uint8, device=DEV)

    def call(B=2, H=H, W=W, rot=0, qh=qt, qd=dq.data_ptr(), s=src.data_ptr(), d=dst.data_ptr(), w=ws.data_ptr(), wb=nws):
        return L.vaa_jpeg_roundtrip(s, B, H, W, rot, qh.ctypes.data if qh is not None else None, qd, d, w, wb, None)

    zero, big = qt.copy(), qt.copy()
    zero[1, 63] = 0
    big[0, 0] = 256
    ops.prof_start(64)
    assert call(B=0) == 0 and call(B=-1) == -1
    assert call(H=7) == -1 and call(W=7) == -1 and call(H=2049) == -1 and call(W=2049) == -1
    assert call(rot=2) == -1
    assert call(s=None) == -1 and call(d=None) == -1 and call(qh=None) == -1 and call(qd=None) == -1
    assert call(s=src.data_ptr() + 2) == -1 and call(d=dst.data_ptr() + 1) == -1 and call(qd=dq.data_ptr() + 1) == -1
    assert call(d=src.data_ptr()) == -1 and b"overlap" in L.vaa_last_error()
    assert call(B=1, d=src.data_ptr() + H * W * 3 - 4) == -1 and b"overlap" in L.vaa_last_error()
    assert call(qh=zero) == -1 and call(qh=big) == -1 and b"1..255" in L.vaa_last_error()
    assert call(w=None) == -4 and call(wb=nws - 1) == -4 and call(w=ws.data_ptr() + 4) == -4
    assert ops.prof_collect() == []                      # no dispatch was recorded
    torch.cuda.synchronize()
    assert bool((dst == 7).all())
    for shape in ((1, 7, 64, 3), (1, 64, 2049, 3)):
        with pytest.raises(_lib.VaaError):
            ops.jpeg_roundtrip(torch.zeros(shape, dtype=torch.uint8, device=DEV), qt)
    with pytest.raises(_lib.VaaError):
        ops.jpeg_roundtrip(src, qt[:1])
    assert tuple(ops.jpeg_roundtrip(src[:0], qt).shape) == (0, H, W, 3)
    ops.prof_start(64)
    assert call() == 0
    assert [n for n, _ in ops.prof_collect()] == ["jpeg_chroma_kernel", "jpeg_luma_finish_kernel"]
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy()[0], jpeg_ref.roundtrip(np.zeros((H, W, 3), np.uint8), qt)) and L.vaa_async_error() == 0


def test_eval_frames_with_a_quality_is_k12_then_k8():
    from roboticattack_amd import ops
    from roboticattack_amd.transform import RandomPatchTransform

    z = jpeg_ref.golden()["z"]
    cam = np.stack([z["in_sines"], z["in_noise"]])
    t = RandomPatchTransform(DEV)
    got = t.eval_frames(cam, rot180=True, jpeg_quality=95)
    by_hand = ops.resize_frames(ops.jpeg_roundtrip(torch.from_numpy(cam).to(DEV), ops.jpeg_qtables(95), True), False)
    assert torch.equal(got, by_hand) and tuple(got.shape) == (2, 224, 224, 3)
    want = np.stack([jpeg_ref.roundtrip(f, jpeg_ref.qtables(95), rot180=True) for f in cam])
    assert torch.equal(got, ops.resize_frames(torch.from_numpy(want).to(DEV), False))
    assert torch.equal(t.eval_frames(cam, True), ops.resize_frames(torch.from_numpy(cam).to(DEV), True))  # without: K8 alone, as before
    assert not torch.equal(got, t.eval_frames(cam, True))


def test_evaluate_patch_with_the_jpeg_step_and_unchanged_without():
    import decode_ref
    from roboticattack_amd import ops
    from roboticattack_amd.attack.evaluate import clean_agreement, evaluate_patch
    from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
    from roboticattack_amd.openvla_model import build_openvla, tiny_cfg
    from roboticattack_amd.transform import RandomPatchTransform

    t = RandomPatchTransform(DEV)
    model = build_openvla(tiny_cfg(), device=DEV, dtype=torch.bfloat16)
    ids, mask, _ = decode_ref.prompt_batch(11, lens=(5, 9, 12), device=DEV)
    patch = torch.from_numpy(np.random.RandomState(3).rand(3, 50, 50).astype(np.float32))
    placements = [(True, 10.0, 0.1, 0.1, 0, 0), (False, 0.0, 0.0, 0.0, 87, 60)]
    kw = dict(center_crop=True, crop_scale=0.9, mean=[MEAN0, MEAN1], std=[STD0, STD1], bs=4)
    z = jpeg_ref.golden()["z"]
    cam = np.stack([z["in_sines"], z["in_noise"], z["in_ramp"]])
    rep = evaluate_patch(model, t, cam, ids, mask, patch, placements, resize="lanczos3", rot180=True, jpeg_quality=95, jpeg_compare=True, **kw)
    trip = ops.jpeg_roundtrip(torch.from_numpy(cam).to(DEV), ops.jpeg_qtables(95), True)
    assert np.array_equal(trip.cpu().numpy(), np.stack([jpeg_ref.roundtrip(f, jpeg_ref.qtables(95), rot180=True) for f in cam]))
    by_hand = evaluate_patch(model, t, ops.resize_frames(trip, False), ids, mask, patch, placements, **kw)
    assert tuple(rep["tokens_patched"].shape) == (2, 3, 7)
    assert torch.equal(rep["tokens_clean"], by_hand["tokens_clean"]) and torch.equal(rep["tokens_patched"], by_hand["tokens_patched"])
    # jpeg_quality=None: today's report
    plain = evaluate_patch(model, t, cam, ids, mask, patch, placements, resize="lanczos3", rot180=True, jpeg_quality=None, **kw)
    today = evaluate_patch(model, t, ops.resize_frames(torch.from_numpy(cam).to(DEV), True), ids, mask, patch, placements, **kw)
    assert sorted(plain) == sorted(today) and "jpeg_agreement" not in plain
    assert torch.equal(plain["tokens_clean"], today["tokens_clean"]) and torch.equal(plain["tokens_patched"], today["tokens_patched"])
    assert rep["jpeg_agreement"] == clean_agreement(rep["tokens_clean"], plain["tokens_clean"])
    assert sorted(set(rep) - set(plain)) == ["jpeg_agreement"]
    with pytest.raises(ValueError):
        evaluate_patch(model, t, ops.resize_frames(trip, False), ids, mask, patch, placements, jpeg_quality=95, **kw)
    torch.cuda.synchronize()
    ops.async_error_check()
