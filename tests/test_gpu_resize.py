"""K8 (vaa_frame_resize) on the GPU: byte for byte against the fp32 restatement of include/vaa.h (resize_ref.resize_f32), against the fp64
reference outside the tie band, and evaluate_patch on camera-sized frames against the same steps composed by hand."""
import numpy as np
import pytest
import torch

import resize_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_REF = {}


def _case(name):
    """(frames, fp32 restatement, fp64 values) of a case, computed once per process and left unchanged."""
    if name not in _REF:
        B, H, W, seed = resize_ref.CASES[name]
        fr = resize_ref.frames(B, H, W, seed)
        _REF[name] = (fr, resize_ref.resize_f32(fr), resize_ref.resize_f64(fr))
    return _REF[name]


def _resize(fr, rot180=False):
    from roboticattack_amd import ops

    out = ops.resize_frames(fr if isinstance(fr, torch.Tensor) else torch.from_numpy(fr).to(DEV), rot180)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (fr.shape[0], 224, 224, 3) and out.data_ptr() % 16 == 0
    return out.cpu().numpy()


def _check(got, r32, v64):
    bad = got != r32
    assert not bad.any(), "%d of %d bytes differ from the fp32 restatement, first at %s" % (int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())
    wrong, excluded = resize_ref.compare_f64(got, v64)
    assert excluded <= resize_ref.MAX_EXCLUDED and wrong == 0


@pytest.mark.parametrize("name", ["libero", "bridge", "upsample", "identity", "min", "tall", "wide_rows"])
def test_kernel_is_the_fp32_restatement(name):
    """256x256 (9 taps), 3 x 480x640 (15 and 19 taps, odd batch), 128x160 (upsampling, 7 taps), 224x224 (must copy), the two limits, and a row
    of more than 1024 pixels (the kernel's 4-row chunks)."""
    fr, r32, v64 = _case(name)
    got = _resize(fr)
    _check(got, r32, v64)
    if name == "identity":
        assert np.array_equal(got, fr)


def test_row_length_not_a_multiple_of_four_and_an_offset_base():
    """250x302: a row is 906 = 4*226 + 2 bytes, so rows start at every second offset inside a dword; the buffer's base is 4 bytes into a
    16-byte aligned allocation (the alignment the header allows)."""
    fr, r32, v64 = _case("odd_row_bytes")
    assert (fr.shape[2] * 3) % 4 == 2 and fr.size % 4 == 0
    flat = torch.zeros(fr.size + 20, dtype=torch.uint8, device=DEV)
    view = flat[4:4 + fr.size].view(fr.shape)
    view.copy_(torch.from_numpy(fr))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _check(_resize(view), r32, v64)
    # one row less: the byte count is no multiple of 4 and the buffer ends inside its last dword (the allocation itself goes on behind it)
    fr2 = np.ascontiguousarray(fr[:, :249])
    assert fr2.size % 4 == 2
    exact = torch.from_numpy(fr2).to(DEV)
    _check(_resize(exact), resize_ref.resize_f32(fr2), resize_ref.resize_f64(fr2))


def test_rot180_is_the_resize_of_the_flipped_frames():
    fr, r32, _ = _case("libero")
    got = _resize(fr, rot180=True)
    flipped = np.ascontiguousarray(fr[:, ::-1, ::-1])
    assert np.array_equal(got, _resize(flipped))
    _check(got, resize_ref.resize_f32(fr, rot180=True), resize_ref.resize_f64(fr, rot180=True))
    assert not np.array_equal(got, r32)
    fb, rb, _ = _case("odd_row_bytes")  # rows at odd offsets, rotated
    assert np.array_equal(_resize(fb, rot180=True), resize_ref.resize_f32(fb, rot180=True))


def test_batch_independent_and_deterministic():
    fr, r32, _ = _case("bridge")
    dev = torch.from_numpy(fr).to(DEV)
    a, b = _resize(dev), _resize(dev)
    assert np.array_equal(a, b)
    for i in range(fr.shape[0]):
        assert np.array_equal(_resize(dev[i:i + 1].clone()), a[i:i + 1])


def test_empty_batch_and_refused_arguments_launch_nothing():
    from roboticattack_amd import _lib, ops, resize

    out = ops.resize_frames(torch.zeros((0, 256, 256, 3), dtype=torch.uint8, device=DEV))
    assert tuple(out.shape) == (0, 224, 224, 3)
    for shape in ((1, 7, 64, 3), (1, 64, 2049, 3)):
        with pytest.raises(_lib.VaaError):
            ops.resize_frames(torch.zeros(shape, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.VaaError):
        ops.resize_frames(torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=DEV)[:, :, ::2])  # not contiguous
    # the C entry point's own codes on device operands
    L = _lib.lib()
    src = torch.zeros((1, 32, 40, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((1, 224, 224, 3), 7, dtype=torch.uint8, device=DEV)
    sx, wx, sy, wy = (np.ascontiguousarray(t) for t in resize.frame_taps(32, 40))
    taps = torch.from_numpy(resize.pack_taps(sx, wx, sy, wy)).to(DEV)

    def call(B=1, H=32, W=40, sx=sx, src_ptr=src.data_ptr(), dst_ptr=dst.data_ptr()):
        return L.vaa_frame_resize(src_ptr, B, H, W, 0, sx.ctypes.data, wx.ctypes.data, 7, sy.ctypes.data, wy.ctypes.data, 7, taps.data_ptr(), dst_ptr, None)

    bad = sx.copy()
    bad[223] = 40 - 6
    assert call(B=0) == 0 and call(B=-1) == -1 and call(H=7) == -2 and call(W=2049) == -2 and call(sx=bad) == -1
    assert call(src_ptr=src.data_ptr() + 2) == -2 and call(dst_ptr=dst.data_ptr() + 4) == -2 and call(src_ptr=None) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7).all())  # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dst == 0).all()) and L.vaa_async_error() == 0


def _tiny_eval():
    import decode_ref
    from roboticattack_amd.openvla_model import build_openvla, tiny_cfg
    from roboticattack_amd.transform import RandomPatchTransform

    t = RandomPatchTransform(DEV)
    model = build_openvla(tiny_cfg(), device=DEV, dtype=torch.bfloat16)
    ids, mask, _ = decode_ref.prompt_batch(11, lens=(5, 9, 12), device=DEV)
    patch = torch.from_numpy(np.random.RandomState(3).rand(3, 50, 50).astype(np.float32))
    placements = [(True, 10.0, 0.1, 0.1, 0, 0), (False, 0.0, 0.0, 0.0, 87, 60)]
    return t, model, ids, mask, patch, placements


def test_evaluate_patch_resizes_camera_frames_once_and_is_unchanged_without_the_keyword():
    from roboticattack_amd import ops
    from roboticattack_amd.attack.evaluate import evaluate_patch
    from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1

    t, model, ids, mask, patch, placements = _tiny_eval()
    kw = dict(center_crop=True, crop_scale=0.9, mean=[MEAN0, MEAN1], std=[STD0, STD1], bs=4)
    cam = resize_ref.frames(3, 256, 256, 21)
    for rot in (False, True):
        rep = evaluate_patch(model, t, cam, ids, mask, patch, placements, resize="lanczos3", rot180=rot, **kw)
        small = ops.resize_frames(torch.from_numpy(cam).to(DEV), rot)
        assert np.array_equal(small.cpu().numpy(), resize_ref.resize_f32(cam, rot180=rot))
        assert torch.equal(t.eval_frames(cam, rot), small)
        by_hand = evaluate_patch(model, t, small, ids, mask, patch, placements, **kw)
        assert tuple(rep["tokens_patched"].shape) == (2, 3, 7)
        assert torch.equal(rep["tokens_clean"], by_hand["tokens_clean"]) and torch.equal(rep["tokens_patched"], by_hand["tokens_patched"])
    # 224x224 frames without the keyword: today's path, token for token (the steps of the unchanged driver composed by hand)
    fr = resize_ref.frames(3, 224, 224, 22)
    rep = evaluate_patch(model, t, fr, ids, mask, patch, placements, **kw)
    clean = model.predict_action(ids, mask, t.eval_pixel_values(fr, kw["mean"], kw["std"], center_crop=True, crop_scale=0.9))[0].cpu()
    assert torch.equal(rep["tokens_clean"], clean)
    want = []
    for i in range(0, 6, 4):
        pairs = list(range(i, min(i + 4, 6)))
        rows = torch.tensor([r % 3 for r in pairs], device=DEV)
        geo, ang, shx, shy, pos = zip(*[(g, a, sx, sy, (x, y)) for g, a, sx, sy, x, y in (placements[r // 3] for r in pairs)])
        pasted = t.simulation_patch_batch(fr[rows.cpu().numpy()], patch, geo, ang, shx, shy, pos)
        want.append(model.predict_action(ids[rows], mask[rows], t.eval_pixel_values(pasted, kw["mean"], kw["std"], center_crop=True, crop_scale=0.9))[0].cpu())
    assert torch.equal(rep["tokens_patched"], torch.cat(want).view(2, 3, 7))
    with pytest.raises(ValueError):
        evaluate_patch(model, t, cam, ids, mask, patch, placements, **kw)  # camera-sized frames without the keyword
    torch.cuda.synchronize()
    ops.async_error_check()
