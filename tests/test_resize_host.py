"""The camera-frame resize (K8) without a GPU: the tap tables of roboticattack_amd.resize against the header's rule restated in resize_ref,
the fp32 restatement against the fp64 reference on every input the GPU test uses, a perturbation self-test of that comparison, the
frames-file loader and the new flags of the eval_patch parser, and the argument guards of vaa_frame_resize (no kernel is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import resize_ref
from conftest import ROOT
from roboticattack_amd import _lib, resize

SIZES = (256, 480, 640, 128, 224)
TAPS = {256: 9, 480: 15, 640: 19, 128: 7, 224: 7}


@pytest.mark.parametrize("n_in", SIZES + (8, 250, 302, 1030, 2048))
def test_tap_tables_follow_the_rule(n_in):
    start, w = resize.lanczos3_taps(n_in)
    T = w.shape[1]
    assert start.dtype == np.int32 and w.dtype == np.float32 and start.shape == (224,) and w.shape == (224, T)
    assert T == resize_ref.tap_count(n_in) == 2 * int(np.ceil(3.0 * max(n_in / 224.0, 1.0))) + 1 <= _lib.FRAME_RESIZE_MAX_TAPS
    if n_in in TAPS:
        assert T == TAPS[n_in]
    # each row of fp32 weights sums to 1 within one fp32 ulp of 1 (the sum of at most 57 fp32 numbers is exact in fp64)
    sums = w.astype(np.float64).sum(1)
    assert np.abs(sums - 1.0).max() <= np.finfo(np.float32).eps
    assert start.min() >= 0 and int(start.max()) + T - 1 <= n_in - 1
    for i in range(224):
        lo, hi = resize_ref.span(n_in, i)
        assert 1 <= hi - lo + 1 <= T
        assert start[i] == max(min(lo, n_in - T), 0)
        nz = np.flatnonzero(w[i])
        assert start[i] + nz.min() >= lo and start[i] + nz.max() <= hi  # nothing outside the rule's span
    # the restatement's tables, bit for bit (the byte-for-byte GPU comparison rests on them)
    rs, rw = resize_ref.taps_f32(n_in)
    assert np.array_equal(start, rs) and np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    assert resize.tap_count(n_in) == T


def test_taps_at_224_are_the_identity():
    start, w = resize.lanczos3_taps(224)
    assert w.shape == (224, 7)
    for i in range(224):
        c = i - int(start[i])
        assert w[i, c] == np.float32(1.0)  # exactly
        rest = np.delete(w[i], c)
        assert np.abs(rest).max() < 2.0 ** -50  # sin(k*pi) in fp64 is not exactly 0; 255 of these cannot move a byte
    B, H, W, seed = resize_ref.CASES["identity"]
    fr = resize_ref.frames(B, H, W, seed)
    assert np.array_equal(resize_ref.resize_f32(fr), fr)
    assert np.array_equal(resize_ref.resize_f32(fr, rot180=True), fr[:, ::-1, ::-1])
    assert fr.min() == 0 and fr.max() == 255


def test_bad_axis_lengths_are_refused():
    for n in (7, 2049, 0):
        with pytest.raises(ValueError):
            resize.lanczos3_taps(n)


_F64 = {}


def _case(name):
    """(frames, fp32 restatement, fp64 values) of a GPU test case, computed once per process and left unchanged."""
    if name not in _F64:
        B, H, W, seed = resize_ref.CASES[name]
        fr = resize_ref.frames(B, H, W, seed)
        _F64[name] = (fr, resize_ref.resize_f32(fr), resize_ref.resize_f64(fr))
    return _F64[name]


@pytest.mark.parametrize("name", sorted(resize_ref.CASES))
def test_fp32_restatement_equals_the_fp64_reference_outside_the_tie_band(name):
    fr, r32, v64 = _case(name)
    assert fr.min() == 0 and fr.max() == 255  # the inputs span the byte range
    bad, excluded = resize_ref.compare_f64(r32, v64)
    print(f"{name}: {bad} mismatches outside the tie band, {excluded:.5f} of the pixels excluded")
    assert excluded <= resize_ref.MAX_EXCLUDED
    assert bad == 0
    if name == "libero":  # the rotated input of the GPU test's rot180 case
        r32r, v64r = resize_ref.resize_f32(fr, rot180=True), resize_ref.resize_f64(fr, rot180=True)
        bad, excluded = resize_ref.compare_f64(r32r, v64r)
        assert bad == 0 and excluded <= resize_ref.MAX_EXCLUDED
        assert not np.array_equal(r32r, r32)


def test_the_comparison_detects_a_shifted_start_and_a_swapped_pass_order():
    fr, r32, v64 = _case("bridge")
    sx, wx = resize_ref.taps_f32(fr.shape[2])
    sy, wy = resize_ref.taps_f32(fr.shape[1])
    for axis in (0, 1):
        shifted = (np.minimum(sx + 1, fr.shape[2] - wx.shape[1]).astype(np.int32), wx, sy, wy) if axis == 0 else \
            (sx, wx, np.minimum(sy + 1, fr.shape[1] - wy.shape[1]).astype(np.int32), wy)
        got = resize_ref.resize_f32(fr, tables=shifted)
        assert not np.array_equal(got, r32)                      # the byte-for-byte comparison sees it
        assert resize_ref.compare_f64(got, v64)[0] > 1000        # and so does the fp64 one, massively
    swapped = resize_ref.resize_f32(fr, order="vh")              # same taps, the vertical pass first: only the roundings differ
    diff = int((swapped != r32).sum())
    print(f"vertical-first differs from horizontal-first in {diff} of {r32.size} bytes")
    assert diff > 0                                              # byte for byte tells the two orders apart
    assert resize_ref.compare_f64(swapped, v64)[0] == 0          # while both are correct roundings outside the tie band


# ---- the frames-file loader and the parser ----
def _eval_patch():
    sys.path.insert(0, os.path.join(ROOT, "VLAAttacker"))
    try:
        import eval_patch
    finally:
        sys.path.pop(0)
    return eval_patch


def test_frames_file_loader(tmp_path):
    from roboticattack_amd import cli

    fr = resize_ref.frames(3, 40, 56, 1)
    ids = np.arange(15, dtype=np.int64).reshape(3, 5)
    np.savez(tmp_path / "a.npz", frames=fr)
    np.savez(tmp_path / "b.npz", frames=fr, input_ids=ids, attention_mask=(ids > 0).astype(np.int64))
    f, i, m = cli.load_frames_file(str(tmp_path / "a.npz"))
    assert np.array_equal(f, fr) and f.dtype == np.uint8 and i is None and m is None
    f, i, m = cli.load_frames_file(str(tmp_path / "b.npz"))
    assert np.array_equal(f, fr) and i.dtype == torch.int64 and torch.equal(i, torch.from_numpy(ids)) and tuple(m.shape) == (3, 5)
    np.savez(tmp_path / "c.npz", frames=fr.astype(np.float32))
    np.savez(tmp_path / "d.npz", frames=fr, input_ids=ids)
    np.savez(tmp_path / "e.npz", frames=fr, input_ids=ids[:2], attention_mask=ids[:2])
    np.savez(tmp_path / "f.npz", images=fr)
    for bad in "cdef":
        with pytest.raises(ValueError):
            cli.load_frames_file(str(tmp_path / f"{bad}.npz"))


def test_eval_patch_parser_takes_the_frame_flags(tmp_path, capsys):
    eval_patch = _eval_patch()
    a = eval_patch.arg_parser(["--patch", "p.pt"])  # the defaults are unchanged
    assert a.frames_file is None and a.frame_resize is None and a.rotate180 is False and a.frames_data is None
    assert a.frames == 16 and a.center_crop is True and a.load_in_4bit is False
    np.savez(tmp_path / "libero.npz", frames=resize_ref.frames(2, 256, 256, 2))
    np.savez(tmp_path / "native.npz", frames=resize_ref.frames(2, 224, 224, 3))
    np.savez(tmp_path / "tiny.npz", frames=resize_ref.frames(2, 6, 224, 3))
    lib, nat = str(tmp_path / "libero.npz"), str(tmp_path / "native.npz")
    a = eval_patch.arg_parser(["--patch", "p.pt", "--frames_file", lib, "--frame_resize", "lanczos3", "--rotate180", "true", "--center_crop", "true"])
    assert a.frame_resize == "lanczos3" and a.rotate180 is True and a.frames_data[0].shape == (2, 256, 256, 3) and a.frames_data[1] is None
    a = eval_patch.arg_parser(["--patch", "p.pt", "--frames_file", nat])  # 224x224 frames need no resize
    assert a.frame_resize is None and a.frames_data[0].shape == (2, 224, 224, 3)
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--frames_file", lib])
    err = capsys.readouterr().err
    assert "--frame_resize" in err and "256x256" in err
    for argv in (["--frames_file", nat, "--rotate180", "true"], ["--frame_resize", "lanczos3"], ["--rotate180", "true"],
                 ["--frames_file", lib, "--frame_resize", "bicubic"], ["--frames_file", str(tmp_path / "absent.npz")],
                 ["--frames_file", str(tmp_path / "tiny.npz"), "--frame_resize", "lanczos3"]):
        with pytest.raises(SystemExit):
            eval_patch.arg_parser(["--patch", "p.pt"] + argv)


def test_evaluate_patch_refuses_unknown_resize_before_touching_the_device():
    from roboticattack_amd.attack.evaluate import evaluate_patch

    for kw in (dict(resize="bilinear"), dict(rot180=True)):
        with pytest.raises(ValueError):
            evaluate_patch(None, None, None, None, None, None, [], mean=None, std=None, **kw)


# ---- the C-ABI's argument checks ----
def test_entry_point_guards_without_gpu():
    """Every refusal is answered before any launch (host buffers stand in for the device operands; nothing dereferences them)."""
    L = _lib.lib()
    raw = (ctypes.c_uint8 * 4096)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    p = lambda off=0: ctypes.c_void_p(base + off)
    H, W = 32, 40
    sx, wx, sy, wy = (np.ascontiguousarray(t) for t in resize.frame_taps(H, W))
    Tx, Ty = wx.shape[1], wy.shape[1]
    assert (Tx, Ty) == (7, 7)
    assert L.vaa_frame_resize_taps_bytes(Tx, Ty) == 224 * (2 + Tx + Ty) * 4 == resize.pack_taps(sx, wx, sy, wy).nbytes
    assert L.vaa_frame_resize_taps_bytes(0, 7) == 0 and L.vaa_frame_resize_taps_bytes(7, 58) == 0 and L.vaa_frame_resize_taps_bytes(57, 57) == 224 * 116 * 4

    def call(src=p(0), B=1, H=H, W=W, rot=0, sx=sx, wx=wx, Tx=Tx, sy=sy, wy=wy, Ty=Ty, taps=p(1024), dst=p(2048)):
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.vaa_frame_resize(src, B, H, W, rot, ptr(sx), ptr(wx), Tx, ptr(sy), ptr(wy), Ty, taps, dst, None)

    assert call(B=0) == 0 and call(B=0, src=None, dst=None, taps=None, sx=None) == 0  # nothing to do, nothing validated
    assert call(B=-1) == -1
    for kw in (dict(src=None), dict(dst=None), dict(taps=None), dict(sx=None), dict(wx=None), dict(sy=None), dict(wy=None)):
        assert call(**kw) == -1 and b"null pointer" in L.vaa_last_error()
    assert call(rot=2) == -1 and call(Tx=0) == -1 and call(Ty=-3) == -1
    for kw in (dict(H=7), dict(W=7), dict(H=2049), dict(W=2049)):
        assert call(**kw) == -2 and b"outside [8, 2048]" in L.vaa_last_error()
    big = np.zeros((224, 58), np.float32)
    assert call(wx=big, Tx=58) == -2 and call(wy=big, Ty=58) == -2 and b"more than 57 taps" in L.vaa_last_error()
    for kw in (dict(src=p(2)), dict(taps=p(1026)), dict(dst=p(2056)), dict(dst=p(2052))):
        assert call(**kw) == -2 and b"aligned" in L.vaa_last_error()
    # the tables: a start whose window leaves the axis, at either end and on either axis; a weight that is not finite
    for axis, n in (("x", W), ("y", H)):
        for i, v in ((0, -1), (223, n - 7 + 1), (100, n)):
            s = (sx if axis == "x" else sy).copy()
            s[i] = v
            assert call(**{"s" + axis: s}) == -1 and (b"start_" + axis.encode()) in L.vaa_last_error()
        w = (wx if axis == "x" else wy).copy()
        w[17, 3] = np.nan
        assert call(**{"w" + axis: w}) == -1 and b"not finite" in L.vaa_last_error()
    assert call(H=8, W=W) == -1  # tables made for H = 32 do not fit an axis of 8 (start_y + 6 > 7)
    with pytest.raises(_lib.VaaError):
        _lib.check(-2, "vaa_frame_resize")
    from roboticattack_amd import ops

    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.resize_frames(torch.zeros(1, 32, 40, 3, dtype=torch.uint8))
    with pytest.raises(_lib.VaaError):
        ops.resize_frames(torch.zeros(1, 32, 40, dtype=torch.uint8))
