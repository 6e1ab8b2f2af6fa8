"""CPU-only checks of K12's definition (tests/jpeg_ref.py, the NumPy integer restatement of include/vaa.h) against a real codec of the libjpeg
family, recorded in tests/golden/jpeg_pillow.npz (tools/gen_jpeg_golden.py: Pillow 12.2 / libjpeg-turbo 3.1), and of the host logic around it.

Measured distance of the committed definition to the recorded codec: 0 bytes differ, on every fixture frame at every recorded quality (95, 75,
50, 100). The idealised real-arithmetic codec differs on 16-75 % of the bytes of the non-trivial frames (largest difference 3-38 levels)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import jpeg_ref
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_pillow.npz")
golden = jpeg_ref.golden


def test_fixture_holds_the_listed_frames_and_qualities():
    z = golden()["z"]
    assert sorted(int(q) for q in z["qualities"]) == [50, 75, 95, 100]
    shapes = sorted(tuple(z["in_" + str(n)].shape) for n in z["names"])
    for want in ((48, 64, 3), (24, 40, 3), (17, 33, 3), (16, 16, 3)):
        assert want in shapes
    assert shapes.count((48, 64, 3)) == 3 and len(shapes) == 8
    assert list(z["qt_q75"][0][:8]) == [8, 6, 5, 8, 12, 20, 26, 31]  # natural order
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_qtables_equal_the_recorded_codec_and_the_restatement():
    from roboticattack_amd import ops

    z = golden()["z"]
    for q in z["qualities"]:
        got = ops.jpeg_qtables(int(q))
        assert got.dtype == np.uint16 and got.shape == (2, 64)
        assert np.array_equal(got, z["qt_q%d" % q]) and np.array_equal(got, jpeg_ref.qtables(int(q)))
    for q in range(1, 101):
        t = ops.jpeg_qtables(q)
        assert np.array_equal(t, jpeg_ref.qtables(q)) and t.min() >= 1 and t.max() <= 255
    assert ops.jpeg_qtables(100).max() == 1 and ops.jpeg_qtables(1).min() == 255
    for bad in (0, 101, -5, 95.0, "95", True, None):
        with pytest.raises(ValueError):
            ops.jpeg_qtables(bad)


def test_qtables_equal_live_pillow():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_jpeg_golden
    finally:
        sys.path.pop(0)
    from roboticattack_amd import ops

    frame = np.zeros((16, 16, 3), np.uint8)
    for q in (1, 10, 50, 75, 95, 100):
        assert np.array_equal(ops.jpeg_qtables(q), gen_jpeg_golden.pillow_roundtrip(frame, q)[1]), q


def test_definition_is_no_further_from_the_codec_than_real_arithmetic():
    """For every fixture frame and quality: share of differing bytes, share differing by more than 1, largest difference — jpeg_ref against
    the recorded codec must not lose to the idealised codec on any of them; and every statistic measured as 0 is pinned at equality."""
    g = golden()
    z = g["z"]
    for n, q in g["cases"]:
        want = z["out_%s_q%d" % (n, q)]
        mine = jpeg_ref.stats(g["ref"][(n, q)], want)
        ideal = jpeg_ref.stats(jpeg_ref.ideal_roundtrip(z["in_" + n], z["qt_q%d" % q]), want)
        print("%-9s q=%3d  jpeg_ref %s   idealised (%.4f, %.4f, %d)" % (n, q, mine, *ideal))
        for a, b in zip(mine, ideal):
            assert a <= b, (n, q, mine, ideal)
        # measured: (0, 0, 0) in all 32 cases — pinned
        assert mine == (0.0, 0.0, 0) and np.array_equal(g["ref"][(n, q)], want), (n, q, mine)


@pytest.mark.parametrize("perturb", ["bias", "swap_tables", "truncate", "nearest"])
def test_comparison_sees_each_step(perturb):
    g = golden()
    z = g["z"]
    moved = [(n, q) for n, q in g["cases"]
             if not np.array_equal(jpeg_ref.roundtrip(z["in_" + n], z["qt_q%d" % q], perturb=perturb), g["ref"][(n, q)])]
    assert moved, "no fixture frame notices a wrong %s" % perturb


def test_rot180_encodes_the_flipped_frame():
    z = golden()["z"]
    f, qt = z["in_odd17x33"], z["qt_q95"]
    assert np.array_equal(jpeg_ref.roundtrip(f, qt, rot180=True), jpeg_ref.roundtrip(np.ascontiguousarray(f[::-1, ::-1]), qt))
    assert not np.array_equal(jpeg_ref.roundtrip(f, qt, rot180=True), jpeg_ref.roundtrip(f, qt)[::-1, ::-1])  # odd sizes: the MCU grid moves


# ---------------------------------------------------------------- host logic
def test_library_sizes_and_refusals_without_a_launch():
    from roboticattack_amd import _lib, ops

    L = _lib.lib()
    assert L.vaa_jpeg_roundtrip_ws_bytes(1, 256, 256) == 2 * 128 * 128 and L.vaa_jpeg_roundtrip_ws_bytes(3, 17, 33) == 3 * 2 * 16 * 24
    assert L.vaa_jpeg_roundtrip_ws_bytes(0, 64, 64) == 0 and L.vaa_jpeg_roundtrip_ws_bytes(1, 7, 64) == 0 and L.vaa_jpeg_roundtrip_ws_bytes(1, 64, 2049) == 0
    qt = ops.jpeg_qtables(95)
    assert L.vaa_jpeg_roundtrip(None, 0, 64, 64, 0, None, None, None, None, 0, None) == 0
    assert L.vaa_jpeg_roundtrip(None, -1, 64, 64, 0, None, None, None, None, 0, None) == -1
    assert L.vaa_jpeg_roundtrip(None, 1, 64, 64, 0, qt.ctypes.data, None, None, None, 0, None) == -1 and b"null pointer" in L.vaa_last_error()
    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.jpeg_roundtrip(torch.zeros(1, 32, 32, 3, dtype=torch.uint8), qt)


def _lib_npz(tmp_path, shape=(2, 48, 64, 3), name="cam.npz"):
    p = str(tmp_path / name)
    np.savez(p, frames=np.zeros(shape, np.uint8))
    return p


def test_eval_patch_flags_and_refusals(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "VLAAttacker"))
    try:
        import eval_patch
    finally:
        sys.path.pop(0)
    cam = _lib_npz(tmp_path)
    nat = _lib_npz(tmp_path, (2, 224, 224, 3), "nat.npz")
    a = eval_patch.arg_parser(["--patch", "p.pt"])
    assert a.frame_jpeg is False and a.frame_jpeg_quality == 95 and a.frame_jpeg_compare is False
    a = eval_patch.arg_parser(["--patch", "p.pt", "--frames_file", cam, "--frame_resize", "lanczos3", "--frame_jpeg", "true"])
    assert a.frame_jpeg is True and a.frame_jpeg_quality == 95
    a = eval_patch.arg_parser(["--patch", "p.pt", "--frames_file", cam, "--frame_resize", "lanczos3", "--frame_jpeg", "true",
                               "--frame_jpeg_quality", "75", "--frame_jpeg_compare", "true"])
    assert a.frame_jpeg_quality == 75 and a.frame_jpeg_compare is True
    for argv in (["--frame_jpeg", "true"],                                                    # no file
                 ["--frames_file", nat, "--frame_jpeg", "true"],                              # no resize
                 ["--frame_resize", "lanczos3", "--frame_jpeg", "true"],
                 ["--frames_file", cam, "--frame_resize", "lanczos3", "--frame_jpeg_compare", "true"],  # nothing to compare
                 ["--frames_file", cam, "--frame_resize", "lanczos3", "--frame_jpeg", "true", "--frame_jpeg_quality", "0"],
                 ["--frames_file", cam, "--frame_resize", "lanczos3", "--frame_jpeg", "true", "--frame_jpeg_quality", "101"]):
        with pytest.raises(SystemExit):
            eval_patch.arg_parser(["--patch", "p.pt"] + argv)
    capsys.readouterr()


def test_evaluate_patch_refuses_jpeg_without_the_resize():
    from roboticattack_amd.attack.evaluate import evaluate_patch

    t = types.SimpleNamespace(device="cpu")
    fr = np.zeros((1, 224, 224, 3), np.uint8)
    ids = torch.zeros((1, 4), dtype=torch.int64)
    kw = dict(mean=None, std=None)
    for extra in (dict(jpeg_quality=95), dict(resize="lanczos3", jpeg_quality=0), dict(resize="lanczos3", jpeg_quality=95.0),
                  dict(resize="lanczos3", jpeg_compare=True)):
        with pytest.raises(ValueError, match="jpeg"):
            evaluate_patch(None, t, fr, ids, ids, torch.zeros(3, 8, 8), [], **extra, **kw)


def test_eval_frames_without_a_quality_makes_todays_calls(monkeypatch):
    from roboticattack_amd import ops
    from roboticattack_amd.transform import RandomPatchTransform

    calls = []
    monkeypatch.setattr(ops, "resize_frames", lambda fr, rot=False: calls.append(("k8", tuple(fr.shape), rot)) or fr)
    monkeypatch.setattr(ops, "jpeg_roundtrip", lambda fr, qt, rot=False: calls.append(("k12", tuple(fr.shape), rot, qt.copy())) or fr)
    t = RandomPatchTransform.__new__(RandomPatchTransform)
    t.device = torch.device("cpu")
    fr = np.zeros((2, 48, 64, 3), np.uint8)
    t.eval_frames(fr, True)
    t.eval_frames(fr, rot180=False, jpeg_quality=None)
    assert calls == [("k8", (2, 48, 64, 3), True), ("k8", (2, 48, 64, 3), False)]
    del calls[:]
    t.eval_frames(fr, True, jpeg_quality=95)
    assert [c[:3] for c in calls] == [("k12", (2, 48, 64, 3), True), ("k8", (2, 48, 64, 3), False)]  # rotate, encode, then resize unrotated
    assert np.array_equal(calls[0][3], ops.jpeg_qtables(95))
    with pytest.raises(ValueError):
        t.eval_frames(fr, True, jpeg_quality=0)
