"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol include/vaa.h declares."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from roboticattack_amd import _lib


def _declared(header="vaa.h"):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(vaa_[a-z0-9_]+)\s*\(", hdr)))


def test_header_and_binding_agree():
    assert _declared() == sorted(_lib.EXPORTS)
    assert _declared("vaa_model_ops.h") == sorted(_lib.MODEL_OP_EXPORTS)  # the optional model-side operators


def test_library_exports_every_declared_symbol():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared() + _declared("vaa_model_ops.h"):
        assert hasattr(L, name), f"libvaa_hip.so does not export {name}"
    assert _lib.lib().vaa_version() >= 100


def test_sizes_and_argument_errors_without_gpu():
    """Pure host-side entry points and argument validation (no kernel is launched)."""
    L = _lib.lib()
    assert L.vaa_patch_grad_ws_bytes(64, 50, 50) == 64 * 3 * 50 * 50 * 4  # one partial tile per image (its row bands are separate workgroups)
    assert L.vaa_patch_grad_ws_bytes(4096, 50, 50) == 512 * 3 * 50 * 50 * 4
    assert L.vaa_patch_grad_ws_bytes(0, 50, 50) == 0
    # the larger of the label-driven schedule's per-position statistics (36 B) and the ROWS route (row map 16 + 16 B/position, rounded to
    # 256 B, + 4 part statistics and one slice statistic per row)
    assert L.vaa_loss_ws_bytes(64, 45) == max(64 * 44 * 36, (16 + 64 * 44 * 16 + 255) // 256 * 256 + 64 * 44 * (4 * 16 + 16))
    assert L.vaa_loss_rowmap_bytes(64, 45) == 16 + 64 * 44 * 16 and L.vaa_loss_rows_ws_bytes(128) == 128 * 80
    assert L.vaa_patch_resize_ws_bytes(4, 100, 100) == 4 * 3 * 100 * 100 * 4 and L.vaa_patch_resize_ws_bytes(1, 100, 100) == 0  # one partial per image group; a single group writes gpatch itself
    # K2': packed weights = 37 column blocks x 16 columns (588 + 4 of padding) x D; towers must be multiples of 64 wide
    assert L.vaa_patch_embed_packed_elems(1024) == 592 * 1024 and L.vaa_patch_embed_packed_elems(96) == 0 and L.vaa_patch_embed_packed_elems(0) == 0
    assert L.vaa_patch_embed_pack_weights(None, 1024, None, None) == -1 and b"null pointer" in L.vaa_last_error()
    assert L.vaa_patch_embed_grad_ws_bytes(64, 50, 50) == L.vaa_patch_grad_ws_bytes(64, 50, 50) + 2 * 64 * 256 * 588 * 4 + 256  # partials + a tile-gradient buffer per tower
    assert L.vaa_patch_embed_grad_multi_ws_bytes(4) == 2 * 4 * 256 * 588 * 4 + 256
    # K3s: shapes it covers and its scratch (two logits + the launch tag per 64-bit word, whole row blocks)
    assert L.vaa_head_slice_applies(128, 4096, 32064) == 1 and L.vaa_head_slice_applies(129, 4096, 32064) == 0 and L.vaa_head_slice_applies(16, 4160, 32064) == 0
    assert L.vaa_head_slice_applies(16, 64, 32064) == 1 and L.vaa_head_slice_applies(16, 64, 40000) == 0 and L.vaa_head_slice_applies(0, 64, 32064) == 0
    assert L.vaa_head_slice_ws_bytes(1) == 16 * 1024 and L.vaa_head_slice_ws_bytes(128) == 128 * 1024 and L.vaa_head_slice_ws_bytes(0) == 0
    assert L.vaa_head_slice_pack(None, 4096, 32064, None, None) == -1 and b"null pointer" in L.vaa_last_error()
    assert L.vaa_head_slice_fwd_bwd(None, None, None, 4096, None, 16, 8, 30, 32064, 1, _lib.f32x([5, .8, .2, 1]), None, None, None, 0, None, None, None, None, 0, None) == -1
    # empty batches return before anything is validated or launched
    assert L.vaa_patch_embed_grad_gather_multi(None, 64, None, 64, None, None, None, None, None, None, None, 0, 50, 50, 1, 0, _lib.f32x([1] * 6), 1, None, None, 0, None) == 0
    assert L.vaa_patch_grad_gather_multi(None, None, None, None, None, None, 0, 50, 50, 1, 0, _lib.f32x([1] * 6), None, None) == 0
    assert L.vaa_patch_embed_grad_gather_multi(None, 64, None, 64, None, None, None, None, None, None, None, 2, 50, 50, 1, 0, _lib.f32x([1] * 6), 1, None, None, 0, None) == -1
    rc = L.vaa_patch_apply_fwd(None, None, None, None, 1, 50, 50, 1, 0, _lib.f32x([0] * 6), _lib.f32x([1] * 6), None, None, None)
    assert rc == -1 and b"null pointer" in L.vaa_last_error()
    rc = L.vaa_patch_update(None, None, None, None, 10, 0, 1e-3, 0.9, 0.999, 1e-6, 1, 0.0, 1.0, None, None)
    assert rc == -1
    with pytest.raises(_lib.VaaError):
        _lib.check(rc, "vaa_patch_update")


def test_attention_range_and_scale_guards_without_gpu():
    """vaa_model_attention_{fwd,bwd} refuse, before any launch, a (batch, head) slice beyond the kernels' 32-bit addressing and a softmax scale
    that is not finite and > 0. Small host buffers stand in for the operands (nothing dereferences them); skipped where a GPU is visible, so it
    can never launch anything."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("host-side guards only: must not be able to launch")
    L = _lib.lib()
    buf = [(ctypes.c_uint16 * 64)() for _ in range(8)]
    f32 = [(ctypes.c_float * 64)() for _ in range(2)]
    p = lambda b: ctypes.cast(b, ctypes.c_void_p)
    s3 = lambda t: (ctypes.c_int64 * 3)(0, t, 64)
    ok = s3(64)

    def fwd(T, strs, scale):
        return L.vaa_model_attention_fwd(p(buf[0]), strs[0], p(buf[1]), strs[1], p(buf[2]), strs[2], p(buf[3]), strs[3], p(f32[0]), None, 1, 1, T, 64, 1,
                                         scale, None)

    def bwd(T, strs, scale):
        return L.vaa_model_attention_bwd(p(buf[0]), strs[0], p(buf[1]), strs[1], p(buf[2]), strs[2], p(buf[3]), strs[3], p(buf[4]), strs[4], p(f32[0]),
                                         p(f32[1]), p(buf[5]), strs[5], p(buf[6]), strs[6], p(buf[7]), strs[7], None, None, None, 1, 1, T, 64, 1, scale,
                                         None)

    for call, n in ((fwd, 4), (bwd, 8)):
        for i in range(n):  # any one operand out of range
            # the descriptor's byte count ((T-1)*stride + hd)*2 > 2^31-1
            assert call(2, [s3(2 ** 30) if j == i else ok for j in range(n)], 0.125) == -2 and b"32-bit" in L.vaa_last_error()
            # the byte count fits (2^30 + 2^24 + 128) but the last tile row's offset (127 rows at T = 65) does not
            assert call(65, [s3(2 ** 23 + 2 ** 17) if j == i else ok for j in range(n)], 0.125) == -2 and b"32-bit" in L.vaa_last_error()
            assert call(2, [s3(-64) if j == i else ok for j in range(n)], 0.125) == -2 and b"32-bit" in L.vaa_last_error()
        for scale in (0.0, -0.125, float("nan"), float("inf")):
            assert call(2, [ok] * n, scale) == -2 and b"scale must be finite and > 0" in L.vaa_last_error()


def test_ops_refuse_cpu_tensors():
    import torch

    from roboticattack_amd import ops

    with pytest.raises(_lib.VaaError, match="no CPU fallback"):
        ops.patch_apply_fwd(torch.zeros(1, 224, 224, 3, dtype=torch.uint8), torch.zeros(3, 50, 50), torch.zeros(1, 2, dtype=torch.int32),
                            torch.zeros(1, 6), True)


def test_missing_library_fails_loudly(tmp_path):
    """No HIP extension -> the product path raises (there is no CPU fallback to drop into)."""
    import subprocess
    import sys

    code = ("import os; os.environ['VAA_LIB_PATH'] = %r\n"
            "from roboticattack_amd import _lib\n"
            "try:\n    _lib.lib()\nexcept _lib.VaaError as e:\n    print('RAISED', e)\n") % str(tmp_path / "absent.so")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert "RAISED" in out.stdout and "no CPU fallback" in out.stdout, out.stdout + out.stderr
