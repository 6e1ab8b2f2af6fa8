"""PyTorch-ROCm front end of the C-ABI (include/vaa.h): device memory, streams and autograd plumbing only.

Every function here enqueues hand-written HIP kernels from libvaa_hip.so on torch's current stream and
returns without synchronising. No function has a CPU path; tensors must live on a ROCm device.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import (  # noqa: F401  (re-exported)
    GRAD_FULL,
    GRAD_SLICE,
    LAYOUT_FULL,
    LAYOUT_ROWS,
    LOSS_CE,
    LOSS_UADA,
    LOSS_UADA_DDP,
    LOSS_UPA,
    MASK_LT_M20,
    MASK_NE_M100,
    OPT_ADAMW_HF,
    OPT_PGD_SIGN,
    SEG_UPA_MAX_GROUPS,
)
from .constants import IMG, MEAN6, STD6

_MEAN = _lib.f32x(MEAN6)
_STD = _lib.f32x(STD6)
_ws_cache: dict = {}

# Optional kernel timing (bench.py): when TIMER is a list, every hand-written kernel launch sequence is bracketed by
# torch.cuda.Event pairs recorded on the launching (= torch current) stream; entries are (name, start, end, info).
TIMER = None


class _timed:
    def __init__(self, name, **info):
        self.name, self.info = name, info

    def __enter__(self):
        if TIMER is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if TIMER is not None:
            self.e.record()
            TIMER.append((self.name, self.s, self.e, self.info))
        return False


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, dtype, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.VaaError(f"{name}: expected a tensor on a ROCm device (there is no CPU fallback)")
    if t.dtype != dtype:
        raise _lib.VaaError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.VaaError(f"{name}: expected a contiguous tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.VaaError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _workspace(device, nbytes: int, kind: str = "k2") -> torch.Tensor:
    """Scratch for one operator KIND on the current stream: K2's partial tiles, K3's row statistics and the resize adjoint each have
    their own buffer per (device, stream), so a caller that overlaps them on different streams never shares scratch (vaa.h: the
    library is re-entrant per stream, the workspace is the caller's)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream, kind)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def prof_start(capacity: int = 4096) -> None:
    """Arm the library's per-dispatch timer (vaa_prof_start): every kernel it launches from now on carries its own start/stop events."""
    _lib.check(_lib.lib().vaa_prof_start(int(capacity)), "vaa_prof_start")


def prof_collect() -> list:
    """Disarm and return [(kernel name, microseconds)] in launch order (waits for the recorded dispatches)."""
    import ctypes as C

    L = _lib.lib()
    n = L.vaa_prof_stop()
    out = []
    name, us = C.c_char_p(), C.c_float()
    for i in range(n):
        _lib.check(L.vaa_prof_get(i, C.byref(name), C.byref(us)), "vaa_prof_get")
        out.append((name.value.decode(), float(us.value)))
    return out


def device_check() -> None:
    _lib.check(_lib.lib().vaa_device_check(), "vaa_device_check")


def async_error_check() -> None:
    """Raises VaaError when a kernel of this process recorded a device-side failure since the last poll (include/vaa.h: vaa_async_error).
    Call it behind a synchronisation point — the word is written by the kernel that failed."""
    _lib.check(_lib.lib().vaa_async_error(), "vaa_async_error")


# ------------------------------------------------------------------------------------------------------
# K1 / K2 / K2': one body per kernel family (_k1, _k2, _k2e); the public wrappers below name the variant
# ------------------------------------------------------------------------------------------------------
def _ptr(t):
    return t.data_ptr() if t is not None else None


def _placement(B: int, patch, xy, theta, geometry: bool, pdesc, max_hw):
    """The arguments every K1 / K2 / K2' call shares, checked once: the patch (or, with pdesc / max_hw, the packed per-image patches and their
    bounds), where it lands (xy) and how it is warped (theta). Returns the C arguments (patch, [pdesc,] xy, theta) and (ph, pw)."""
    _need(patch, torch.float32, "patch")
    _need(xy, torch.int32, "xy", (B, 2))
    if geometry:
        _need(theta, torch.float32, "theta", (B, 6))
    if pdesc is None:
        return (patch.data_ptr(), xy.data_ptr(), theta.data_ptr() if geometry else None), (int(patch.shape[1]), int(patch.shape[2]))
    _need(pdesc, torch.int32, "pdesc", (B, 4))
    return (patch.data_ptr(), pdesc.data_ptr(), xy.data_ptr(), theta.data_ptr() if geometry else None), (int(max_hw[0]), int(max_hw[1]))


def _partials_view(ws, B: int, ph: int, pw: int):
    """The partial tiles [parts, 3*ph*pw] a deferred K2 / K2' left at the front of its workspace, for ops.step_epilogue to add."""
    parts, n = _lib.lib().vaa_patch_grad_partials(B), 3 * ph * pw
    return ws[: parts * n * 4].view(torch.float32).view(parts, n)


def _k1(img_u8, patch, xy, theta, geometry, mask_mode, mean6, std6, pdesc=None, max_hw=None, tiles=False, want_keep=True):
    """K1 in every form. Planar: -> (bf16 [B,6,224,224], keep bits or None); tiles: -> (out0, out1, keep_tiles, tile_flags)."""
    B = img_u8.shape[0]
    _need(img_u8, torch.uint8, "img_u8", (B, IMG, IMG, 3))
    place, (ph, pw) = _placement(B, patch, xy, theta, geometry, pdesc, max_hw)
    dev = img_u8.device
    if tiles:
        name = "patch_apply_fwd_tiles"
        outs = (torch.empty((B, 256, 588), dtype=torch.bfloat16, device=dev), torch.empty((B, 256, 588), dtype=torch.bfloat16, device=dev),
                torch.empty((B, 3, 256, 14), dtype=torch.int16, device=dev), torch.empty((B, 256), dtype=torch.int32, device=dev))
        if pdesc is None:  # this entry point takes the descriptor in both cases
            place = (place[0], None) + place[1:]
    else:
        name = "patch_apply_fwd" if pdesc is None else "patch_apply_fwd_multi"
        outs = (torch.empty((B, 6, IMG, IMG), dtype=torch.bfloat16, device=dev),
                torch.empty((B, 3, IMG * IMG // 8), dtype=torch.uint8, device=dev) if want_keep else None)
    mean_c = _MEAN if mean6 is None else _lib.f32x(mean6)
    std_c = _STD if std6 is None else _lib.f32x(std6)
    with _timed("K1_" + name, B=B, ph=ph, pw=pw):
        rc = getattr(_lib.lib(), "vaa_" + name)(img_u8.data_ptr(), *place, B, ph, pw, int(bool(geometry)), int(mask_mode), mean_c, std_c,
                                                *map(_ptr, outs), _stream())
    _lib.check(rc, "vaa_" + name)
    return outs


def _grad_call(name, kind, B, lead, patch, xy, theta, mask, geometry, mask_mode, std6, tail, pdesc, max_hw, defer_reduce):
    """What K2 and K2' share behind their own leading (`lead`: the incoming gradient) and trailing (`tail`) arguments: the placement, the keep
    mask (`mask`: tensors as the entry point takes them), the output and the workspace. One patch: -> dL/d patch [3,ph,pw], or with defer_reduce
    the partial tiles (_partials_view). pdesc / max_hw: -> the gradient of every image's own patch, in the layout of the packed `patch`."""
    place, (ph, pw) = _placement(B, patch, xy, theta, geometry, pdesc, max_hw)
    L = _lib.lib()
    ws = ()
    if pdesc is not None:  # (no partial tiles here: no wrapper offers defer_reduce with per-image patches)
        out = torch.zeros_like(patch)
        if kind == "k2e":
            ws = (_workspace(patch.device, L.vaa_patch_embed_grad_multi_ws_bytes(B), kind),)
    else:
        out = None if defer_reduce else torch.empty_like(patch)
        ws = (_workspace(patch.device, (L.vaa_patch_grad_ws_bytes if kind == "k2" else L.vaa_patch_embed_grad_ws_bytes)(B, ph, pw), kind),)
    std_c = _STD if std6 is None else _lib.f32x(std6)
    with _timed("K2_" + name, B=B, ph=ph, pw=pw):
        rc = getattr(L, "vaa_" + name)(*lead, *place, *map(_ptr, mask), B, ph, pw, int(bool(geometry)), int(mask_mode), std_c, *tail, _ptr(out),
                                       *(a for w in ws for a in (w.data_ptr(), w.numel())), _stream())
    _lib.check(rc, "vaa_" + name)
    return _partials_view(ws[0], B, ph, pw) if defer_reduce else out


def _k2(gout_bf16, patch, xy, theta, keep_bits, geometry, mask_mode, std6, pdesc=None, max_hw=None, defer_reduce=False):
    """K2 in every form: the model's bf16 pixel gradient [B,6,224,224] -> the patch gradient (_grad_call). keep_bits=None: the mask is re-derived."""
    B = gout_bf16.shape[0]
    _need(gout_bf16, torch.bfloat16, "gout_bf16", (B, 6, IMG, IMG))
    if keep_bits is not None:
        _need(keep_bits, torch.uint8, "keep_bits", (B, 3, IMG * IMG // 8))
    name = "patch_grad_gather" if pdesc is None else "patch_grad_gather_multi"
    return _grad_call(name, "k2", B, (gout_bf16.data_ptr(),), patch, xy, theta, (keep_bits,), geometry, mask_mode, std6, (), pdesc, max_hw, defer_reduce)


def _k2e(dy0, dy1, wp0, wp1, patch, xy, theta, keep, tile_flags, geometry, mask_mode, std6, round_bf16, pdesc=None, max_hw=None, defer_reduce=False):
    """K2' in every form: the gradients of the two patch-embed outputs -> the patch gradient (_grad_call). The keep mask is K1's: keep bits
    (tile_flags=None), or the tile-major keep words with their tile flags."""
    B = dy0.shape[0]
    D0, D1 = int(dy0.shape[2]), int(dy1.shape[2])
    _need(dy0, torch.bfloat16, "dy0", (B, 256, D0))
    _need(dy1, torch.bfloat16, "dy1", (B, 256, D1))
    _need(wp0, torch.bfloat16, "wp0", (592 * D0,))
    _need(wp1, torch.bfloat16, "wp1", (592 * D1,))
    if tile_flags is None:
        mask = (_need(keep, torch.uint8, "keep_bits", (B, 3, IMG * IMG // 8)),)
    else:
        mask = (_need(keep, torch.int16, "keep_tiles", (B, 3, 256, 14)), _need(tile_flags, torch.int32, "tile_flags", (B, 256)))
    name = "patch_embed_grad_gather" + ("" if pdesc is None else "_multi") + ("" if tile_flags is None else "_tiles")
    lead = (dy0.data_ptr(), D0, dy1.data_ptr(), D1, wp0.data_ptr(), wp1.data_ptr())
    return _grad_call(name, "k2e", B, lead, patch, xy, theta, mask, geometry, mask_mode, std6, (int(bool(round_bf16)),), pdesc, max_hw, defer_reduce)


def patch_apply_fwd(img_u8, patch, xy, theta, geometry: bool, mask_mode: int = MASK_LT_M20, want_keep: bool = True,
                    mean6=None, std6=None):
    """K1. img_u8 [B,224,224,3] u8, patch [3,ph,pw] f32, xy [B,2] i32, theta [B,6] f32 -> (bf16 [B,6,224,224], keep bits)."""
    return _k1(img_u8, patch, xy, theta, geometry, mask_mode, mean6, std6, want_keep=want_keep)


def patch_apply_fwd_tiles(img_u8, patch, xy, theta, geometry: bool, mask_mode: int = MASK_LT_M20, mean6=None, std6=None, pdesc=None, max_hw=None):
    """K1 in tile-major form (vaa_patch_apply_fwd_tiles): -> (out0, out1 bf16 [B,256,588], keep_tiles u16 [B,3,256,14], tile_flags u32 [B,256]).
    out_k are the operands of the two ViT patch-embed GEMMs (tile t = ty*16 + tx, element c*196 + y*14 + x). pdesc/max_hw: per-image patches."""
    return _k1(img_u8, patch, xy, theta, geometry, mask_mode, mean6, std6, pdesc, max_hw, tiles=True)


def patch_grad_gather(gout_bf16, patch, xy, theta, keep_bits, geometry: bool, mask_mode: int = MASK_LT_M20, std6=None, defer_reduce: bool = False):
    """K2. gout_bf16 [B,6,224,224] bf16 -> dL/d patch [3,ph,pw] f32 (sum over the batch). defer_reduce=True returns the partial tiles
    [parts, 3*ph*pw] (a view of the workspace) for ops.step_epilogue to add."""
    return _k2(gout_bf16, patch, xy, theta, keep_bits, geometry, mask_mode, std6, defer_reduce=defer_reduce)


def pack_embed_weights(wt):
    """Conv weights of one tower, flattened and transposed to wt [588,D] bf16, re-ordered into the MFMA fragment order K2' reads
    (vaa_patch_embed_pack_weights; once per model — the weights are frozen during an attack). Returns bf16 [592*D]."""
    D = int(wt.shape[1])
    _need(wt, torch.bfloat16, "wt", (588, D))
    L = _lib.lib()
    n = L.vaa_patch_embed_packed_elems(D)
    if n == 0:
        raise ValueError(f"pack_embed_weights: tower width {D} is not a multiple of 64")
    packed = torch.empty(n, dtype=torch.bfloat16, device=wt.device)
    _lib.check(L.vaa_patch_embed_pack_weights(wt.data_ptr(), D, packed.data_ptr(), _stream()), "vaa_patch_embed_pack_weights")
    return packed


def patch_embed_grad_gather(dy0, dy1, wp0, wp1, patch, xy, theta, keep_bits, geometry: bool, mask_mode: int = MASK_LT_M20, std6=None,
                            round_bf16: bool = True):
    """K2' (SURVEY.md 8f-3): dL/d patch from the gradients of the two ViT patch-embed OUTPUTS. dy0 [B,256,D0], dy1 [B,256,D1] bf16
    (tokens in tile order), wp0 / wp1 = pack_embed_weights(W^T [588,D]) of the two towers. Only tiles with kept pixels are
    evaluated (MFMA); the pixel gradient is never materialised."""
    return _k2e(dy0, dy1, wp0, wp1, patch, xy, theta, keep_bits, None, geometry, mask_mode, std6, round_bf16)


def patch_embed_grad_gather_tiles(dy0, dy1, wp0, wp1, patch, xy, theta, keep_tiles, tile_flags, geometry: bool, mask_mode: int = MASK_LT_M20,
                                  std6=None, round_bf16: bool = True, defer_reduce: bool = False):
    """K2' fed by the tile-major mask of patch_apply_fwd_tiles. defer_reduce=True returns (partials view [parts, 3*ph*pw] of the workspace):
    the fixed-order sum is then left to ops.step_epilogue."""
    return _k2e(dy0, dy1, wp0, wp1, patch, xy, theta, keep_tiles, tile_flags, geometry, mask_mode, std6, round_bf16, defer_reduce=defer_reduce)


def patch_embed_grad_gather_multi(dy0, dy1, wp0, wp1, packed, pdesc, max_hw, xy, theta, keep_bits, geometry: bool, mask_mode: int = MASK_LT_M20,
                                  std6=None, round_bf16: bool = True):
    """K2' with one patch per image (resize_patch=True): like patch_grad_gather_multi, fed by the patch-embed output gradients."""
    return _k2e(dy0, dy1, wp0, wp1, packed, xy, theta, keep_bits, None, geometry, mask_mode, std6, round_bf16, pdesc, max_hw)


def patch_embed_grad_gather_multi_tiles(dy0, dy1, wp0, wp1, packed, pdesc, max_hw, xy, theta, keep_tiles, tile_flags, geometry: bool,
                                        mask_mode: int = MASK_LT_M20, std6=None, round_bf16: bool = True):
    """K2' with one patch per image, fed by the tile-major mask of patch_apply_fwd_tiles(pdesc=...)."""
    return _k2e(dy0, dy1, wp0, wp1, packed, xy, theta, keep_tiles, tile_flags, geometry, mask_mode, std6, round_bf16, pdesc, max_hw)


# ------------------------------------------------------------------------------------------------------
# resize_patch=True (config 5): per-image patches
# ------------------------------------------------------------------------------------------------------
def make_pdesc(sizes, align: int = 4):
    """sizes [B,2] (h,w) host ints -> (pdesc int32 numpy [B,4] = {h, w, offset, 0}, packed length in floats)."""
    import numpy as np

    sizes = np.asarray(sizes, np.int32).reshape(-1, 2)
    pdesc = np.zeros((sizes.shape[0], 4), np.int32)
    off = 0
    for b, (h, w) in enumerate(sizes):
        if h <= 0 or w <= 0 or h > IMG or w > IMG:
            raise _lib.VaaError(f"resized patch {h}x{w} of image {b} does not fit the {IMG}x{IMG} frame")
        pdesc[b] = (h, w, off, 0)
        off += (3 * int(h) * int(w) + align - 1) // align * align
    return pdesc, off


def _patch_stage_call(fn: str, lead, hw, extra, pdesc, total=None, ws=None):
    """One entry point of a per-image patch stage (K0 resize, K0c jitter), in the C argument order all four share: the float32 `lead` tensors
    ((name, tensor), ...; the base patch last where there is one), its (ph, pw) = hw (None: the base patch's own), the stage's `extra` float32
    [B,3] tensors, pdesc [B,4], B, the output (total given: the zero-filled packed [total] of a forward; None: an adjoint's [3,ph,pw]), [the
    workspace of ws = the stage's word in its vaa_patch_<ws>_ws_bytes and its _workspace kind,] the stream."""
    for name, t in lead:
        _need(t, torch.float32, name)
    B = int(pdesc.shape[0])
    ph, pw = hw if hw is not None else (int(v) for v in lead[-1][1].shape[1:])
    _need(pdesc, torch.int32, "pdesc", (B, 4))
    for name, t in extra:
        _need(t, torch.float32, name, (B, 3))
    dev = lead[0][1].device
    out = torch.empty((3, ph, pw), dtype=torch.float32, device=dev) if total is None else torch.zeros(int(total), dtype=torch.float32, device=dev)
    L = _lib.lib()
    args = [t.data_ptr() for _, t in lead] + [ph, pw] + [t.data_ptr() for _, t in extra] + [pdesc.data_ptr(), B, out.data_ptr()]
    if ws is not None:
        buf = _workspace(dev, getattr(L, f"vaa_patch_{ws}_ws_bytes")(B, ph, pw), ws)
        args += [buf.data_ptr(), buf.numel()]
    with _timed("K0_" + fn[4:], B=B):
        rc = getattr(L, fn)(*args, _stream())
    _lib.check(rc, fn)
    return out


def patch_resize_fwd(patch, pdesc, total: int):
    """Base patch [3,ph,pw] f32 -> packed f32 [total]: image b's antialias-bilinear resized patch [3,h_b,w_b] at pdesc[b].offset."""
    return _patch_stage_call("vaa_patch_resize_fwd", (("patch", patch),), None, (), pdesc, total)


def patch_resize_bwd(gpacked, pdesc, ph: int, pw: int):
    """Adjoint of patch_resize_fwd summed over the images: gpacked f32 [total] -> d L / d base patch [3,ph,pw]."""
    return _patch_stage_call("vaa_patch_resize_bwd", (("gpacked", gpacked),), (ph, pw), (), pdesc, ws="resize")


def patch_jitter_fwd(patch, factors, pdesc, total: int):
    """colorjitter (K0c): base patch [3,ph,pw] f32, factors [B,3] f32 (brightness, contrast, saturation) -> packed f32 [total]: image b's
    jittered patch [3,ph,pw] at pdesc[b].offset (include/vaa.h states the arithmetic)."""
    return _patch_stage_call("vaa_patch_jitter_fwd", (("patch", patch),), None, (("factors", factors),), pdesc, total)


def patch_jitter_bwd(gpacked, patch, factors, pdesc):
    """Adjoint of patch_jitter_fwd summed over the images: gpacked f32 [total] -> d L / d base patch [3,ph,pw] (gates recomputed from `patch`)."""
    return _patch_stage_call("vaa_patch_jitter_bwd", (("gpacked", gpacked), ("patch", patch)), None, (("factors", factors),), pdesc, ws="jitter")


def patch_reg_grad(patch, palette, w_tv: float, w_nps: float, grad=None, accumulate: bool = False, part=None, want_grad: bool = True):
    """K6 (include/vaa.h states the arithmetic): the gradient r of w_tv*TV(patch) + w_nps*NPS(patch, palette) and the per-workgroup partial sums
    of the two values, ONE launch. patch [3,ph,pw] f32; palette [K,3] f32 (K <= 64), or None when w_nps == 0. `grad` None: a new tensor receives
    r; given: r is written to it, or with `accumulate` added to it in place (one rounded add of the same r). `want_grad=False`: values only.
    -> (grad | None, part f64 [parts,2]); TV / NPS are folded from `part` by patch_reg_values when somebody wants them."""
    _need(patch, torch.float32, "patch")
    if patch.dim() != 3 or int(patch.shape[0]) != 3:
        raise _lib.VaaError(f"patch: expected shape (3, ph, pw), got {tuple(patch.shape)}")
    ph, pw = int(patch.shape[1]), int(patch.shape[2])
    K = 0
    if palette is not None:
        K = int(palette.shape[0])
        _need(palette, torch.float32, "palette", (K, 3))
    L = _lib.lib()
    parts = int(L.vaa_patch_reg_parts(ph, pw))
    if part is None:
        part = torch.empty((parts, 2), dtype=torch.float64, device=patch.device)
    _need(part, torch.float64, "part", (parts, 2))
    if not want_grad:
        grad = None
    elif grad is None:
        grad, accumulate = torch.empty_like(patch), False
    else:
        _need(grad, torch.float32, "grad", tuple(patch.shape))
    with _timed("K6_patch_reg"):
        rc = L.vaa_patch_reg(patch.data_ptr(), ph, pw, _ptr(palette), K, float(w_tv), float(w_nps), _ptr(grad), int(bool(accumulate)), part.data_ptr(),
                             _stream())
    _lib.check(rc, "vaa_patch_reg")
    return grad, part


def patch_reg_values(part, n3: int):
    """(TV, NPS) as device fp64 scalars from K6's partial sums: part[:,0].sum()/n3, part[:,1].sum()/n3 (n3 = 3*ph*pw). Nothing is read back."""
    s = part.sum(dim=0) / float(n3)
    return s[0], s[1]


def patch_apply_fwd_multi(img_u8, packed, pdesc, max_hw, xy, theta, geometry: bool, mask_mode: int = MASK_LT_M20, want_keep: bool = True,
                          mean6=None, std6=None):
    """K1 with one patch per image (packed/pdesc from patch_resize_fwd or patch_jitter_fwd). max_hw = (max h, max w) over the batch (host ints)."""
    return _k1(img_u8, packed, xy, theta, geometry, mask_mode, mean6, std6, pdesc, max_hw, want_keep=want_keep)


def patch_grad_gather_multi(gout_bf16, packed, pdesc, max_hw, xy, theta, keep_bits, geometry: bool, mask_mode: int = MASK_LT_M20, std6=None):
    """K2 with one patch per image: returns gpacked (layout of `packed`): d L / d (every image's own patch)."""
    return _k2(gout_bf16, packed, xy, theta, keep_bits, geometry, mask_mode, std6, pdesc, max_hw)


# ------------------------------------------------------------------------------------------------------
# autograd: the seven Functions share one forward and one backward; each names its variant
# ------------------------------------------------------------------------------------------------------
class PatchEmbeds(tuple):
    """(e0, e1): the two ViT patch-embed outputs [B,256,D] of a patched batch, standing in for `pixel_values` on the path that
    keeps the pixel gradient un-materialised (PatchApplyEmbed). `OpenVLAShaped.forward_rows(..., patch_embeds=...)` consumes it."""


def unfold_tiles(x3: torch.Tensor) -> torch.Tensor:
    """[B,3,224,224] -> [B,256,588]: the 14x14 tiles of timm's PatchEmbed conv (kernel == stride), columns ordered (c, y, x)."""
    B = x3.shape[0]
    return x3.reshape(B, 3, 16, 14, 16, 14).permute(0, 2, 4, 1, 3, 5).reshape(B, 256, 588)


def sweep_pdesc(P: int, Bp: int, ph: int, pw: int, device) -> torch.Tensor:
    """[P*Bp, 4] int32 patch descriptors of a maskidx sweep: image b of group g = b // Bp pastes patch g of the packed [P,3,ph,pw] tensor."""
    g = torch.arange(P * Bp, dtype=torch.int32) // Bp
    d = torch.stack([torch.full_like(g, ph), torch.full_like(g, pw), g * (3 * ph * pw), torch.zeros_like(g)], dim=1)
    return d.contiguous().to(device, non_blocking=True)


def _stage_pack(stage: str, patch, rows):
    """The prologue of a per-image patch stage: the descriptor, its device copy and the stage's forward on the base patch -> (every image's own
    patch, packed; pdesc on the device; (max h, max w)). "resize" (K0): rows = host sizes [B,2] (h,w); "jitter" (K0c): rows = factors [B,3] on
    the device, every image's patch keeps the base size."""
    ph, pw = int(patch.shape[1]), int(patch.shape[2])
    pdesc_np, total = make_pdesc(rows if stage == "resize" else [(ph, pw)] * int(rows.shape[0]))
    pdesc = torch.from_numpy(pdesc_np).to(patch.device, non_blocking=True)
    if stage == "resize":
        return patch_resize_fwd(patch, pdesc, total), pdesc, (int(pdesc_np[:, 0].max()), int(pdesc_np[:, 1].max()))
    return patch_jitter_fwd(patch, rows, pdesc, total), pdesc, (ph, pw)


def _paste_forward(ctx, p, img_u8, xy, theta, geometry, mask_mode, mean6, std6, pdesc=None, max_hw=None, embed=None, sink=None, stage=None, base=None,
                   factors=None):
    """Forward of every PatchApply* Function. p: what K1 pastes — the patch, or with pdesc / max_hw the per-image patches. embed=None: K1 planar
    -> pixel values; embed=(w0, b0, wp0, w1, b1, wp1): K1 writes the two GEMM operands directly (tile-major: no [B,6,224,224] tensor, no im2col
    copies) -> the two patch-embed outputs. stage ("resize" | "jitter"): the per-image patch stage that made p from the base patch `base` [and
    the factors [B,3]]; it stays on ctx and names the adjoint that ends the backward."""
    if embed is None:
        ret, keep = _k1(img_u8, p, xy, theta, geometry, mask_mode, mean6, std6, pdesc, max_hw)
        mask = (keep,)
    else:
        w0, b0, wp0, w1, b1, wp1 = embed
        t0, t1, keep_t, flags = _k1(img_u8, p, xy, theta, geometry, mask_mode, mean6, std6, pdesc, max_hw, tiles=True)
        ret = torch.nn.functional.linear(t0, w0, b0), torch.nn.functional.linear(t1, w1, b1)
        mask = (keep_t, flags, wp0, wp1)
    staged = (pdesc, base, factors if factors is not None else xy) if stage is not None else (xy, xy, xy)
    ctx.save_for_backward(p, xy, theta if geometry else xy, *staged, *mask)
    ctx.geometry, ctx.mask_mode, ctx.std6, ctx.sink = bool(geometry), int(mask_mode), std6, sink
    ctx.stage, ctx.max_hw = stage, (max_hw if stage is not None else None)
    return ret


def _stage_paste_forward(ctx, stage, patch, img_u8, rows, xy, theta, geometry, mask_mode, mean6, std6, embed=None):
    """Forward of the four per-image Functions, which name only their stage: its prologue on the base patch, then the paste of the packed patches."""
    p = patch.detach().contiguous()
    packed, pdesc, max_hw = _stage_pack(stage, p, rows)
    return _paste_forward(ctx, packed, img_u8, xy, theta, geometry, mask_mode, mean6, std6, pdesc, max_hw, embed=embed, stage=stage, base=p,
                          factors=rows if stage == "jitter" else None)


def _paste_backward(ctx, *grads):
    """Backward of every PatchApply* Function: K2 on the pixel gradient, or K2' on the gradients of the two patch-embed outputs. With a sink the
    partial tiles are left in sink["partials"] for the caller's step epilogue and there is no gradient; per-image patches end in the adjoint of
    the stage the forward stored (ctx.stage)."""
    p, xy, theta, pdesc, base, factors, *mask = ctx.saved_tensors
    g = [t.to(torch.bfloat16).contiguous() for t in grads]
    if p.dim() == 4:  # a sweep's patches [P,3,ph,pw]: the keep words are given, K2' never reads patch values, only the [3,ph,pw] shape
        p = p[0]
    theta, resized, defer = theta if ctx.geometry else None, ctx.stage is not None, ctx.sink is not None
    rest = (ctx.geometry, ctx.mask_mode, ctx.std6)
    # through the public wrappers, looked up when called: they are where a caller counts or replaces the K2 / K2' of a step
    if len(g) == 1:
        if resized:
            out = patch_grad_gather_multi(g[0], p, pdesc, ctx.max_hw, xy, theta, mask[0], *rest)
        else:
            out = patch_grad_gather(g[0], p, xy, theta, mask[0], *rest, defer_reduce=defer)
    else:
        keep_t, flags, wp0, wp1 = mask
        if resized:
            out = patch_embed_grad_gather_multi_tiles(g[0], g[1], wp0, wp1, p, pdesc, ctx.max_hw, xy, theta, keep_t, flags, *rest)
        else:
            out = patch_embed_grad_gather_tiles(g[0], g[1], wp0, wp1, p, xy, theta, keep_t, flags, *rest, defer_reduce=defer)
    if defer:
        ctx.sink["partials"] = out
        return None
    if ctx.stage is None:
        return out
    return patch_jitter_bwd(out, base, factors, pdesc) if ctx.stage == "jitter" else patch_resize_bwd(out, pdesc, int(base.shape[1]), int(base.shape[2]))


class PatchApply(torch.autograd.Function):
    """Differentiable (w.r.t. `patch`) K1: PyTorch-ROCm autograd hands the model's bf16 pixel gradient to K2."""

    @staticmethod
    def forward(ctx, patch, img_u8, xy, theta, geometry, mask_mode, mean6=None, std6=None, sink=None):
        """sink (dict, optional): as in PatchApplyEmbed — the backward leaves K2's partial tiles in sink["partials"] and no patch gradient."""
        return _paste_forward(ctx, patch.detach().contiguous(), img_u8, xy, theta, geometry, mask_mode, mean6, std6, sink=sink)

    @staticmethod
    def backward(ctx, gout):
        return (_paste_backward(ctx, gout),) + (None,) * 8


class PatchApplyResized(torch.autograd.Function):
    """resize_patch=True: resize (K0) + K1 with per-image patches forward; K2 (per-image gradients) + resize adjoint backward.
    `sizes` is a host int array [B,2] (h,w); four launches + one fixed-order reduce per step, independent of B."""

    @staticmethod
    def forward(ctx, patch, img_u8, sizes, xy, theta, geometry, mask_mode, mean6=None, std6=None):
        return _stage_paste_forward(ctx, "resize", patch, img_u8, sizes, xy, theta, geometry, mask_mode, mean6, std6)

    @staticmethod
    def backward(ctx, gout):
        return (_paste_backward(ctx, gout),) + (None,) * 8


class PatchApplyJittered(torch.autograd.Function):
    """colorjitter: jitter (K0c) + K1 with per-image patches forward; K2 (per-image gradients) + jitter adjoint backward.
    `factors` is a device tensor [B,3] f32 (brightness, contrast, saturation)."""

    @staticmethod
    def forward(ctx, patch, img_u8, factors, xy, theta, geometry, mask_mode, mean6=None, std6=None):
        return _stage_paste_forward(ctx, "jitter", patch, img_u8, factors, xy, theta, geometry, mask_mode, mean6, std6)

    @staticmethod
    def backward(ctx, gout):
        return (_paste_backward(ctx, gout),) + (None,) * 8


class PatchApplyEmbed(torch.autograd.Function):
    """K1 + both patch-embed GEMMs forward; backward = K2' (SURVEY.md 8f-3): the gradients of the patch-embed OUTPUTS go straight to
    `patch_embed_grad_gather`, which evaluates the patch-embed backward only for the tiles under the patch. w: [D,588], wp: pack_embed_weights(w^T)."""

    @staticmethod
    def forward(ctx, patch, img_u8, xy, theta, geometry, mask_mode, mean6, std6, w0, b0, wp0, w1, b1, wp1, sink=None):
        """sink (a dict, optional): the backward then leaves K2''s partial tiles in sink["partials"] and returns NO gradient for `patch`
        — the caller's step epilogue (ops.step_epilogue) adds them straight into the DDP message."""
        return _paste_forward(ctx, patch.detach().contiguous(), img_u8, xy, theta, geometry, mask_mode, mean6, std6,
                              embed=(w0, b0, wp0, w1, b1, wp1), sink=sink)

    @staticmethod
    def backward(ctx, d0, d1):
        return (_paste_backward(ctx, d0, d1),) + (None,) * 14


class PatchApplySweepEmbed(torch.autograd.Function):
    """PatchApplyEmbed for a maskidx sweep: P groups of Bp images, image b pastes patch b // Bp of `patches` [P,3,ph,pw] (K1 tile-major with a
    per-image descriptor pointing into the shared read-only patches). The backward is K2' with one partial tile per image (P*Bp < 512): it leaves
    the [P*Bp, n] partials in sink["partials"], group g's at rows g*Bp .., for ops.step_epilogue_seg; no gradient is returned."""

    @staticmethod
    def forward(ctx, patches, img_u8, xy, theta, geometry, mask_mode, mean6, std6, w0, b0, wp0, w1, b1, wp1, sink):
        P, ph, pw = int(patches.shape[0]), int(patches.shape[2]), int(patches.shape[3])
        B = int(img_u8.shape[0])
        if B % P != 0:
            raise _lib.VaaError(f"PatchApplySweepEmbed: {B} images are not {P} equal groups")
        if _lib.lib().vaa_patch_grad_partials(B) != B:
            raise _lib.VaaError(f"PatchApplySweepEmbed: {B} images exceed K2''s one-partial-per-image schedule (at most 511)")
        if sink is None:
            raise _lib.VaaError("PatchApplySweepEmbed: the partial tiles need a sink (there is no gradient for `patches`)")
        p = patches.detach().contiguous()
        return _paste_forward(ctx, p, img_u8, xy, theta, geometry, mask_mode, mean6, std6, sweep_pdesc(P, B // P, ph, pw, p.device), (ph, pw),
                              embed=(w0, b0, wp0, w1, b1, wp1), sink=sink)

    @staticmethod
    def backward(ctx, d0, d1):
        return (_paste_backward(ctx, d0, d1),) + (None,) * 14


class PatchApplyResizedEmbed(torch.autograd.Function):
    """resize_patch=True with the pixel gradient un-materialised: resize (K0) + K1 with per-image patches + both patch-embed GEMMs forward;
    K2' in per-image mode + the resize adjoint backward."""

    @staticmethod
    def forward(ctx, patch, img_u8, sizes, xy, theta, geometry, mask_mode, mean6, std6, w0, b0, wp0, w1, b1, wp1):
        return _stage_paste_forward(ctx, "resize", patch, img_u8, sizes, xy, theta, geometry, mask_mode, mean6, std6, (w0, b0, wp0, w1, b1, wp1))

    @staticmethod
    def backward(ctx, d0, d1):
        return (_paste_backward(ctx, d0, d1),) + (None,) * 14


class PatchApplyJitteredEmbed(torch.autograd.Function):
    """colorjitter with the pixel gradient un-materialised: jitter (K0c) + K1 tile-major with per-image patches + both patch-embed GEMMs
    forward; K2' in per-image mode + the jitter adjoint backward."""

    @staticmethod
    def forward(ctx, patch, img_u8, factors, xy, theta, geometry, mask_mode, mean6, std6, w0, b0, wp0, w1, b1, wp1):
        return _stage_paste_forward(ctx, "jitter", patch, img_u8, factors, xy, theta, geometry, mask_mode, mean6, std6, (w0, b0, wp0, w1, b1, wp1))

    @staticmethod
    def backward(ctx, d0, d1):
        return (_paste_backward(ctx, d0, d1),) + (None,) * 14


# ------------------------------------------------------------------------------------------------------
# K3
# ------------------------------------------------------------------------------------------------------
def _dtype_code(logits) -> int:
    """The library's dtype code of a logits tensor (f32 | bf16) on the device."""
    if logits.dtype == torch.float32:
        dt = _lib.DTYPE_F32
    elif logits.dtype == torch.bfloat16:
        dt = _lib.DTYPE_BF16
    else:
        raise _lib.VaaError(f"logits: unsupported dtype {logits.dtype}")
    _need(logits, logits.dtype, "logits")
    return dt


def _loss_params(w, alpha, beta, scale):
    return _lib.f32x([w, alpha, beta, scale])


def _pred_maps(B: int, L: int, device, want: bool = True, want_full=None):
    """The two [B, L-1] prediction maps K3 fills (action-slice argmax, full-vocabulary argmax), None for one that is not wanted."""
    want_full = want if want_full is None else want_full
    return tuple(torch.empty((B, L - 1), dtype=torch.int32, device=device) if on else None for on in (want, want_full))


def _loss_forward(ctx, scalars, pred, pred_full, *saved):
    """The forward tail of the K3 autograd Functions: (total, scalars f32[8], pred_slice, pred_full) with `saved` kept for the backward."""
    ctx.save_for_backward(*saved)
    ctx.mark_non_differentiable(scalars, pred, pred_full)
    return scalars[0].clone(), scalars, pred, pred_full


def _loss_backward(g, gtotal, n_args: int, w_head=None):
    """... and their backward: the gradient the forward produced times d / d total (through the LM-head rows w_head when the forward's first
    argument was the hidden rows), then None for the other n_args - 1 arguments of the forward."""
    d = g * gtotal.to(g.dtype)
    return (d if w_head is None else d @ w_head,) + (None,) * (n_args - 1)


def loss_fwd_bwd(logits, labels, mode: int, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0,
                 layout: int = LAYOUT_FULL, want_grad: bool = True, want_pred: bool = True, glogits=None, want_pred_full: bool = False):
    """K3. Returns (scalars f32[8] on device, pred_tokens i32 [B,L-1] or None, glogits or None[, pred_full i32 [B,L-1]]).

    scalars = [total, CE, w^2*MSE, UPA angle, UPA dist, #CE rows, #action rows, UAD]. pred_tokens = 31744 + argmax of the action
    slice (what UAD uses, UADA.py:395); pred_full (want_pred_full) = argmax over the whole vocabulary (UADA.py:165-167 metrics)."""
    dt = _dtype_code(logits)
    _need(labels, torch.int64, "labels")
    B, Lt = int(labels.shape[0]), int(labels.shape[1])
    if layout == LAYOUT_FULL:
        if logits.dim() != 3 or logits.shape[0] != B:
            raise _lib.VaaError(f"logits: FULL layout expects [B,S,V], got {tuple(logits.shape)}")
        S, V = int(logits.shape[1]), int(logits.shape[2])
    else:
        if logits.dim() != 2:
            raise _lib.VaaError(f"logits: ROWS layout expects [R,V], got {tuple(logits.shape)}")
        S, V = int(logits.shape[0]), int(logits.shape[1])  # ROWS: S carries the row count R
    L = _lib.lib()
    ws = _workspace(logits.device, L.vaa_loss_ws_bytes(B, Lt), "k3")
    scalars = torch.empty(8, dtype=torch.float32, device=logits.device)
    pred, pred_full = _pred_maps(B, Lt, logits.device, want_pred, want_pred_full)
    if want_grad and glogits is None:
        glogits = torch.zeros_like(logits) if layout == LAYOUT_FULL else torch.empty_like(logits)
    with _timed("K3_loss_fwd_bwd", B=B, L=Lt, V=V, dtype=str(logits.dtype), rows=(int(logits.shape[0]) if layout == LAYOUT_ROWS else -1)):
        rc = L.vaa_loss_fwd_bwd_ex(
            logits.data_ptr(), dt, int(layout), labels.data_ptr(), B, S, Lt, V, int(mode), _loss_params(w, alpha, beta, scale),
            scalars.data_ptr(), _ptr(pred), _ptr(pred_full), glogits.data_ptr() if want_grad else None, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "vaa_loss_fwd_bwd")
    if want_pred_full:
        return scalars, pred, (glogits if want_grad else None), pred_full
    return scalars, pred, (glogits if want_grad else None)


class DiscrepancyLoss(torch.autograd.Function):
    """total = loss(logits, labels) with d total/d logits produced by the same fused launch sequence.
    Returns (total, scalars f32[8], pred_slice i32 [B,L-1], pred_full i32 [B,L-1])."""

    @staticmethod
    def forward(ctx, logits, labels, mode, w, alpha, beta, scale, layout):
        scalars, pred, g, pred_full = loss_fwd_bwd(logits.detach(), labels, mode, w, alpha, beta, scale, layout, want_grad=True,
                                                   want_pred_full=True)
        return _loss_forward(ctx, scalars, pred, pred_full, g)

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        return _loss_backward(ctx.saved_tensors[0], gtotal, 8)


# ------------------------------------------------------------------------------------------------------
# K3 on the labelled rows with a prebuilt row map (what the attack loops use)
# ------------------------------------------------------------------------------------------------------
ACTION_LO, N_ACTION = 31744, 256
SLICE_MODES = (LOSS_UADA_DDP, LOSS_UPA)  # gradient confined to the 256 action columns


class LossRowMap:
    """Device row map of a label matrix [B,L] (vaa_loss_rowmap_build): built once per outer iteration, reused by every inner step."""

    def __init__(self, labels: torch.Tensor):
        _need(labels, torch.int64, "labels")
        self.B, self.L = int(labels.shape[0]), int(labels.shape[1])
        L = _lib.lib()
        self.buf = torch.empty(L.vaa_loss_rowmap_bytes(self.B, self.L), dtype=torch.uint8, device=labels.device)
        _lib.check(L.vaa_loss_rowmap_build(labels.data_ptr(), self.B, self.L, self.buf.data_ptr(), self.buf.numel(), _stream()), "vaa_loss_rowmap_build")


class LossRowMapSeg:
    """Segmented device row map (vaa_loss_rowmap_build_seg) of a maskidx sweep: labels [P*Bp, L] = P groups of Bp rows, each with its own masking.
    Usable wherever a LossRowMap is for K3s / K3h (UADA_DDP), and by step_epilogue_seg to fold every group with its own map."""

    def __init__(self, labels: torch.Tensor, P: int):
        _need(labels, torch.int64, "labels")
        self.B, self.L, self.P = int(labels.shape[0]), int(labels.shape[1]), int(P)
        L = _lib.lib()
        nb = L.vaa_loss_rowmap_seg_bytes(self.B, self.L, self.P)
        if nb == 0:
            raise _lib.VaaError(f"LossRowMapSeg: {self.B} label rows are not {self.P} equal groups")
        self.buf = torch.empty(nb, dtype=torch.uint8, device=labels.device)
        _lib.check(L.vaa_loss_rowmap_build_seg(labels.data_ptr(), self.B, self.L, self.P, self.buf.data_ptr(), self.buf.numel(), _stream()),
                   "vaa_loss_rowmap_build_seg")


def loss_rows_fwd_bwd(logits, rowmap: LossRowMap, mode: int, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0,
                      want_grad: bool = True, grad_kind: int = GRAD_FULL, want_pred: bool = True, grad=None):
    """K3 on logits [R,V] of the labelled rows. Returns (scalars f32[8], pred_slice i32 [B,L-1] | None, pred_full i32 [B,L-1] | None,
    grad [R,V] | [R,256] | None). pred_slice = 31744 + argmax of the action logits (UAD), pred_full = argmax over the vocabulary."""
    dt = _dtype_code(logits)
    if logits.dim() != 2:
        raise _lib.VaaError(f"logits: expected [R,V], got {tuple(logits.shape)}")
    R, V = int(logits.shape[0]), int(logits.shape[1])
    B, Lt = rowmap.B, rowmap.L
    L = _lib.lib()
    ws = _workspace(logits.device, L.vaa_loss_rows_ws_bytes(R), "k3")
    scalars = torch.empty(8, dtype=torch.float32, device=logits.device)
    pred, pred_full = _pred_maps(B, Lt, logits.device, want_pred)
    if want_grad and grad is None:
        grad = torch.empty((R, N_ACTION if grad_kind == GRAD_SLICE else V), dtype=logits.dtype, device=logits.device)
    ws = ws if R > 0 else _workspace(logits.device, 256, "k3")
    with _timed("K3_loss_rows_fwd_bwd", B=B, L=Lt, V=V, dtype=str(logits.dtype), rows=R, grad_kind=grad_kind):
        rc = L.vaa_loss_rows_fwd_bwd(logits.data_ptr(), dt, rowmap.buf.data_ptr(), R, B, Lt, V, int(mode), _loss_params(w, alpha, beta, scale),
                                     scalars.data_ptr(), _ptr(pred), _ptr(pred_full), grad.data_ptr() if want_grad else None, int(grad_kind),
                                     ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "vaa_loss_rows_fwd_bwd")
    return scalars, pred, pred_full, (grad if want_grad else None)


def _loss_rows_seg(name, logits, rowmap, P, grad_cols, want_grad, want_pred, grad, call):
    """The body of the segmented K3 calls (vaa_<name>): logits [R,V] of P groups, `rowmap` a LossRowMapSeg of P groups or a LossRowMap with P = 1,
    a gradient of `grad_cols` columns per row (None: full rows). `call(lib, front, outs, tail)` places the entry point's own arguments between the shared ones.
    Returns (scalars f32 [P,8], pred_slice, pred_full i32 [B,L-1] | None (group g's images at rows g*B/P ..), grad | None)."""
    dt = _dtype_code(logits)
    if logits.dim() != 2:
        raise _lib.VaaError(f"logits: expected [R,V], got {tuple(logits.shape)}")
    R, V = int(logits.shape[0]), int(logits.shape[1])
    B, Lt, grad_cols = rowmap.B, rowmap.L, grad_cols or V
    if getattr(rowmap, "P", 1) != P:
        raise _lib.VaaError(f"{name}: the row map holds {getattr(rowmap, 'P', 1)} groups, the call states {P}")
    L = _lib.lib()
    ws = _workspace(logits.device, max(L.vaa_loss_rows_ws_bytes(R), 256), "k3")
    scalars = torch.empty((P, 8), dtype=torch.float32, device=logits.device)
    pred, pred_full = _pred_maps(B, Lt, logits.device, want_pred)
    if want_grad and grad is None:
        grad = torch.empty((R, grad_cols), dtype=logits.dtype, device=logits.device)
    elif want_grad:
        _need(grad, logits.dtype, "grad", (R, grad_cols))
    with _timed("K3_" + name, B=B, L=Lt, V=V, dtype=str(logits.dtype), rows=R, P=P):
        rc = call(L, (logits.data_ptr(), dt, rowmap.buf.data_ptr(), R, B, Lt, V, P),
                  (scalars.data_ptr(), _ptr(pred), _ptr(pred_full), grad.data_ptr() if want_grad else None), (ws.data_ptr(), ws.numel(), _stream()))
    _lib.check(rc, "vaa_" + name)
    return scalars, pred, pred_full, (grad if want_grad else None)


def loss_rows_fwd_bwd_seg(logits, rowmap, P: int, mode: int = LOSS_CE, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0,
                          want_grad: bool = True, want_pred: bool = True, grad=None):
    """K3 in LOSS_CE mode on logits [R,V] of P groups (vaa_loss_rows_fwd_bwd_seg): every row's gradient is normalised by its group's row count, every
    group folded on its own. Returns _loss_rows_seg's tuple with grad [R,V]: per group the bits of loss_rows_fwd_bwd on the group's rows alone."""
    params = _loss_params(w, alpha, beta, scale)
    return _loss_rows_seg("loss_rows_fwd_bwd_seg", logits, rowmap, int(P), None, want_grad, want_pred, grad,
                          lambda L, front, outs, tail: L.vaa_loss_rows_fwd_bwd_seg(*front, int(mode), params, *outs, GRAD_FULL, *tail))


def loss_rows_fwd_bwd_seg_upa(logits, rowmap, P: int, pairs, w: float = 5.0, scale: float = 1.0, want_grad: bool = True, want_pred: bool = True,
                              grad=None):
    """K3 in LOSS_UPA mode on logits [R,V] of P groups with one (alpha, beta) pair each (vaa_loss_rows_fwd_bwd_seg_upa; `pairs` = P (alpha, beta)
    tuples): UPA's batch means are folded per group. Returns _loss_rows_seg's tuple with grad_slice [R,256]: per group the bits of
    loss_rows_fwd_bwd(LOSS_UPA, GRAD_SLICE) on the group's rows alone with its pair."""
    P = int(P)
    pairs = [(float(a), float(b)) for a, b in pairs]
    if len(pairs) != P:
        raise _lib.VaaError(f"loss_rows_fwd_bwd_seg_upa: {len(pairs)} (alpha, beta) pairs for {P} groups")
    params = _lib.f32x([x for a, b in pairs for x in (w, a, b, scale)])
    return _loss_rows_seg("loss_rows_fwd_bwd_seg_upa", logits, rowmap, P, N_ACTION, want_grad, want_pred, grad,
                          lambda L, front, outs, tail: L.vaa_loss_rows_fwd_bwd_seg_upa(*front, params, *outs, *tail))


def loss_rows_stats(logits, rowmap: LossRowMap, mode: int, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0, grad=None):
    """The statistics pass of K3 alone (vaa_loss_rows_stats). In LOSS_UADA_DDP mode `grad` [R,256] receives the gradient slice in the same pass.
    Returns the workspace tensor that step_epilogue folds into the scalars."""
    dt = _dtype_code(logits)
    if logits.dim() != 2:
        raise _lib.VaaError(f"logits: expected [R,V], got {tuple(logits.shape)}")
    R, V = int(logits.shape[0]), int(logits.shape[1])
    L = _lib.lib()
    ws = _workspace(logits.device, L.vaa_loss_rows_ws_bytes(R), "k3")
    if grad is not None:
        _need(grad, logits.dtype, "grad", (R, N_ACTION))
    with _timed("K3_loss_rows_stats", B=rowmap.B, L=rowmap.L, V=V, rows=R):
        rc = L.vaa_loss_rows_stats(logits.data_ptr(), dt, rowmap.buf.data_ptr(), R, rowmap.B, rowmap.L, V, int(mode), _loss_params(w, alpha, beta, scale),
                                   _ptr(grad), GRAD_SLICE, ws.data_ptr(), ws.numel(), _stream())
    _lib.check(rc, "vaa_loss_rows_stats")
    return ws


def head_loss_rows_applies(R: int, D: int, V: int) -> bool:
    return bool(_lib.lib().vaa_head_loss_rows_applies(int(R), int(D), int(V)))


def head_loss_rows_stats(hidden, w_head, rowmap: "LossRowMap", mode: int = LOSS_UADA_DDP, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2,
                         scale: float = 1.0, grad=None, want_logits: bool = False):
    """vaa_head_loss_rows_stats (see _head_stats): returns the K3 workspace for ops.step_epilogue(loss_ws=...) exactly like loss_rows_stats
    (and the bf16 logits [R,V] the statistics were made of when want_logits: tests)."""
    ws, _, dbg = _head_stats(hidden, w_head, rowmap, mode, w, alpha, beta, scale, grad, want_logits)
    return (ws, dbg) if want_logits else ws


def _head_stats(hidden, w_head, rowmap, mode, w, alpha, beta, scale, grad, want_logits):
    """vaa_head_loss_rows_stats: LM head on the labelled rows fused with K3's statistics — `hidden` [R,D] bf16, `w_head` [V,D]
    bf16; the [R,V] logits are never written. Returns (K3 workspace, the head's own workspace [per-workgroup PartStats + slice logits] — the
    very tensor vaa_head_loss_rows_finish must be handed, not a second look-up of the cache —, debug logits | None)."""
    R, D = int(hidden.shape[0]), int(hidden.shape[1])
    V = int(w_head.shape[0])
    _need(hidden, torch.bfloat16, "hidden", (R, D))
    _need(w_head, torch.bfloat16, "w_head", (V, D))
    if grad is not None:
        _need(grad, torch.bfloat16, "grad", (R, N_ACTION))
    L = _lib.lib()
    ws = _workspace(hidden.device, L.vaa_loss_rows_ws_bytes(R), "k3")
    hws = _workspace(hidden.device, L.vaa_head_loss_ws_bytes(R, V), "k3h")
    dbg = torch.empty((R, V), dtype=torch.bfloat16, device=hidden.device) if want_logits else None
    with _timed("K3_head_loss_rows_stats", rows=R, V=V, D=D):
        rc = L.vaa_head_loss_rows_stats(hidden.data_ptr(), w_head.data_ptr(), D, rowmap.buf.data_ptr(), R, rowmap.B, rowmap.L, V, int(mode),
                                        _loss_params(w, alpha, beta, scale), _ptr(grad), ws.data_ptr(), ws.numel(), hws.data_ptr(), hws.numel(),
                                        _ptr(dbg), _stream())
    _lib.check(rc, "vaa_head_loss_rows_stats")
    return ws, hws, dbg


def head_loss_rows_fwd_bwd(hidden, w_head, rowmap: "LossRowMap", mode: int, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0,
                           want_grad: bool = True, want_pred: bool = True, want_logits: bool = False):
    """LM head + K3 on the labelled rows WITHOUT logits in memory: vaa_head_loss_rows_stats (weight stream + per-row fold) followed by
    vaa_head_loss_rows_finish (scalars, prediction maps, UPA's gradient slice). Same returns as loss_rows_fwd_bwd with GRAD_SLICE:
    (scalars f32[8], pred_slice, pred_full, grad [R,256] bf16 | None). A gradient exists for the modes whose loss lives in the action
    columns (SLICE_MODES); the other modes are evaluated only (want_grad=False: validation passes)."""
    if want_grad and mode not in SLICE_MODES:
        raise _lib.VaaError(f"head_loss_rows_fwd_bwd: mode {mode} has a cross-entropy term — its gradient needs the [R,V] logits (HeadLossRows)")
    R = int(hidden.shape[0])
    V = int(w_head.shape[0])
    dev = hidden.device
    grad = torch.empty((R, N_ACTION), dtype=torch.bfloat16, device=dev) if want_grad else None
    ws, hws, lg = _head_stats(hidden, w_head, rowmap, mode, w, alpha, beta, scale, grad if mode == LOSS_UADA_DDP else None, want_logits)
    L = _lib.lib()
    scalars = torch.empty(8, dtype=torch.float32, device=dev)
    pred, pred_full = _pred_maps(rowmap.B, rowmap.L, dev, want_pred)
    with _timed("K3_head_loss_rows_finish", rows=R, V=V):
        rc = L.vaa_head_loss_rows_finish(rowmap.buf.data_ptr(), R, rowmap.B, rowmap.L, V, int(mode), _loss_params(w, alpha, beta, scale), ws.data_ptr(), ws.numel(),
                                         hws.data_ptr(), hws.numel(), scalars.data_ptr(), _ptr(pred), _ptr(pred_full),
                                         grad.data_ptr() if (want_grad and mode == LOSS_UPA) else None, _stream())
    _lib.check(rc, "vaa_head_loss_rows_finish")
    return (scalars, pred, pred_full, grad, lg) if want_logits else (scalars, pred, pred_full, grad)


_slice_t_cache = []  # [(weakref to the weight tensor, its _version when packed, [D,256] transposed action slice)]


def head_slice_applies(R: int, D: int, V: int) -> bool:
    return bool(_lib.lib().vaa_head_slice_applies(int(R), int(D), int(V)))


def head_slice_packed(w_head: torch.Tensor) -> torch.Tensor:
    """[D,256] bf16 transposed copy of the action rows of the LM-head weight (vaa_head_slice_pack), built once per weight TENSOR OBJECT (held by a
    weak reference: an address can be recycled by the allocator, an object cannot) and kept resident — the weights are frozen (UADA_ddp.py:50-51);
    an in-place edit of the weight (its _version) rebuilds it."""
    import weakref

    V, D = int(w_head.shape[0]), int(w_head.shape[1])
    _need(w_head, torch.bfloat16, "w_head", (V, D))
    live = [e for e in _slice_t_cache if e[0]() is not None]
    if len(live) != len(_slice_t_cache):
        _slice_t_cache[:] = live
    for ref, ver, wt in _slice_t_cache:
        if ref() is w_head and ver == w_head._version and wt.device == w_head.device:
            return wt
    wt = torch.empty((D, N_ACTION), dtype=torch.bfloat16, device=w_head.device)
    _lib.check(_lib.lib().vaa_head_slice_pack(w_head.data_ptr(), D, V, wt.data_ptr(), _stream()), "vaa_head_slice_pack")
    _slice_t_cache[:] = [e for e in _slice_t_cache if e[0]() is not w_head][-7:] + [(weakref.ref(w_head), w_head._version, wt)]
    return wt


def head_slice_fwd_bwd(hidden, w_head, rowmap: "LossRowMap", mode: int, w: float = 5.0, alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0,
                       want_dh: bool = True, want_scalars: bool = True, want_grad_slice: bool = False):
    """K3s (vaa_head_slice_fwd_bwd): slice-only LM head + statistics + gradient + head backward in one launch (modes UADA_DDP / UPA).
    Returns dict(dh [R,D] bf16 | None, ws = the K3 workspace (SliceStats + neutral parts: step_epilogue(loss_ws=...) folds it),
    scalars f32[8] | None, pred, pred_full i32 [B,L-1] | None (pred_full = -1: no full-vocabulary argmax on a slice-only step),
    grad_slice [R,256] bf16 | None)."""
    if mode not in SLICE_MODES:
        raise _lib.VaaError(f"head_slice_fwd_bwd: mode {mode} has a cross-entropy term — its loss does not live in the action columns")
    R, D = int(hidden.shape[0]), int(hidden.shape[1])
    V = int(w_head.shape[0])
    _need(hidden, torch.bfloat16, "hidden", (R, D))
    _need(w_head, torch.bfloat16, "w_head", (V, D))
    dev = hidden.device
    L = _lib.lib()
    wt = head_slice_packed(w_head) if want_dh else None
    lws = _workspace(dev, L.vaa_loss_rows_ws_bytes(R), "k3")
    zws = _workspace(dev, L.vaa_head_slice_ws_bytes(R), "k3s")
    dh = torch.empty((R, D), dtype=torch.bfloat16, device=dev) if want_dh else None
    gs = torch.empty((R, N_ACTION), dtype=torch.bfloat16, device=dev) if want_grad_slice else None
    scalars = torch.empty(8, dtype=torch.float32, device=dev) if want_scalars else None
    pred, pred_full = _pred_maps(rowmap.B, rowmap.L, dev, want_scalars)
    with _timed("K3s_head_slice_fwd_bwd", rows=R, D=D):
        rc = L.vaa_head_slice_fwd_bwd(hidden.data_ptr(), w_head.data_ptr(), _ptr(wt), D, rowmap.buf.data_ptr(), R, rowmap.B, rowmap.L, V, int(mode),
                                      _loss_params(w, alpha, beta, scale), _ptr(dh), _ptr(gs), lws.data_ptr(), lws.numel(), _ptr(scalars), _ptr(pred),
                                      _ptr(pred_full), zws.data_ptr(), zws.numel(), _stream())
    _lib.check(rc, "vaa_head_slice_fwd_bwd")
    return {"dh": dh, "ws": lws, "zs": zws, "scalars": scalars, "pred": pred, "pred_full": pred_full, "grad_slice": gs}


def step_epilogue(partials, msg, scalars, rowmap: LossRowMap = None, R: int = 0, V: int = 32064, mode: int = LOSS_UADA_DDP, w: float = 5.0,
                  alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0, loss_ws=None, want_pred: bool = True, update=None):
    """vaa_step_epilogue: msg[0..n) = fixed-order sum of K2's partial tiles [parts, n]; with `rowmap` (+ the workspace loss_rows_stats left)
    K3's statistics are folded into `scalars` (f32[8], output) and the prediction maps; msg[n..n+4) = {CE, w^2*MSE, UAD, total}.
    update = dict(patch=, m=, v=, mode=, lr=, step=, beta1=, beta2=, eps=, stat_part= f64 [ceil(n/64), 2]) fuses K4 (single-GPU step:
    vaa_step_epilogue_update). Returns (pred_slice, pred_full) or (None, None)."""
    return _step_epilogue(None, partials, msg, scalars, rowmap, R, V, mode, w, alpha, beta, scale, loss_ws, want_pred, update)


def step_epilogue_seg(partials, msg, scalars, P: int, rowmap=None, R: int = 0, V: int = 32064, mode: int = LOSS_UADA_DDP, w: float = 5.0,
                      alpha: float = 0.8, beta: float = 0.2, scale: float = 1.0, loss_ws=None, want_pred: bool = True, update=None):
    """vaa_step_epilogue_seg[_update]: step_epilogue for each of P sweep groups in ONE launch. partials [P*nparts, n] (group g's at g*nparts),
    msg f32 [>= P*n + 4P] = [P gradients | P x {CE, w^2*MSE, UAD, total}] (a ZERO tail in the pass-through form, rowmap=None), scalars f32 [P,8]
    (the folded groups; untouched when rowmap is None). update = dict as step_epilogue's, patch / m / v [P*n] and stat_part f64 [P*ceil(n/64), 2].
    Returns (pred_slice, pred_full) [B, L-1] (group g's images at rows g*B/P ..) or (None, None)."""
    return _step_epilogue(int(P), partials, msg, scalars, rowmap, R, V, mode, w, alpha, beta, scale, loss_ws, want_pred, update)


def step_epilogue_seg_tail(partials, msg, scalars_in, P: int, update=None):
    """vaa_step_epilogue_seg_tail[_update]: step_epilogue_seg's pass-through form for a step whose loss scalars are final already (a target sweep:
    loss_rows_fwd_bwd_seg folded them before the backward) — msg = [P gradients | P x scalars_in[g, (1, 2, 7, 0)]]; `update` as step_epilogue_seg's."""
    P = int(P)
    _need(partials, torch.float32, "partials")
    rows, n = int(partials.shape[0]), int(partials.shape[1])
    if rows % P != 0:
        raise _lib.VaaError(f"partials: {rows} tiles are not {P} equal groups")
    _need(msg, torch.float32, "msg")
    _need(scalars_in, torch.float32, "scalars_in", (P, 8))
    if msg.numel() < P * (n + 4):
        raise _lib.VaaError(f"msg: needs {P * (n + 4)} floats, has {msg.numel()}")
    common = (partials.data_ptr(), rows // P, n, P, scalars_in.data_ptr(), msg.data_ptr())
    with _timed("EPI_step_epilogue_seg_tail", n=n, parts=rows // P, P=P):
        if update is None:
            rc = _lib.lib().vaa_step_epilogue_seg_tail(*common, _stream())
        else:
            rc = _lib.lib().vaa_step_epilogue_seg_tail_update(*common, *_update_args(update, P, n), _stream())
    _lib.check(rc, "vaa_step_epilogue_seg_tail")


def _update_args(u, P, n):
    """The K4 arguments of the *_update epilogues from an `update` dict (PatchOptimizer.fused_update_args)."""
    _need(u["patch"], torch.float32, "patch")
    if u["patch"].numel() != P * n:
        raise _lib.VaaError(f"update: patch has {u['patch'].numel()} elements, the gradients {P} x {n}")
    sp = u.get("stat_part")
    if sp is not None:
        _need(sp, torch.float64, "stat_part", (P * ((n + 63) // 64), 2))
    return (u["patch"].data_ptr(), _ptr(u.get("m")), _ptr(u.get("v")), int(u["mode"]), float(u["lr"]), float(u.get("beta1", 0.9)),
            float(u.get("beta2", 0.999)), float(u.get("eps", 1e-6)), int(u["step"]), _ptr(sp))


def _step_epilogue(P, partials, msg, scalars, rowmap, R, V, mode, w, alpha, beta, scale, loss_ws, want_pred, update):
    """The body of step_epilogue (P None: one group, scalars f32[8], vaa_step_epilogue[_update]) and step_epilogue_seg (vaa_step_epilogue_seg[_update])."""
    seg, P = P is not None, P or 1
    name = "vaa_step_epilogue_seg" if seg else "vaa_step_epilogue"
    _need(partials, torch.float32, "partials")
    rows, n = int(partials.shape[0]), int(partials.shape[1])
    if rows % P != 0:
        raise _lib.VaaError(f"partials: {rows} tiles are not {P} equal groups")
    nparts = rows // P
    _need(msg, torch.float32, "msg")
    _need(scalars, torch.float32, "scalars", (P, 8) if seg else (8,))
    if msg.numel() < P * (n + 4):
        raise _lib.VaaError(f"msg: needs {P * (n + 4)} floats, has {msg.numel()}")
    fold = rowmap is not None
    pred, pred_full = _pred_maps(rowmap.B, rowmap.L, msg.device) if fold and want_pred else (None, None)
    common = ((partials.data_ptr(), nparts, n) + ((P,) if seg else ())
              + (rowmap.buf.data_ptr() if fold else None, int(R), rowmap.B if fold else 0, rowmap.L if fold else 0, int(V), int(mode),
                 _loss_params(w, alpha, beta, scale), _ptr(loss_ws), loss_ws.numel() if loss_ws is not None else 0, scalars.data_ptr(),
                 _ptr(pred), _ptr(pred_full), msg.data_ptr()))
    with _timed("EPI_" + name[4:], n=n, parts=nparts, **({"P": P} if seg else {})):
        if update is None:
            rc = getattr(_lib.lib(), name)(*common, _stream())
        else:
            rc = getattr(_lib.lib(), name + "_update")(*common, *_update_args(update, P, n), _stream())
    _lib.check(rc, name)
    return pred, pred_full


class DiscrepancyLossRows(torch.autograd.Function):
    """total = loss(logits [R,V], row map); d total / d logits by the same launch sequence (full-row gradient storage)."""

    @staticmethod
    def forward(ctx, logits, rowmap, mode, w, alpha, beta, scale):
        scalars, pred, pred_full, g = loss_rows_fwd_bwd(logits.detach(), rowmap, mode, w, alpha, beta, scale, want_grad=True, grad_kind=GRAD_FULL)
        return _loss_forward(ctx, scalars, pred, pred_full, g)

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        return _loss_backward(ctx.saved_tensors[0], gtotal, 7)


class HeadLossRows(torch.autograd.Function):
    """LM head + loss on the labelled rows: logits = hidden [R,D] @ W^T [V,D] through hipBLASLt, K3 on them, and
    for the modes whose gradient lives in the 256 action columns (UADA_DDP, UPA) the backward is dh = g_slice [R,256] @ W[31744:32000]
    — a contraction over 256 columns instead of the 32,064 of the generic head backward; other modes contract over the full rows."""

    @staticmethod
    def forward(ctx, hidden, weight, rowmap, mode, w, alpha, beta, scale):
        logits = torch.nn.functional.linear(hidden.detach(), weight)
        sliced = mode in SLICE_MODES
        scalars, pred, pred_full, g = loss_rows_fwd_bwd(logits, rowmap, mode, w, alpha, beta, scale, want_grad=True,
                                                        grad_kind=GRAD_SLICE if sliced else GRAD_FULL)
        ctx.sliced = sliced
        return _loss_forward(ctx, scalars, pred, pred_full, g, weight)

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        g, weight = ctx.saved_tensors
        return _loss_backward(g, gtotal, 8, weight[ACTION_LO : ACTION_LO + N_ACTION] if ctx.sliced else weight)


def _head_seg_forward(ctx, hidden, weight, k3):
    """The forward of the sweeps' GEMM-head Functions: ONE hipBLASLt head over the rows of all groups, `k3(logits)` -> (scalars [P,8], pred_slice,
    pred_full, gradient) with the segmented row map; total = the sum of the groups' totals (the groups share no parameter, so every patch gets its
    own group's gradient)."""
    logits = torch.nn.functional.linear(hidden.detach(), weight)
    scalars, pred, pred_full, g = k3(logits)
    ctx.save_for_backward(g, weight)
    ctx.mark_non_differentiable(scalars, pred, pred_full)
    return scalars[:, 0].sum(), scalars, pred, pred_full


class HeadLossRowsSeg(torch.autograd.Function):
    """HeadLossRows for the sweeps on the GEMM head (P groups): ONE hipBLASLt head over the rows of all groups, K3 with the segmented row map, ONE
    head backward. `pairs` None (a target sweep): LOSS_CE (loss_rows_fwd_bwd_seg), full-row gradient, dh = g @ W. `pairs` = the groups'
    (alpha, beta) (a UPA sweep): LOSS_UPA with `w` (loss_rows_fwd_bwd_seg_upa), dh = g_slice [R,256] @ W[31744:32000] — HeadLossRows' 256-column
    contraction. Returns (total = sum of the groups' totals — the groups share no parameter, so every patch gets its own group's gradient —,
    scalars f32 [P,8], pred_slice, pred_full)."""

    @staticmethod
    def forward(ctx, hidden, weight, rowmap, P, pairs, w, scale):
        ctx.sliced = pairs is not None
        if ctx.sliced:
            return _head_seg_forward(ctx, hidden, weight, lambda z: loss_rows_fwd_bwd_seg_upa(z, rowmap, P, pairs, w=w, scale=scale, want_grad=True))
        return _head_seg_forward(ctx, hidden, weight, lambda z: loss_rows_fwd_bwd_seg(z, rowmap, P, LOSS_CE, scale=scale, want_grad=True))

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        g, weight = ctx.saved_tensors
        return _loss_backward(g, gtotal, 7, weight[ACTION_LO : ACTION_LO + N_ACTION] if ctx.sliced else weight)


class HeadLossRowsFused(torch.autograd.Function):
    """HeadLossRows for the modes whose loss lives in the 256 action columns (UADA_DDP, UPA) with the LM head FUSED into K3's statistics
    (head_loss_rows_fwd_bwd: the [R,V] logits never reach memory); backward dh = g_slice [R,256] @ W[31744:32000] as in HeadLossRows."""

    @staticmethod
    def forward(ctx, hidden, weight, rowmap, mode, w, alpha, beta, scale):
        scalars, pred, pred_full, g = head_loss_rows_fwd_bwd(hidden.detach().contiguous(), weight, rowmap, mode, w, alpha, beta, scale, want_grad=True)
        return _loss_forward(ctx, scalars, pred, pred_full, g, weight)

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        g, weight = ctx.saved_tensors
        return _loss_backward(g, gtotal, 8, weight[ACTION_LO : ACTION_LO + N_ACTION])


_silent_cache = {}


def _silent_outputs(device, B: int, L: int):
    """What a step whose loss scalars nobody reads hands back: zeros[8] and -1 maps (allocated once per device and shape; never written)."""
    key = (device.index, B, L)
    hit = _silent_cache.get(key)
    if hit is None:
        hit = (torch.zeros(8, dtype=torch.float32, device=device), torch.full((B, L - 1), -1, dtype=torch.int32, device=device))
        _silent_cache[key] = hit
    return hit


class HeadSliceLoss(torch.autograd.Function):
    """The slice modes' head + loss + head backward as K3s (head_slice_fwd_bwd: ONE launch; d total / d hidden is produced in the forward and
    handed back by the backward). `read_scalars=False` — a step whose loss scalars the loop never reads (every inner step but the last of an
    outer iteration: UADA_ddp.py:214-221, UPA.py:171-186) — runs the launch without its fold: scalars = 0, maps = -1. `full_ce` — a step whose
    full-vocabulary CE / argmax is READ (the last inner step of the data-parallel UADA loop; validation passes that log CE) — adds K3h's
    statistics pass + fold for the scalars and prediction maps. The gradient path is K3s's on every step, so the patch trajectory does not
    depend on which steps evaluate what.
    Returns (total, scalars f32[8], pred_slice, pred_full); scalars[1] (CE) = 0 and pred_full = -1 unless full_ce."""

    @staticmethod
    def forward(ctx, hidden, weight, rowmap, mode, w, alpha, beta, scale, full_ce, read_scalars=True):
        h = hidden.detach().contiguous()
        full_ce = bool(full_ce and read_scalars)
        o = head_slice_fwd_bwd(h, weight, rowmap, mode, w, alpha, beta, scale, want_dh=True, want_scalars=bool(read_scalars and not full_ce))
        if full_ce:  # K3s left the SliceStats + neutral parts; K3h now writes the real parts (and the same SliceStat bits) into the same workspace
            scalars, pred, pred_full, _ = head_loss_rows_fwd_bwd(h, weight, rowmap, mode, w, alpha, beta, scale, want_grad=False)
        elif read_scalars:
            scalars, pred, pred_full = o["scalars"], o["pred"], o["pred_full"]
        else:
            scalars, pred = _silent_outputs(h.device, rowmap.B, rowmap.L)
            pred_full = pred
        return _loss_forward(ctx, scalars, pred, pred_full, o["dh"])

    @staticmethod
    def backward(ctx, gtotal, _gs, _gp, _gf):
        return _loss_backward(ctx.saved_tensors[0], gtotal, 10)


# ------------------------------------------------------------------------------------------------------
# K4
# ------------------------------------------------------------------------------------------------------
def patch_update(patch, grad, m, v, mode: int, lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-6, l1_clip: float = 0.0, grad_scale: float = 1.0, want_stats: bool = True):
    """K4 (in place on patch/m/v). Returns stats f32[2] = [sum|g|, mean g] (device) or None."""
    return _patch_update(None, patch, grad, m, v, mode, lr, step, beta1, beta2, eps, l1_clip, grad_scale, want_stats)


def patch_update_seg(patch, grad, m, v, P: int, mode: int, lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999,
                     eps: float = 1e-6, l1_clip: float = 0.0, grad_scale: float = 1.0, want_stats: bool = True):
    """K4 on P groups of patch.numel() / P elements in ONE launch (vaa_patch_update_seg): bit for bit P patch_update calls. Returns stats f32 [P,2]."""
    return _patch_update(int(P), patch, grad, m, v, mode, lr, step, beta1, beta2, eps, l1_clip, grad_scale, want_stats)


def _patch_update(P, patch, grad, m, v, mode, lr, step, beta1, beta2, eps, l1_clip, grad_scale, want_stats):
    """The body of patch_update (P None: one group, grad of the patch's shape, stats [2]) and patch_update_seg (stats [P,2])."""
    seg, P = P is not None, P or 1
    name = "vaa_patch_update_seg" if seg else "vaa_patch_update"
    _need(patch, torch.float32, "patch")
    _need(grad, torch.float32, "grad", None if seg else patch.shape)
    n_all = int(patch.numel())
    if grad.numel() != n_all or n_all % P != 0:
        raise _lib.VaaError(f"patch_update_seg: {n_all} patch / {grad.numel()} gradient elements are not {P} equal groups")
    if mode == OPT_ADAMW_HF:
        _need(m, torch.float32, "m", patch.shape)
        _need(v, torch.float32, "v", patch.shape)
    stats = torch.empty((P, 2) if seg else 2, dtype=torch.float32, device=patch.device) if want_stats else None
    with _timed("K4_" + name[4:], n=n_all, **({"P": P} if seg else {})):
        rc = getattr(_lib.lib(), name)(
            patch.data_ptr(), grad.data_ptr(), m.data_ptr() if m is not None else None, v.data_ptr() if v is not None else None,
            n_all // P, *((P,) if seg else ()), int(mode), float(lr), float(beta1), float(beta2), float(eps), int(step), float(l1_clip),
            float(grad_scale), stats.data_ptr() if want_stats else None, _stream())
    _lib.check(rc, name)
    return stats


# ------------------------------------------------------------------------------------------------------
# eval-time paste (simulation_random_patch)
# ------------------------------------------------------------------------------------------------------
def patch_apply_eval(img_u8, patch, xy, theta, geometry):
    """uint8 frames [B,224,224,3] + float patch [3,ph,pw] -> uint8 frames with the (uint8-quantised, optionally warped) patch."""
    B = img_u8.shape[0]
    _need(img_u8, torch.uint8, "img_u8", (B, IMG, IMG, 3))
    _need(patch, torch.float32, "patch")
    _need(xy, torch.int32, "xy", (B, 2))
    _need(theta, torch.float32, "theta", (B, 6))
    _need(geometry, torch.int32, "geometry", (B,))
    out = torch.empty_like(img_u8)
    with _timed("K5_patch_apply_eval", B=B):
        rc = _lib.lib().vaa_patch_apply_eval(img_u8.data_ptr(), patch.data_ptr(), xy.data_ptr(), theta.data_ptr(), geometry.data_ptr(), B,
                                             int(patch.shape[1]), int(patch.shape[2]), out.data_ptr(), _stream())
    _lib.check(rc, "vaa_patch_apply_eval")
    return out


# ------------------------------------------------------------------------------------------------------
# evaluation front end (get_vla_action's centre crop + the processor)
# ------------------------------------------------------------------------------------------------------
def eval_preprocess(img_u8, crop_scale: float = 0.0, mean6=None, std6=None):
    """K7. uint8 frames [B,224,224,3] -> the model's pixel_values, bf16 [B,6,224,224]: centre crop to `crop_scale` of the area and bilinear
    resize back (crop_scale = 0: no crop), uint8 conversion, both normalisations (include/vaa.h states the arithmetic)."""
    B = img_u8.shape[0]
    _need(img_u8, torch.uint8, "img_u8", (B, IMG, IMG, 3))
    out = torch.empty((B, 6, IMG, IMG), dtype=torch.bfloat16, device=img_u8.device)
    mean_c = _MEAN if mean6 is None else _lib.f32x(mean6)
    std_c = _STD if std6 is None else _lib.f32x(std6)
    with _timed("K7_eval_preprocess", B=B):
        rc = _lib.lib().vaa_eval_preprocess(img_u8.data_ptr(), B, float(crop_scale), mean_c, std_c, out.data_ptr(), _stream())
    _lib.check(rc, "vaa_eval_preprocess")
    return out


# ------------------------------------------------------------------------------------------------------
# K9 / K10 / K11, the planar frame stages between K1 and the model: one host layer. Each stage has one row of host float32 values per image
# (its rows spec: the noun of the messages and the width), a forward and an adjoint entry point, and a Function that names only what differs.
# ------------------------------------------------------------------------------------------------------
def _planar_batch(t, name: str) -> int:
    B = t.shape[0] if isinstance(t, torch.Tensor) and t.dim() == 4 else 0
    _need(t, torch.bfloat16, name, (B, 6, IMG, IMG))
    return B


def _host_rows(rows, B: int, width: int, what: str, device):
    """rows [B,width]: a host float32 array (copied to the device here) or a (host array, device tensor) pair. The host copy is what the
    library validates, the device copy what the kernels read (include/vaa.h)."""
    import numpy as np

    host, dev = rows if isinstance(rows, tuple) else (rows, None)
    host = np.ascontiguousarray(np.asarray(host, dtype=np.float32))
    if host.shape != (B, width):
        raise _lib.VaaError(f"{what}: expected shape {(B, width)}, got {host.shape}")
    if dev is None:
        dev = torch.from_numpy(host).to(device, non_blocking=True)
    return host, _need(dev, torch.float32, f"{what} (device copy)", (B, width))


def _stage_call(fn: str, tensors, rows, norm=None, ws=None):
    """One entry point of a frame stage, in the C argument order all of them share: the bf16 [B,6,224,224] `tensors` ((name, tensor), ...), the
    rows pair of `rows` = (what, width, value), [norm = (mean6, std6),] B, the output, [the workspace of ws = (its *_ws_bytes function, its
    _workspace kind),] the stream."""
    B = _planar_batch(tensors[0][1], tensors[0][0])
    for name, t in tensors[1:]:
        _need(t, torch.bfloat16, name, (B, 6, IMG, IMG))
    what, width, value = rows
    host, dev = _host_rows(value, B, width, what, tensors[0][1].device)
    L = _lib.lib()
    args = [t.data_ptr() for _, t in tensors] + [host.ctypes.data, dev.data_ptr()]
    if norm is not None:
        args += [_MEAN if norm[0] is None else _lib.f32x(norm[0]), _STD if norm[1] is None else _lib.f32x(norm[1])]
    out = torch.empty_like(tensors[0][1])
    args += [B, out.data_ptr()]
    if ws is not None:
        buf = _workspace(out.device, getattr(L, ws[0])(B), ws[1])
        args += [buf.data_ptr(), buf.numel()]
    with _timed(fn, B=B):
        rc = getattr(L, fn)(*args, _stream())
    _lib.check(rc, fn)
    return out


def _stage_forward(ctx, fwd, spec, pixel_values, rows, *norm, save_input=False):
    """Forward of every frame-stage Function: `fwd` (the stage's public wrapper) on the contiguous input with the rows pair of spec = (what,
    width), which stays on ctx for the adjoint; save_input: the adjoint reads the forward's input too."""
    x = pixel_values.contiguous() if isinstance(pixel_values, torch.Tensor) else pixel_values
    ctx.rows, ctx.norm = _host_rows(rows, _planar_batch(x, "pixel_values"), spec[1], spec[0], x.device), norm
    if save_input:
        ctx.save_for_backward(x)
    return fwd(x, ctx.rows, *norm)


def _stage_backward(ctx, bwd, gout):
    """Backward of every frame-stage Function: `bwd` on the bf16 gradient [and the saved input]; no gradient for the rows or mean / std."""
    return (bwd(gout.to(torch.bfloat16).contiguous(), *ctx.saved_tensors, ctx.rows, *ctx.norm), None) + (None,) * len(ctx.norm)


# K9: the evaluation's crop inside a training step (crop + bilinear resize of K1's pixel values, and the adjoint)
_BOXES = ("boxes", 4)  # {y1, x1, y2, x2}


def crop_resize_fwd(pixel_values, boxes):
    """K9. pixel_values bf16 [B,6,224,224] (K1's planar output) -> the same planes cropped to each image's box {y1, x1, y2, x2} (normalised
    coordinates, sides in [0.5, 1]) and resized back bilinearly: K7's geometry on the normalised values (include/vaa.h states the arithmetic)."""
    return _stage_call("vaa_crop_resize_fwd", (("pixel_values", pixel_values),), _BOXES + (boxes,))


def crop_resize_bwd(gout, boxes):
    """K9's adjoint: the gradient of crop_resize_fwd's output -> the gradient of its input, the exact transpose of the forward's taps."""
    return _stage_call("vaa_crop_resize_bwd", (("gout", gout),), _BOXES + (boxes,))


class CropResize(torch.autograd.Function):
    """Differentiable K9 between K1 (PatchApply*) and the model: (pixel_values, boxes) -> pixel_values. `boxes`: host float32 [B,4]."""

    @staticmethod
    def forward(ctx, pixel_values, boxes):
        return _stage_forward(ctx, crop_resize_fwd, _BOXES, pixel_values, boxes)

    @staticmethod
    def backward(ctx, gout):
        return _stage_backward(ctx, crop_resize_bwd, gout)


# ------------------------------------------------------------------------------------------------------
# K10: scene-lighting jitter of the pasted frame (brightness, contrast, saturation, hue of the pixel values, and the adjoint)
# ------------------------------------------------------------------------------------------------------
HUE_T = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))  # RGB -> YIQ (include/vaa.h, K10)


def scene_factors(delta, kappa, sigma, hue):
    """Per-image draws -> K10's factor rows, float32 [B,12] = {delta, kappa, sigma, R(hue) row-major}. R(h) = I + Tinv (rot(2 pi h) - I) T in fp64,
    rounded to fp32: exactly the identity for h = 0 (include/vaa.h)."""
    import numpy as np

    d, k, s, h = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (delta, kappa, sigma, hue))
    B = max(d.size, k.size, s.size, h.size)
    d, k, s, h = (np.broadcast_to(v, (B,)) for v in (d, k, s, h))
    T = np.array(HUE_T, np.float64)
    Tinv = np.linalg.inv(T)
    out = np.empty((B, 12), np.float32)
    for b in range(B):
        a = 2.0 * np.pi * h[b]
        c, sn = np.cos(a), np.sin(a)
        rot_m_i = np.array([[0.0, 0.0, 0.0], [0.0, c - 1.0, -sn], [0.0, sn, c - 1.0]])
        R = np.eye(3) + Tinv @ rot_m_i @ T
        out[b, 0], out[b, 1], out[b, 2] = d[b], k[b], s[b]
        out[b, 3:] = R.reshape(9)
    return out


_FACTORS = ("factors", 12)  # {delta, kappa, sigma, R(hue) row-major}
_SCENE_WS = ("vaa_scene_jitter_ws_bytes", "scene")


def scene_jitter_fwd(pixel_values, factors, mean6=None, std6=None):
    """K10. pixel_values bf16 [B,6,224,224] (K1 / K9's planar output) -> the same frames under each image's brightness / contrast / saturation /
    hue factors (`scene_factors`), both towers alike (include/vaa.h states the arithmetic)."""
    return _stage_call("vaa_scene_jitter_fwd", (("pixel_values", pixel_values),), _FACTORS + (factors,), (mean6, std6), _SCENE_WS)


def scene_jitter_bwd(gout, pixel_values, factors, mean6=None, std6=None):
    """K10's adjoint: the gradient of scene_jitter_fwd's output -> the gradient of its input, the exact derivative with torch.clamp's gates
    (recomputed from `pixel_values` and the factors), the whole-image term of the contrast mean included."""
    return _stage_call("vaa_scene_jitter_bwd", (("gout", gout), ("pixel_values", pixel_values)), _FACTORS + (factors,), (mean6, std6), _SCENE_WS)


class SceneJitter(torch.autograd.Function):
    """Differentiable K10 between K1 / K9 and the model: (pixel_values, factors, mean6, std6) -> pixel_values. `factors`: host float32 [B,12]."""

    @staticmethod
    def forward(ctx, pixel_values, factors, mean6=None, std6=None):
        return _stage_forward(ctx, scene_jitter_fwd, _FACTORS, pixel_values, factors, mean6, std6, save_input=True)

    @staticmethod
    def backward(ctx, gout):
        return _stage_backward(ctx, scene_jitter_bwd, gout)


# ------------------------------------------------------------------------------------------------------
# K11: camera defocus blur of the pasted frame (separable 13-tap Gaussian with edge replication on the pixel values, and the adjoint)
# ------------------------------------------------------------------------------------------------------
BLUR_MAX_SIGMA = 2.0  # six taps on each side are 3 sigma at 2.0
BLUR_TAP_FLOOR = 2.0 ** -40  # an un-normalised tap below this is set to 0 (keeps the products out of the subnormals)


def blur_taps(sigma):
    """Per-image sigmas -> K11's tap rows, float32 [B,8] = {w0, ..., w6, 0}; the one place the taps are made. In fp64: e_t = exp(-t^2 / (2 sigma^2))
    for t = 0..6, any e_t < 2^-40 set to 0, divided by e_0 + 2*sum(e_1..e_6), rounded to fp32. sigma == 0 gives exactly (1, 0, ..., 0)."""
    import numpy as np

    s = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if s.ndim != 1 or not np.all(np.isfinite(s)) or np.any(s < 0.0) or np.any(s > BLUR_MAX_SIGMA):
        raise ValueError(f"blur sigma must be finite and in [0, {BLUR_MAX_SIGMA}], got {sigma!r}")
    t = np.arange(7, dtype=np.float64)
    e = np.zeros((s.size, 7), np.float64)
    e[:, 0] = 1.0
    pos = s > 0.0
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):  # a sigma whose square underflows: every e_t but e_0 is 0
        e[pos] = np.exp(-(t[None, :] ** 2) / (2.0 * s[pos, None] ** 2))
    e[:, 0] = 1.0
    e[~(e >= BLUR_TAP_FLOOR)] = 0.0
    e /= (e[:, :1] + 2.0 * e[:, 1:].sum(axis=1, keepdims=True))
    out = np.zeros((s.size, 8), np.float32)
    out[:, :7] = e
    return out


_TAPS = ("taps", 8)  # {w0, ..., w6, 0}


def defocus_blur_fwd(x, taps):
    """K11. x bf16 [B,6,224,224] (K1's planar output) -> every plane under image b's separable 13-tap kernel `taps[b]` (`blur_taps`), rows then
    columns, edges replicated, the intermediate kept in fp32 (include/vaa.h states the arithmetic)."""
    return _stage_call("vaa_defocus_blur_fwd", (("x", x),), _TAPS + (taps,))


def defocus_blur_bwd(gout, taps):
    """K11's adjoint: the gradient of defocus_blur_fwd's output -> the gradient of its input, the exact transpose (the edge rows and columns
    collect the taps the replication folded onto them)."""
    return _stage_call("vaa_defocus_blur_bwd", (("gout", gout),), _TAPS + (taps,))


class DefocusBlur(torch.autograd.Function):
    """Differentiable K11 between K1 (PatchApply*) and K9 / K10 / the model: (pixel_values, taps) -> pixel_values. `taps`: host float32 [B,8]."""

    @staticmethod
    def forward(ctx, pixel_values, taps):
        return _stage_forward(ctx, defocus_blur_fwd, _TAPS, pixel_values, taps)

    @staticmethod
    def backward(ctx, gout):
        return _stage_backward(ctx, defocus_blur_bwd, gout)


# ------------------------------------------------------------------------------------------------------
# camera frames -> 224x224 in front of the eval-time paste (tf.image.resize lanczos3 + round + clip + uint8)
# ------------------------------------------------------------------------------------------------------
_resize_taps: dict = {}


def _frame_taps(H: int, W: int, device):
    """The tap tables of an H x W source, computed once per (H, W, device): the host arrays the library validates and their packed device copy."""
    import numpy as np

    from . import resize

    key = (H, W, device.index if device.index is not None else torch.cuda.current_device())
    hit = _resize_taps.get(key)
    if hit is None:
        sx, wx, sy, wy = (np.ascontiguousarray(t) for t in resize.frame_taps(H, W))
        dev = torch.from_numpy(resize.pack_taps(sx, wx, sy, wy)).to(device)
        hit = _resize_taps[key] = (sx, wx, sy, wy, dev)
    return hit


def resize_frames(frames_u8, rot180: bool = False):
    """K8. uint8 frames [B,H,W,3] (8 <= H, W <= 2048) -> uint8 [B,224,224,3]: the lanczos3 resize with antialias, round half to even, clip
    (include/vaa.h states the arithmetic and the tap rule). rot180: the frames are read as frames[:, ::-1, ::-1] (LIBERO), in the same launch."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise _lib.VaaError("frames_u8: expected a uint8 tensor [B,H,W,3] on a ROCm device (there is no CPU fallback)")
    _need(frames_u8, torch.uint8, "frames_u8")
    B, H, W = (int(v) for v in frames_u8.shape[:3])
    from . import resize

    if not (resize.MIN_SIDE <= H <= resize.MAX_SIDE and resize.MIN_SIDE <= W <= resize.MAX_SIDE):
        raise _lib.VaaError(f"frames_u8: {H}x{W} frames outside [{resize.MIN_SIDE}, {resize.MAX_SIDE}] per side")
    sx, wx, sy, wy, taps = _frame_taps(H, W, frames_u8.device)
    out = torch.empty((B, IMG, IMG, 3), dtype=torch.uint8, device=frames_u8.device)
    with _timed("K8_frame_resize", B=B, H=H, W=W):
        rc = _lib.lib().vaa_frame_resize(frames_u8.data_ptr(), B, H, W, int(bool(rot180)), sx.ctypes.data, wx.ctypes.data, int(wx.shape[1]),
                                         sy.ctypes.data, wy.ctypes.data, int(wy.shape[1]), taps.data_ptr(), out.data_ptr(), _stream())
    _lib.check(rc, "vaa_frame_resize")
    return out


# ------------------------------------------------------------------------------------------------------
# K12: the JPEG round trip of camera frames in front of K8 (tf.io.encode_jpeg + decode_image in the simulators' resize_image)
# ------------------------------------------------------------------------------------------------------
JPEG_DEFAULT_QUALITY = 95  # tf.image.encode_jpeg's default, stated from memory (include/vaa.h)
# Annex K of ITU-T T.81 (luminance, chrominance), natural order
_JPEG_BASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32,
)
_jpeg_qtab_dev: dict = {}


def jpeg_qtables(quality):
    """libjpeg's quantisation tables of an integer quality 1..100, uint16 [2,64] {luminance, chrominance} in natural order: the Annex K tables
    scaled by s = 5000 // q below 50, else 200 - 2q, each entry (base*s + 50) // 100 clamped to 1..255 (baseline)."""
    import numpy as np

    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg quality must be an integer in 1..100, got {quality!r}")
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(_JPEG_BASE, dtype=np.int64) * s + 50) // 100, 1, 255).astype(np.uint16)


def _jpeg_tables(qtables, device):
    """qtables [2,64]: a host uint16 array or a (host array, device tensor) pair. The device copy of a host array is made once per table
    contents and device. The host copy is what the library validates, the device copy what the kernels read (include/vaa.h)."""
    import numpy as np

    host, dev = qtables if isinstance(qtables, tuple) else (qtables, None)
    host = np.asarray(host)
    if host.shape != (2, 64) or host.dtype.kind not in "iu":
        raise _lib.VaaError(f"qtables: expected an integer array of shape (2, 64), got {host.dtype} {host.shape}")
    if host.min() < 0 or host.max() > 65535:
        raise _lib.VaaError("qtables: entries must be in 1..255")
    host = np.ascontiguousarray(host.astype(np.uint16))
    if dev is None:
        key = (device.index if device.index is not None else torch.cuda.current_device(), host.tobytes())
        dev = _jpeg_qtab_dev.get(key)
        if dev is None:
            if len(_jpeg_qtab_dev) >= 64:
                _jpeg_qtab_dev.clear()
            dev = _jpeg_qtab_dev[key] = torch.from_numpy(host.view(np.int16).copy()).to(device)
    return host, _need(dev, torch.int16, "qtables (device copy)", (2, 64))


def jpeg_roundtrip(frames_u8, qtables, rot180: bool = False):
    """K12. uint8 frames [B,H,W,3] (8 <= H, W <= 2048) -> uint8 [B,H,W,3]: the pixels after a baseline 4:2:0 JPEG encoder and decoder of the
    libjpeg family with the quantisation tables `qtables` (`jpeg_qtables(quality)`), integer arithmetic throughout (include/vaa.h states every
    step). rot180: the frames are read as frames[:, ::-1, ::-1] (LIBERO rotates before it encodes). Owns the workspace and the tables' device copy."""
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dim() != 4 or frames_u8.shape[-1] != 3:
        raise _lib.VaaError("frames_u8: expected a uint8 tensor [B,H,W,3] on a ROCm device (there is no CPU fallback)")
    _need(frames_u8, torch.uint8, "frames_u8")
    B, H, W = (int(v) for v in frames_u8.shape[:3])
    host, dev = _jpeg_tables(qtables, frames_u8.device)
    L = _lib.lib()
    out = torch.empty_like(frames_u8)
    nbytes = int(L.vaa_jpeg_roundtrip_ws_bytes(B, H, W))
    ws = _workspace(frames_u8.device, nbytes, "k12") if B > 0 and nbytes > 0 else None
    with _timed("K12_jpeg_roundtrip", B=B, H=H, W=W):
        rc = L.vaa_jpeg_roundtrip(frames_u8.data_ptr(), B, H, W, int(bool(rot180)), host.ctypes.data, dev.data_ptr(), out.data_ptr(),
                                  ws.data_ptr() if ws is not None else None, nbytes if ws is not None else 0, _stream())
    _lib.check(rc, "vaa_jpeg_roundtrip")
    return out
