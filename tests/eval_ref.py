"""References of the evaluation front end (K7, include/vaa.h: vaa_eval_preprocess), shared by test_eval_host.py and test_gpu_eval.py.

  crop_u8_f32  the contract restated in numpy with EVERY operation on np.float32 (one rounding per operation, no FMA): what the kernel must
               reproduce byte for byte.
  crop_u8_f64  the same formulas in float64; the box and the source coordinates are taken in float64 from the float32 crop_scale.
Both map uint8 frames [B,224,224,3] to the uint8 frames the processor sees after get_vla_action's centre crop
(experiments/robot/openvla_utils.py:132-155): TensorFlow's CropAndResize (bilinear, extrapolation value 0) between two convert_image_dtype calls.
"""
import numpy as np

from roboticattack_amd import synthetic

N = 224
SCALES = (0.9, 0.5, 1.0, 0.04)
KINDS = ("noise", "smooth", "constant", "checker")


def frames(kind: str, batch: int = 3, seed: int = 5) -> np.ndarray:
    """uint8 [batch,224,224,3]: synth_images' two kinds, a constant frame (another level per image and channel) and a one-pixel checkerboard."""
    if kind in ("noise", "smooth"):
        return synthetic.synth_images(seed, batch, kind)
    if kind == "constant":
        lv = np.array([[0, 255, 128], [37, 1, 254], [200, 100, 50]], np.uint8)
        return np.broadcast_to(lv[np.arange(batch) % 3][:, None, None, :], (batch, N, N, 3)).copy()
    if kind == "checker":
        yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
        board = ((yy + xx) & 1).astype(np.uint8)
        hi = np.array([255, 200, 13], np.uint8)
        lo = np.array([0, 31, 240], np.uint8)
        one = np.where(board[:, :, None] == 1, hi, lo).astype(np.uint8)
        return np.stack([np.roll(one, b, axis=1) for b in range(batch)])
    raise ValueError(kind)


def _resample(frames_u8, in_c, flt):
    """The bilinear taps of CropAndResize for source coordinates in_c (the same along both axes) in the float type `flt`."""
    f = frames_u8.astype(flt) * (flt(1.0) / flt(255.0))
    lo = np.floor(in_c)
    hi = np.ceil(in_c)
    w = (in_c - lo).astype(flt)
    valid = (in_c >= 0) & (in_c <= N - 1)
    li, hi_i = np.clip(lo, 0, N - 1).astype(np.int64), np.clip(hi, 0, N - 1).astype(np.int64)
    ly, lx = w[None, :, None, None], w[None, None, :, None]
    t, b = f[:, li], f[:, hi_i]
    tl, tr, bl, br = t[:, :, li], t[:, :, hi_i], b[:, :, li], b[:, :, hi_i]
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    v = top + (bot - top) * ly
    ok = valid[None, :, None, None] & valid[None, None, :, None]
    v = np.where(ok, v, flt(0.0))
    assert v.dtype == flt
    return np.minimum(np.maximum(v, flt(0.0)), flt(1.0))


def crop_u8_f32(frames_u8: np.ndarray, crop_scale: float) -> np.ndarray:
    """include/vaa.h's arithmetic, every operation one np.float32 operation. crop_scale == 0: the frames themselves."""
    frames_u8 = np.asarray(frames_u8, dtype=np.uint8)
    if crop_scale == 0:
        return frames_u8.copy()
    f32 = np.float32
    s = np.minimum(np.maximum(np.sqrt(f32(crop_scale)), f32(0.0)), f32(1.0))
    y1 = (f32(1.0) - s) / f32(2.0)
    y2 = y1 + s
    scale = ((y2 - y1) * f32(N - 1)) / f32(N - 1)
    in_c = y1 * f32(N - 1) + np.arange(N, dtype=f32) * scale
    assert in_c.dtype == f32 and scale.dtype == f32
    v = _resample(frames_u8, in_c, f32)
    return np.minimum(255, (v * f32(255.5)).astype(np.int32)).astype(np.uint8)


def crop_u8_f64(frames_u8: np.ndarray, crop_scale: float) -> np.ndarray:
    """The same formulas in float64 (box and coordinates from the float32 crop_scale)."""
    frames_u8 = np.asarray(frames_u8, dtype=np.uint8)
    if crop_scale == 0:
        return frames_u8.copy()
    f64 = np.float64
    s = min(max(np.sqrt(f64(np.float32(crop_scale))), 0.0), 1.0)
    y1 = (1.0 - s) / 2.0
    y2 = y1 + s
    scale = ((y2 - y1) * (N - 1)) / (N - 1)
    in_c = y1 * (N - 1) + np.arange(N, dtype=f64) * scale
    v = _resample(frames_u8, in_c, f64)
    return np.minimum(255, (v * 255.5).astype(np.int32)).astype(np.uint8)
