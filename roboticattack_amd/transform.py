"""RandomPatchTransform — host-side mirror of VLAAttacker/white_patch/appply_random_transform.py:8-197.

Same class name, method names, argument meaning and RNG draw order as the reference; the per-image PyTorch op
chain is replaced by ONE fused HIP launch per batch (K1, `ops.PatchApply`) whose backward is K2. The random
draws stay in Python (`random`, `numpy.random`) so that seeded runs consume the generators exactly like the
reference does; only their results (x, y, 2x3 theta) travel to the device.

Differences a caller can observe (all documented in DESIGN.md):
  * the returned tensor is already bfloat16 (every reference call site casts `.to(torch.bfloat16)` immediately:
    UADA.py:142, UADA_ddp.py:199, UPA.py:142, TMA.py:145); pass out_dtype=torch.float32 to get the fp32 view.
  * images may be a list of PIL images / HWC uint8 arrays (staged to the device once and cached while the same
    list object is passed again, i.e. for all innerLoop steps of an outer iteration) or a uint8 device tensor.
  * Appendix A defects: D1 (IndentationError) n/a; D2 (resize_patch UnboundLocalError) resolved as "scale the BASE
    patch per image"; D3 (`colorjitter=` kwarg, dead in the reference) given a meaning here: a per-image brightness / contrast /
    saturation draw on the patch (include/vaa.h states the arithmetic; `_draw_jitter` the draws). Off by default: zero extra RNG calls.
  * `train_crop`, `scene_jitter`, `defocus_blur` (EXTENSIONS, each off by default: no extra RNG call, no extra launch): the frame stages
    K9 / K10 / K11 on K1's pixel values between the paste and the model — `FRAME_STAGES` the table, `set_frame_stages` what each one does.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .constants import IMG, MAX_ANGLE_DEG, MAX_SHEAR, P_IDENTITY

JITTER_STRENGTH = (0.2, 0.2, 0.2)  # colorjitter=True: brightness, contrast, saturation factors ~ U(1 - s, 1 + s)
SCENE_JITTER_STRENGTH = (0.2, 0.2, 0.2, 0.05)  # scene_jitter=True: OpenVLA's image_aug (prismatic/vla/datasets/datasets.py:126-138)
DEFOCUS_BLUR_SIGMA = 1.0  # defocus_blur=True: sigma ~ U(0, 1.0) pixels per image
TRAIN_CROP_MODES = (None, "center", "random")
TRAIN_CROP_SCALE = 0.9  # the evaluation's centre crop keeps this share of the area (experiments/robot/openvla_utils.py:143)


def train_crop_arg(mode, scale=TRAIN_CROP_SCALE):
    """`train_crop` / `train_crop_scale` as the callers pass them -> (None | "center" | "random", area share in [0.25, 1])."""
    mode = None if mode in (None, False, "none") else mode
    if mode not in TRAIN_CROP_MODES:
        raise ValueError(f"train_crop must be None, 'center' or 'random', got {mode!r}")
    scale = float(scale)
    if not 0.25 <= scale <= 1.0:  # NaN fails both
        raise ValueError(f"train_crop_scale is the crop's share of the area and must be in [0.25, 1] (K9 takes box sides from 0.5), got {scale!r}")
    return mode, scale


def center_crop_box(scale):
    """K7's box for an area share `scale`, in fp32 as vaa_eval_preprocess computes it: s = sqrt(scale), y1 = x1 = (1 - s)/2, y2 = x2 = y1 + s."""
    one = np.float32(1.0)
    s = np.minimum(np.maximum(np.sqrt(np.float32(scale)), np.float32(0.0)), one)
    y1 = (one - s) / np.float32(2.0)
    y2 = y1 + s
    return np.array([y1, y1, y2, y2], np.float32)


def _fit_side(lo, s):
    """[lo, lo + s] in fp32 as K9 accepts it: inside [0, 1], and a side that is still >= 0.5 after the fp32 subtraction."""
    lo = np.float32(lo)
    hi = np.float32(min(np.float32(lo + s), np.float32(1.0)))
    while np.float32(hi - lo) < np.float32(0.5):  # s == 0.5 and a rounding: widen by one ulp on the side that has room
        if hi < np.float32(1.0):
            hi = np.nextafter(hi, np.float32(2.0))
        else:
            lo = np.nextafter(lo, np.float32(-1.0))
    return lo, hi


def jitter_strength(colorjitter):
    """`colorjitter` as the callers pass it -> None (off) or the three strengths (True: the default; a 3-tuple sets them)."""
    if colorjitter is None or colorjitter is False:
        return None
    if colorjitter is True:
        return JITTER_STRENGTH
    s = tuple(float(v) for v in colorjitter)
    if len(s) != 3 or not all(0.0 <= v <= 1.0 for v in s):
        raise ValueError(f"colorjitter must be a bool or three strengths in [0, 1] (brightness, contrast, saturation), got {colorjitter!r}")
    return s


def scene_strength(scene_jitter):
    """`scene_jitter` as the callers pass it -> None (off) or the four strengths (True: OpenVLA's; a 4-tuple sets them): brightness delta ~
    U(-s0, s0), contrast and saturation factors ~ U(1 - s, 1 + s), hue ~ U(-s3, s3) turns."""
    if scene_jitter is None or scene_jitter is False:
        return None
    if scene_jitter is True:
        return SCENE_JITTER_STRENGTH
    s = tuple(float(v) for v in scene_jitter)
    if len(s) != 4 or not all(0.0 <= v <= 1.0 for v in s[:3]) or not 0.0 <= s[3] <= 0.5:
        raise ValueError("scene_jitter must be a bool or four strengths (brightness, contrast, saturation in [0, 1], hue in [0, 0.5]), "
                         f"got {scene_jitter!r}")
    return s


def blur_arg(defocus_blur):
    """`defocus_blur` as the callers pass it -> None (off) or the maximum sigma in pixels (True: DEFOCUS_BLUR_SIGMA; a float in (0, 2.0] sets it)."""
    if defocus_blur is None or defocus_blur is False:
        return None
    if defocus_blur is True:
        return DEFOCUS_BLUR_SIGMA
    try:
        s = float(defocus_blur)
    except (TypeError, ValueError):
        s = float("nan")
    if not 0.0 < s <= ops.BLUR_MAX_SIGMA:  # NaN fails both
        raise ValueError(f"defocus_blur must be a bool or a maximum sigma in (0, {ops.BLUR_MAX_SIGMA}] pixels, got {defocus_blur!r}")
    return s


def _six(mean, std):
    m = [float(v) for t in mean for v in (t.tolist() if hasattr(t, "tolist") else t)]
    s = [float(v) for t in std for v in (t.tolist() if hasattr(t, "tolist") else t)]
    if len(m) != 6 or len(s) != 6:
        raise ValueError("mean/std must be two 3-vectors each (DINOv2 stats, SigLIP stats)")
    return m, s


# The planar frame stages between the paste and the model, in kernel order. flag: the attribute that switches the stage on (None = off);
# function: its ops Function; draw: the method that makes the call's rows, looked up on the instance when the stage runs; train_only: it runs in
# differentiable calls only and its draw takes (batch) — a stage that runs in every call takes (batch, patch) and tells the calls apart itself;
# norm: its Function takes (mean6, std6); why: the reason each refusing site gives (a stage's gradient is one K2' cannot take).
FrameStage = namedtuple("FrameStage", "flag function draw train_only norm why")
FRAME_STAGES = (
    FrameStage("train_crop", ops.CropResize, "_crop_boxes", False, False,
               dict(grad_sink="the pixel gradient goes through the crop adjoint first", apply_sweep_batch="K2' cannot take the cropped gradient",
                    sweep="the sweeps' K2' cannot take the cropped pixel gradient")),
    FrameStage("scene_jitter", ops.SceneJitter, "_scene_draw", True, True,
               dict(grad_sink="the pixel gradient goes through the scene-jitter adjoint first",
                    apply_sweep_batch="K2' cannot take the pixel gradient behind K10", sweep="the sweeps' K2' cannot take the pixel gradient behind K10")),
    FrameStage("defocus_blur", ops.DefocusBlur, "_blur_draw", True, False,
               dict(grad_sink="the pixel gradient goes through the blur adjoint first",
                    apply_sweep_batch="K2' cannot take the pixel gradient behind K11", sweep="the sweeps' K2' cannot take the pixel gradient behind K11")),
)
FRAME_CHAIN = ("defocus_blur", "train_crop", "scene_jitter")  # the order they run (and draw) in: optics, then the crop, then the lighting
assert sorted(FRAME_CHAIN) == sorted(s.flag for s in FRAME_STAGES), "every frame stage has one place in the chain"


def frame_stage(flag):
    """The row of FRAME_STAGES whose flag is `flag` (KeyError: no such stage)."""
    return {s.flag: s for s in FRAME_STAGES}[flag]


class RandomPatchTransform:
    def __init__(self, device, resize_patch: bool = False, train_crop=None, train_crop_scale: float = TRAIN_CROP_SCALE):
        self.device = torch.device(device)
        self.angle = MAX_ANGLE_DEG  # appply_random_transform.py:11
        self.shx = MAX_SHEAR  # :12
        self.shy = MAX_SHEAR  # :13
        self.resize_patch = resize_patch
        self.colorjitter = False  # set by the attackers whose training steps jitter: those steps stay off the fused single-patch paths
        self._staged_key = None
        self._staged = None
        self.embed_with = None  # a model exposing patch_embed_params(): training calls then return ops.PatchEmbeds
        self.last_params = None  # (xy, theta) of the most recent call, host numpy (tests / logging)
        self.last_sizes = None   # resize_patch=True: per-image (h, w) of the most recent call
        self.last_jitter = None  # colorjitter: per-image (brightness, contrast, saturation) factors of the most recent call, float32 [B,3]
        # train_crop: None | "center" | "random" (set_train_crop; set by the attackers like colorjitter: those steps stay off the fused paths)
        self.set_train_crop(train_crop, train_crop_scale)
        self.last_crop = None    # train_crop: per-image boxes {y1, x1, y2, x2} of the most recent call, float32 [B,4]
        self.scene_jitter = None  # None | four strengths (set_scene_jitter; set by the attackers: those steps stay off the fused paths)
        self.last_scene = None   # scene_jitter: K10's factor rows {delta, kappa, sigma, R} of the most recent training call, float32 [B,12]
        self.defocus_blur = None  # None | maximum sigma (set_defocus_blur; set by the attackers: those steps stay off the fused paths)
        self.last_blur = None    # defocus_blur: the per-image sigmas of the most recent training call, float32 [B]

    def set_train_crop(self, mode, scale=TRAIN_CROP_SCALE):
        """Every paste of a training step is followed by the evaluation's crop (K9, ops.CropResize): "center" = K7's box for the area share
        `scale`, "random" = the same side at a per-image random offset (OpenVLA's fine-tuning augmentation); None switches it off."""
        self.train_crop, self.train_crop_scale = train_crop_arg(mode, scale)

    def _crop_boxes(self, batch, patch):
        """The boxes of one call. A differentiable call (a training step) uses `train_crop`; any other call (the validation passes inside the
        loops) the centre box, which is what the evaluation will do. "center" makes no RNG call; "random" makes 2 per image after every other
        draw of the call, image-major: y1 = random.uniform(0, 1 - s), then x1."""
        box = center_crop_box(self.train_crop_scale)
        boxes = np.tile(box, (batch, 1))
        if self.train_crop == "random" and patch.requires_grad and torch.is_grad_enabled():
            s = box[2] - box[0]
            for b in range(batch):
                y1, y2 = _fit_side(random.uniform(0.0, 1.0 - float(s)), s)
                x1, x2 = _fit_side(random.uniform(0.0, 1.0 - float(s)), s)
                boxes[b] = (y1, x1, y2, x2)
        self.last_crop = boxes
        return boxes

    def set_scene_jitter(self, strength):
        """Every paste of a training step is followed (behind K9) by a per-image brightness / contrast / saturation / hue draw of the whole
        frame (K10, ops.SceneJitter): True = OpenVLA's strengths (0.2, 0.2, 0.2, 0.05), four strengths set them, None / False switch it off."""
        self.scene_jitter = scene_strength(strength)

    def _scene_draw(self, batch):
        """4 * batch calls random.uniform, image-major, after every other draw of the call: delta ~ U(-s0, s0), kappa ~ U(1 - s1, 1 + s1),
        sigma ~ U(1 - s2, 1 + s2), h ~ U(-s3, s3)."""
        s = self.scene_jitter
        d = np.empty((batch, 4), np.float64)
        for b in range(batch):
            d[b] = (random.uniform(-s[0], s[0]), random.uniform(1.0 - s[1], 1.0 + s[1]), random.uniform(1.0 - s[2], 1.0 + s[2]),
                    random.uniform(-s[3], s[3]))
        self.last_scene = ops.scene_factors(d[:, 0], d[:, 1], d[:, 2], d[:, 3])
        return self.last_scene

    def set_defocus_blur(self, max_sigma):
        """Every paste of a training step is followed at once (in front of K9 and K10) by a Gaussian blur of the whole frame with a per-image
        sigma ~ U(0, max_sigma) pixels (K11, ops.DefocusBlur): True = 1.0, a float in (0, 2.0] sets it, None / False switch it off."""
        self.defocus_blur = blur_arg(max_sigma)

    def _blur_draw(self, batch):
        """batch calls random.uniform(0, max_sigma), image-major, after the paste's own draws and before the crop's and the scene's."""
        self.last_blur = np.array([random.uniform(0.0, self.defocus_blur) for _ in range(batch)], np.float32)
        return ops.blur_taps(self.last_blur)  # from the fp32 sigmas: ops.blur_taps(last_blur) reproduces the call's taps

    def set_frame_stages(self, train_crop=None, train_crop_scale=TRAIN_CROP_SCALE, scene_jitter=False, defocus_blur=False):
        """The three frame stages as the attackers' keywords name them (EXTENSIONS, all off by default); `_finish` chains the ones that are set.
        train_crop (None | "center" | "random", with train_crop_scale the crop's share of the area): every training step sends the pasted frames
        through the evaluation's crop (K9 on K1's pixel values); the validation passes use the centre box, as the evaluation will.
        scene_jitter (True = OpenVLA's image_aug strengths (0.2, 0.2, 0.2, 0.05), or four strengths): every training step ends in a per-image
        brightness / contrast / saturation / hue draw of the whole pasted frame (K10, behind K9); validation passes get none.
        defocus_blur (True = a maximum sigma of 1.0 pixels, or a maximum sigma in (0, 2.0]): every training step blurs the pasted frame with a
        per-image Gaussian of sigma ~ U(0, maximum) (K11, in front of K9 and K10); validation passes see the sharp frame.
        A step with any of them takes the planar, un-fused path (K2' cannot take the gradient behind them); the sweeps refuse all three."""
        self.set_train_crop(train_crop, train_crop_scale)
        self.set_scene_jitter(scene_jitter)
        self.set_defocus_blur(defocus_blur)

    def frame_stages_on(self):
        """The flags of the frame stages that are set, in FRAME_STAGES' order: what keeps a step off K2' (grad_sink, the sweeps, the fused paths)."""
        return tuple(s.flag for s in FRAME_STAGES if getattr(self, s.flag) is not None)

    def _refuse_frame_stages(self, site):
        """`site` ("grad_sink" | "apply_sweep_batch") hands K2' the gradient: ValueError naming the first frame stage that is set, and why."""
        on = self.frame_stages_on()
        if on:
            raise ValueError(f"{site} is not available with {on[0]} ({frame_stage(on[0]).why[site]})")

    def _finish(self, out, patch, out_dtype, mean6=None, std6=None):
        """The tail of every paste that returns pixel values: the frame stages that are set, in FRAME_CHAIN's order ([K11 with the call's taps
        ->] [K9 with the call's boxes ->] [K10 with the call's factors]), then the caller's dtype. K11 and K10 run in a differentiable call only
        (a training step): the validation passes inside the loops see the frame sharp and as it is lit. Draw order behind the paste's own
        draws, the chain's: the blur's sigmas (one per image), then the crop's offsets (two per image), then the scene's factors (four per
        image), each image-major."""
        training = patch.requires_grad and torch.is_grad_enabled()
        for stage in map(frame_stage, FRAME_CHAIN):
            if getattr(self, stage.flag) is None or (stage.train_only and not training):
                continue
            draw, batch = getattr(self, stage.draw), int(out.shape[0])
            rows = draw(batch) if stage.train_only else draw(batch, patch)
            out = stage.function.apply(out, rows, mean6, std6) if stage.norm else stage.function.apply(out, rows)
        return out if out_dtype == torch.bfloat16 else out.to(out_dtype)

    # ---- small tensor helpers kept for API compatibility (:16-24) ----
    def normalize(self, images, mean, std):
        return (images - mean[None, :, None, None]) / std[None, :, None, None]

    def denormalize(self, images, mean, std):
        return images * std[None, :, None, None] + mean[None, :, None, None]

    # ---- geometry (:26-41, :80-91) ----
    def rotation_matrix(self, theta):
        t = np.deg2rad(theta)
        c, s = np.cos(t), np.sin(t)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float32)

    def shear_matrix(self, shx, shy):
        return np.array([[1, shx, 0], [shy, 1, 0], [0, 0, 1]], dtype=np.float32)

    def combined_transform_matrix(self):
        """p=0.2 identity, else S(shx,shy) @ R(angle) with angle~U(-30,30) deg, shear~U(-0.2,0.2); float32 3x3 tensor."""
        if np.random.rand() < P_IDENTITY:
            return torch.tensor(np.eye(3, dtype=np.float32))
        angle = np.random.uniform(-self.angle, self.angle)
        shx = np.random.uniform(-self.shx, self.shx)
        shy = np.random.uniform(-self.shy, self.shy)
        return torch.tensor(np.dot(self.shear_matrix(shx, shy), self.rotation_matrix(angle)))

    # ---- staging ----
    def stage_images(self, images) -> torch.Tensor:
        """uint8 [B,224,224,3] on the device. The reference re-runs ToTensor + H2D for every image on every inner step
        (:108); the frames do not change during an outer iteration, so they are staged once."""
        if isinstance(images, torch.Tensor):
            t = images
            if t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (IMG, IMG, 3):
                raise ValueError("image tensor must be uint8 [B,224,224,3] (HWC)")
            return t.to(self.device).contiguous()
        # the cache holds the list object itself and compares by identity (an id() alone can be recycled by a new list)
        if self._staged_key is images and self._staged is not None and self._staged.shape[0] == len(images):
            return self._staged
        arr = np.stack([np.asarray(im, dtype=np.uint8) for im in images])
        if arr.shape[1:] != (IMG, IMG, 3):
            raise ValueError(f"images must be 224x224 RGB, got {arr.shape[1:]}")
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device, non_blocking=True)
        self._staged_key, self._staged = images, t
        return t

    def _draw(self, batch, ph, pw, geometry):
        """RNG draw order per image (:120-128): randint(x), randint(y), then (geometry) rand [, uniform x3]."""
        xy = np.empty((batch, 2), np.int32)
        theta = np.empty((batch, 6), np.float32)
        for b in range(batch):
            xy[b, 0] = random.randint(0, IMG - pw)
            xy[b, 1] = random.randint(0, IMG - ph)
            m = self.combined_transform_matrix().numpy() if geometry else np.eye(3, dtype=np.float32)
            theta[b] = m[:2].reshape(6)
        return xy, theta

    _RING = 8  # staging slots: the host may run several steps ahead of the GPU

    def _to_dev(self, xy, theta):
        """(x, y) and theta of one step -> device tensors through ONE pinned staging buffer and ONE async copy (the only host->device traffic
        of a step: 32 B per image). The HOST side is a ring of pinned slots, each guarded by the event of the copy that last read it; the
        DEVICE side is a fresh tensor from the caching allocator per call (no launch, no hipMalloc), so a tensor that an autograd graph saved
        for its backward (PatchApply / PatchApplyEmbed keep xy and theta) lives exactly as long as that graph — however many later calls
        (validation sweeps, micro-batches built before backward, retain_graph) happen in between (round 3 handed out views of a reused
        8-slot device ring: ADVICE r3)."""
        self.last_params = (xy, theta)
        if self.device.type != "cuda":
            return torch.from_numpy(xy).to(self.device), torch.from_numpy(theta).to(self.device)
        B = int(xy.shape[0])
        ring = getattr(self, "_ring", None)
        if ring is None or ring["B"] != B:
            ring = self._ring = {"B": B, "i": 0, "host": [torch.empty(8 * B, dtype=torch.int32).pin_memory() for _ in range(self._RING)],
                                 "ev": [None] * self._RING}
        k = ring["i"]
        ring["i"] = (k + 1) % self._RING
        if ring["ev"][k] is not None:
            ring["ev"][k].synchronize()  # the copy that last read this slot is done (it was enqueued _RING steps ago)
        h, d = ring["host"][k], torch.empty(8 * B, dtype=torch.int32, device=self.device)
        hn = h.numpy()
        hn[: 2 * B] = xy.reshape(-1)
        hn[2 * B :].view(np.float32)[:] = theta.reshape(-1)
        d.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        ring["ev"][k] = ev
        return d[: 2 * B].view(B, 2), d[2 * B :].view(torch.float32).view(B, 6)

    # ---- the operators ----
    def apply_random_patch_batch(self, images, patch, mean, std, geometry, colorjitter=False, out_dtype=torch.bfloat16, grad_sink=None, draws=None):
        """Paste `patch` at a random position of every image, optionally warp it by a random rotation+shear, composite
        where the warped canvas is >= -20, normalise twice and stack to 6 channels (:104-136). Differentiable w.r.t. patch.
        grad_sink (dict, one patch for the batch): the backward leaves K2's (or K2''s) partial tiles in grad_sink["partials"] instead of a
        patch gradient — the caller adds them with ops.step_epilogue (into the DDP message and / or straight through the optimiser).
        draws: (xy, theta) host arrays from `draw_params` to use instead of drawing (a maskidx sweep hands every group the same draws).
        colorjitter (True: strengths 0.2 each; or three strengths): every image pastes its own brightness / contrast / saturation variant of the
        patch (`_apply_jittered`); False makes no extra RNG call.
        With a frame stage set (`set_frame_stages`) the result is K1's pixel values behind `_finish`'s chain (the planar path; no grad_sink)."""
        if grad_sink is not None:
            self._refuse_frame_stages("grad_sink")
        mean6, std6 = _six(mean, std)
        img = self.stage_images(images)
        B = img.shape[0]
        strength = jitter_strength(colorjitter)
        if strength is not None:
            if self.resize_patch:
                raise ValueError("colorjitter with resize_patch is not supported")
            if grad_sink is not None:
                raise ValueError("grad_sink is not available with colorjitter (per-image gradients go through the jitter adjoint)")
            return self._apply_jittered(img, patch, mean6, std6, geometry, out_dtype, strength, draws)
        if self.resize_patch:
            if grad_sink is not None:
                raise ValueError("grad_sink is not available with resize_patch=True (per-image gradients go through the resize adjoint)")
            return self._apply_resized(img, patch, mean6, std6, geometry, out_dtype)
        ph, pw = int(patch.shape[1]), int(patch.shape[2])
        xy, theta = self._to_dev(*(draws if draws is not None else self._draw(B, ph, pw, geometry)))
        return self._paste_tail((ops.PatchApply, ops.PatchApplyEmbed), (), patch, img, xy, theta, geometry, ops.MASK_LT_M20, mean6, std6, out_dtype,
                                (grad_sink,))

    def draw_params(self, batch, ph, pw, geometry):
        """The host draws of one apply_random_patch_batch call on `batch` frames (the same RNG consumption), for `draws=` / apply_sweep_batch."""
        return self._draw(batch, ph, pw, geometry)

    def apply_sweep_batch(self, images, patches, mean, std, geometry, grad_sink, draws=None):
        """maskidx sweep (training step): `images` uint8 [P*Bp,224,224,3] = the same Bp frames replicated P times, `patches` [P,3,ph,pw]; image b
        gets patch b // Bp and the draws of frame b % Bp — ONE draw per frame, exactly what a standalone call on the Bp frames consumes, shared by
        every group. Returns the patch-embed outputs (ops.PatchEmbeds); the backward leaves the per-image partial tiles in grad_sink["partials"]."""
        mean6, std6 = _six(mean, std)
        img = self.stage_images(images)
        P, ph, pw = int(patches.shape[0]), int(patches.shape[2]), int(patches.shape[3])
        Bp = int(img.shape[0]) // P
        if self.embed_with is None:
            raise ValueError("apply_sweep_batch needs a model that exposes its patch-embed weights")
        self._refuse_frame_stages("apply_sweep_batch")
        xy_n, th_n = draws if draws is not None else self._draw(Bp, ph, pw, geometry)
        xy, theta = self._to_dev(np.tile(xy_n, (P, 1)), np.tile(th_n, (P, 1)))
        emb = self.embed_with.patch_embed_params()
        return ops.PatchEmbeds(ops.PatchApplySweepEmbed.apply(patches, img, xy, theta, bool(geometry), ops.MASK_LT_M20, mean6, std6, *emb, grad_sink))

    def _embed_params(self, patch, out_dtype):
        """Patch-embed weights for the path that never materialises the pixel gradient — only for differentiable bf16 calls, and never with a
        frame stage set: K2' evaluates only the tiles under the uncropped patch and cannot be fed the gradient behind K9 / K10 / K11."""
        if self.frame_stages_on() or self.embed_with is None or not patch.requires_grad or out_dtype != torch.bfloat16 or not torch.is_grad_enabled():
            return None
        return self.embed_with.patch_embed_params()

    def _paste_tail(self, functions, lead, patch, img, xy, theta, geometry, mask_mode, mean6, std6, out_dtype, sink=()):
        """The tail of the four paste sites. functions: the site's (planar, embed) Function pair; lead: their arguments in front of xy (nothing,
        the sizes, the factors); sink: (grad_sink,) at the one site whose pair takes it. With patch-embed weights (`_embed_params`) the embed
        Function's outputs as ops.PatchEmbeds, else the planar Function's pixel values behind `_finish`."""
        planar, embed = functions
        emb = self._embed_params(patch, out_dtype)
        if emb is not None:
            return ops.PatchEmbeds(embed.apply(patch, img, *lead, xy, theta, bool(geometry), mask_mode, mean6, std6, *emb, *sink))
        return self._finish(planar.apply(patch, img, *lead, xy, theta, bool(geometry), mask_mode, mean6, std6, *sink), patch, out_dtype, mean6, std6)

    def _draw_resized(self, batch, ph0, pw0, geometry):
        """Draw order per image with resize_patch=True (:114, :123-128): uniform (scale) BEFORE the position, the position against
        the resized size, then the transform matrix."""
        sizes = np.empty((batch, 2), np.int32)
        xy = np.empty((batch, 2), np.int32)
        theta = np.empty((batch, 6), np.float32)
        for b in range(batch):
            scale = random.uniform(0.61, 1.39)
            h, w = max(1, int(ph0 * scale)), max(1, int(pw0 * scale))
            sizes[b] = (h, w)
            xy1, th1 = self._draw(1, h, w, geometry)
            xy[b], theta[b] = xy1[0], th1[0]
        return sizes, xy, theta

    def _apply_resized(self, img, patch, mean6, std6, geometry, out_dtype):
        """resize_patch=True (:113-116, Appendix A-D2): per image s~U(0.61,1.39); the BASE patch is resized (bilinear, antialias)
        to (int(ph*s), int(pw*s)). The whole batch is one resize launch + one K1 launch with per-image patches
        (`ops.PatchApplyResized`); the backward is K2 with per-image outputs + the resize adjoint."""
        sizes, xy_n, theta_n = self._draw_resized(img.shape[0], int(patch.shape[1]), int(patch.shape[2]), geometry)
        self.last_sizes = sizes
        xy, theta = self._to_dev(xy_n, theta_n)
        return self._paste_tail((ops.PatchApplyResized, ops.PatchApplyResizedEmbed), (sizes,), patch, img, xy, theta, geometry, ops.MASK_LT_M20,
                                mean6, std6, out_dtype)

    def _draw_jitter(self, batch, strength):
        """3 * batch calls random.uniform(1 - s_k, 1 + s_k): image-major, in order brightness, contrast, saturation."""
        f = np.empty((batch, 3), np.float32)
        for b in range(batch):
            for k in range(3):
                f[b, k] = random.uniform(1.0 - strength[k], 1.0 + strength[k])
        return f

    def _apply_jittered(self, img, patch, mean6, std6, geometry, out_dtype, strength, draws=None):
        """colorjitter: the placement draws of the un-jittered call first, then the factors. The whole batch is one jitter launch + one K1
        launch with per-image patches (`ops.PatchApplyJittered`); the backward is K2 / K2' with per-image outputs + the jitter adjoint."""
        B, ph, pw = int(img.shape[0]), int(patch.shape[1]), int(patch.shape[2])
        xy_n, theta_n = draws if draws is not None else self._draw(B, ph, pw, geometry)
        self.last_jitter = self._draw_jitter(B, strength)
        xy, theta = self._to_dev(xy_n, theta_n)
        factors = torch.from_numpy(self.last_jitter).to(self.device, non_blocking=True)
        return self._paste_tail((ops.PatchApplyJittered, ops.PatchApplyJitteredEmbed), (factors,), patch, img, xy, theta, geometry, ops.MASK_LT_M20,
                                mean6, std6, out_dtype)

    def _paste(self, images, patch, mean, std, out_dtype):
        mean6, std6 = _six(mean, std)
        img = self.stage_images(images)
        ph, pw = int(patch.shape[1]), int(patch.shape[2])
        xy, theta = self._to_dev(*self._draw(img.shape[0], ph, pw, False))
        return self._paste_tail((ops.PatchApply, ops.PatchApplyEmbed), (), patch, img, xy, theta, False, ops.MASK_NE_M100, mean6, std6, out_dtype), xy

    def random_paste_patch(self, images, patch, mean, std, out_dtype=torch.bfloat16):
        """:138-158 — paste without warp, mask rule `canvas != -100`."""
        return self._paste(images, patch, mean, std, out_dtype)[0]

    def paste_patch_fix(self, images, patch, mean, std, inference=False, out_dtype=torch.bfloat16):
        """:160-188 — identical to random_paste_patch; with inference=True also returns the per-image canvases."""
        out, xy = self._paste(images, patch, mean, std, out_dtype)
        if not inference:
            return out
        ph, pw = int(patch.shape[1]), int(patch.shape[2])
        canvases = []
        for b, (x, y) in enumerate(self.last_params[0]):
            c = torch.ones(3, IMG, IMG, device=self.device) * -100
            c[:, y : y + ph, x : x + pw] = patch.detach()
            canvases.append(c)
        return out, canvases

    def simulation_random_patch(self, image, patch, geometry=False, colorjitter=False, angle=1, shx=0.1, shy=0.1, position=(0, 0)):
        """:43-78 — eval-time paste on ONE uint8 HWC frame (numpy in, numpy out) with a fixed angle/shear/position."""
        out = self.simulation_patch_batch(np.asarray(image, dtype=np.uint8)[None], patch, [geometry], [angle], [shx], [shy], [position])
        return out[0].cpu().numpy()

    def simulation_patch_batch(self, images_u8, patch, geometry, angle, shx, shy, position) -> torch.Tensor:
        """Batched form for rollouts: per-frame geometry flag, angle (deg), shears and (x, y); returns uint8 [B,224,224,3] on device."""
        img = self.stage_images(torch.as_tensor(np.asarray(images_u8)) if not isinstance(images_u8, torch.Tensor) else images_u8)
        B = img.shape[0]
        theta = np.empty((B, 6), np.float32)
        for b in range(B):
            m = np.dot(self.shear_matrix(shx[b], shy[b]), self.rotation_matrix(angle[b])) if geometry[b] else np.eye(3, dtype=np.float32)  # :66-73
            theta[b] = m[:2].reshape(6)
        xy = torch.from_numpy(np.asarray(position, np.int32).reshape(B, 2)).to(self.device)
        geo = torch.from_numpy(np.asarray(geometry).astype(np.int32)).to(self.device)
        return ops.patch_apply_eval(img, patch.detach().to(self.device, torch.float32).contiguous(), xy, torch.from_numpy(theta).to(self.device), geo)

    def eval_pixel_values(self, frames_u8, mean, std, center_crop=False, crop_scale=0.9, out_dtype=torch.bfloat16):
        """The evaluation's image front end behind the paste (experiments/robot/openvla_utils.py:132-166): uint8 frames [B,224,224,3] (numpy or
        a device tensor, e.g. simulation_patch_batch's output) -> pixel_values [B,6,224,224]. center_crop=True crops the centre to `crop_scale`
        of the area and resizes back bilinearly before the uint8 conversion (mandatory for the fine-tuned LIBERO checkpoints); one launch (K7)."""
        mean6, std6 = _six(mean, std)
        img = self.stage_images(frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.as_tensor(np.asarray(frames_u8)))
        out = ops.eval_preprocess(img, float(crop_scale) if center_crop else 0.0, mean6, std6)
        return out if out_dtype == torch.bfloat16 else out.to(out_dtype)

    def eval_frames(self, frames, rot180=False, jpeg_quality=None) -> torch.Tensor:
        """A simulator's camera frames, uint8 [F,H,W,3] of any size from 8 to 2048 per side (numpy or a tensor) -> uint8 [F,224,224,3] on the
        device, as the reference's evaluations hand them on (experiments/robot/libero/libero_utils.py:44-58, bridgev2_utils.py:112): lanczos3
        resize with antialias, round, clip; rot180=True reads the frames as frames[:, ::-1, ::-1] first (LIBERO). One launch (K8).
        jpeg_quality (an integer 1..100; LIBERO's resize_image: 95): the frames go through a JPEG encoder and decoder at that quality first
        (libero_utils.py:42-43), after the rotation and before the resize: K12 with rot180, then K8 without it."""
        t = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(frames)))
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3:
            raise ValueError("frames must be uint8 [F,H,W,3] (HWC)")
        if jpeg_quality is None:
            return ops.resize_frames(t.to(self.device).contiguous(), rot180)
        return ops.resize_frames(ops.jpeg_roundtrip(t.to(self.device).contiguous(), ops.jpeg_qtables(jpeg_quality), rot180), False)

    def im_process(self, images, mean, std, out_dtype=torch.bfloat16):
        """:190-197 — normalise the clean frames only (K1 with a 1x1 sentinel patch that is never kept)."""
        mean6, std6 = _six(mean, std)
        img = self.stage_images(images)
        B = img.shape[0]
        sentinel = torch.full((3, 1, 1), -100.0, device=self.device)
        xy = torch.zeros((B, 2), dtype=torch.int32, device=self.device)
        out, _ = ops.patch_apply_fwd(img, sentinel, xy, None, False, ops.MASK_LT_M20, want_keep=False, mean6=mean6, std6=std6)
        return out if out_dtype == torch.bfloat16 else out.to(out_dtype)
