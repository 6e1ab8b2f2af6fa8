"""fp64 reference for K10 (include/vaa.h: vaa_scene_jitter_fwd / _bwd), the scene-lighting jitter of the pasted frame.

Three statements of the header's arithmetic, and the bounds the GPU tests hold the kernels to:
  * `fwd64` / `bwd64`: NumPy, float64, forward and hand-written adjoint (torch.clamp's gate at each clamp, the transposed hue matrix, the
    whole-image term of the contrast mean).
  * `fwd_torch`: the same forward in torch.float64, so torch.autograd supplies a gradient that shares no line with `bwd64`.
  * `fwd_bound` / `bwd64`'s bound: per-element bounds of |kernel - reference|, derived below from the arithmetic, never from a kernel's output.

Inputs of the fp32 kernel are exact in fp64 (bf16 values, fp32 factors, fp32 mean / std, the fp32 roundings of 0.299 / 0.587 / 0.114, the fp32
differences 1 - kappa and 1 - sigma), so the reference differs from the kernel by the kernel's own roundings only. With u = 2^-24 (fp32, round to
nearest: |fl(a) - a| <= u |a|), first-order error propagation through the header's chain gives, per element (e_k the bound after stage k; clamp is
1-Lipschitz, so e(y_k) <= e(pre_k) at EVERY element, gate or not — the forward is continuous and is compared everywhere):
    p    = fma(x, std, mean)                 e_p   = u |p|
    pre1 = p + delta                         e_1   = e_p + u |pre1|
    m    = fp32(fp64 sum / N)                e_m   = mean over the pixels of e_1 + u |m|      (the fp64 sum of 50,176 fp32 values adds < 1e-12)
    km   = (1-kappa) * m                     e_km  = |1-kappa| e_m + u |km|
    pre2 = fma(kappa, y1, km)                e_2   = kappa e_1 + e_km + u |pre2|
    gray = fma(.114, y2B, fma(.587, y2G, .299 y2R))      e_g = sum_d w_d e_2d + 3 u gray       (all terms >= 0)
    sg   = (1-sigma) * gray                  e_sg  = |1-sigma| e_g + u |sg|
    pre3 = fma(sigma, y2, sg)                e_3   = sigma e_2 + e_sg + u |pre3|
    pre4 = fma(R2, y3B, fma(R1, y3G, R0 y3R))            e_4 = sum_d |R_cd| e_3d + 3 u sum_d |R_cd| y3_d
    v    = (y4 - mean) / std                 e_v   = (e_4 + u |y4 - mean|) / std + u |v|
    out  = bf16(v)                           + half a bf16 ulp of a value in [|v| - e_v, |v| + e_v]
FP_SAFETY = 2 multiplies the fp32 part: it covers the second-order terms (each < 2^-20 of the first-order ones) and the reference's own fp64
rounding with a wide margin and is not tuned to any kernel.

The adjoint is linear in gout once the gates are fixed. Its chain, with a_k the same expression evaluated on absolute values (the magnitude an
fp32 rounding is relative to) and e_k the error bound:
    G4 = gout * fp32(1/std)                  e_4 = 2 u |G4|            (the rounding of 1/std and of the product)
    G3_d = sum_c R_cd G4_c                   e_3 = sum_c |R_cd| e_4c + 3 u sum_c |R_cd| |G4_c|
    G2_c = sigma G3_c + ((1-sigma) w_c) * ((G3R + G3G) + G3B)      e_2 = sigma e_3c + |1-sigma| w_c sum_d e_3d + 4 u a_2c
    s_c = fp32(fp64 sum / N)                 e_s = mean e_2c + u |s_c| + (1/N) sum over the UNCERTAIN pixels of a_2c(all gates open)
    kg = (1-kappa) s_c;  G1 = fma(kappa, G2, kg)                   e_1 = kappa e_2 + |1-kappa| e_s + u |kg| + u |G1|
    gx = bf16(G1 * std)                      e_x = e_1 std + u |gx|,   + half a bf16 ulp
A gate is NEAR when its pre-clamp value lies within GATE_MARGIN = 1e-5 of 0 or 1: the fp32 kernel and the fp64 reference may then decide
differently (the forward bounds e_1..e_4 stay below 4e-6 for |p| <= 3, asserted in the host tests). An element (pixel, channel c) is NEAR-GATE —
excluded from the adjoint comparison — unless gate 1 of c is robustly shut (then gx_c = 0 whatever the other gates do), when gate 1 of c is near,
or gate 2 of c is not robustly shut and gate 2 of c or ANY gate 3 / gate 4 of the pixel is near (saturation and hue couple the channels). A pixel
is UNCERTAIN for s_c when the second condition holds: a flipped gate there changes s_c, for every pixel of the plane, by at most a_2c / N with all
gates taken as open — the last term of e_s. Elements whose gate 1 is robustly shut have value 0 and bound 0: the kernel must write exactly 0.
"""
import numpy as np
import torch

from roboticattack_amd.constants import MEAN6, STD6

N = 224 * 224
U32 = 2.0 ** -24
FP_SAFETY = 2.0
GATE_MARGIN = 1e-5
W32 = np.array([np.float32(0.299), np.float32(0.587), np.float32(0.114)], np.float64)  # the kernels' fp32 constants, exact in fp64
HUE_T = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], np.float64)


# ---- bf16 helpers ----
def f32_to_bf16_bits(a):
    """fp32 array -> bf16 bits (uint16), round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def bits_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def half_ulp_bf16(v, e):
    """Half a bf16 ulp of any value within e of v (normal range; a floor of 2^-127 for tiny values)."""
    a = np.maximum(np.abs(v) + e, 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 8)


# ---- the factors ----
def hue_matrix(h):
    """R(h) = I + Tinv (rot(2 pi h) - I) T in fp64 (include/vaa.h)."""
    a = 2.0 * np.pi * float(h)
    c, s = np.cos(a), np.sin(a)
    d = np.array([[0.0, 0.0, 0.0], [0.0, c - 1.0, -s], [0.0, s, c - 1.0]])
    return np.eye(3) + np.linalg.inv(HUE_T) @ d @ HUE_T


def factors(delta, kappa, sigma, h):
    """One row per image, float32 [B,12] = {delta, kappa, sigma, R row-major}."""
    rows = [np.concatenate(([d, k, s], hue_matrix(hh).reshape(9))) for d, k, s, hh in zip(delta, kappa, sigma, h)]
    return np.asarray(rows, np.float64).astype(np.float32)


def _split(F):
    F = np.asarray(F, np.float32)
    delta, kappa, sigma = (F[:, k].astype(np.float64) for k in range(3))
    omk = (np.float32(1.0) - F[:, 1]).astype(np.float64)  # the kernels' fp32 differences
    oms = (np.float32(1.0) - F[:, 2]).astype(np.float64)
    return delta, kappa, sigma, omk, oms, F[:, 3:].astype(np.float64).reshape(-1, 3, 3)


def _towers(a):
    """[B,6,H,W] -> [B,2,3,H*W]"""
    return a.reshape(a.shape[0], 2, 3, -1)


def _norm(mean6, std6):
    m = np.asarray(mean6, np.float32).astype(np.float64).reshape(1, 2, 3, 1)
    s = np.asarray(std6, np.float32).astype(np.float64).reshape(1, 2, 3, 1)
    return m, s


def clamp01(a):
    return np.minimum(np.maximum(a, 0.0), 1.0)


def gate(a):
    return (a >= 0.0) & (a <= 1.0)


# ---- forward ----
def stages64(x, F, mean6=MEAN6, std6=STD6, wrong=None):
    """x float64 [B,6,224,224] -> dict of the header's intermediates, towers split ([B,2,3,N]). `wrong` names one deliberately wrong stage (the
    perturbation self-test of the bounds): "gray_mean" = K0c's single gray mean instead of one mean per channel, "hue_t" = the transposed hue
    matrix, "mul_brightness" = a multiplicative brightness."""
    delta, kappa, sigma, omk, oms, R = _split(F)
    mean, std = _norm(mean6, std6)
    b4 = lambda v: v.reshape(-1, 1, 1, 1)
    xs = _towers(np.asarray(x, np.float64))
    p = xs * std + mean
    pre1 = p * (1.0 + b4(delta)) if wrong == "mul_brightness" else p + b4(delta)
    y1 = clamp01(pre1)
    m = y1.sum(axis=3, keepdims=True) / y1.shape[3]
    if wrong == "gray_mean":
        m = np.broadcast_to((m * W32.reshape(1, 1, 3, 1)).sum(axis=2, keepdims=True), m.shape)
    m = m.astype(np.float32).astype(np.float64)  # the header rounds the mean once to fp32
    km = b4(omk) * m
    pre2 = b4(kappa) * y1 + km
    y2 = clamp01(pre2)
    gray = (y2 * W32.reshape(1, 1, 3, 1)).sum(axis=2, keepdims=True)
    sg = b4(oms) * gray
    pre3 = b4(sigma) * y2 + sg
    y3 = clamp01(pre3)
    Rm = np.swapaxes(R, 1, 2) if wrong == "hue_t" else R
    pre4 = np.einsum("bcd,btdn->btcn", Rm, y3)
    y4 = clamp01(pre4)
    v = (y4 - mean) / std
    return dict(p=p, pre1=pre1, y1=y1, m=m, km=km, pre2=pre2, y2=y2, gray=gray, sg=sg, pre3=pre3, y3=y3, pre4=pre4, y4=y4, v=v, F=(delta, kappa, sigma, omk, oms, R),
                norm=(mean, std))


def fwd64(x, F, mean6=MEAN6, std6=STD6, wrong=None):
    """-> the unrounded fp64 output [B,6,224,224]."""
    return stages64(x, F, mean6, std6, wrong)["v"].reshape(np.shape(x))


def fwd_bound(st):
    """Per-element bound of |kernel's bf16 output - st["v"]| (module docstring), [B,6,224,224]-shaped like v."""
    delta, kappa, sigma, omk, oms, R = st["F"]
    mean, std = st["norm"]
    b4 = lambda v: np.abs(v).reshape(-1, 1, 1, 1)
    u = U32
    e1 = u * np.abs(st["p"]) + u * np.abs(st["pre1"])
    em = e1.mean(axis=3, keepdims=True) + u * np.abs(st["m"])
    ekm = b4(omk) * em + u * np.abs(st["km"])
    e2 = b4(kappa) * e1 + ekm + u * np.abs(st["pre2"])
    eg = (e2 * W32.reshape(1, 1, 3, 1)).sum(axis=2, keepdims=True) + 3 * u * st["gray"]
    esg = b4(oms) * eg + u * np.abs(st["sg"])
    e3 = b4(sigma) * e2 + esg + u * np.abs(st["pre3"])
    aR = np.abs(R)
    e4 = np.einsum("bcd,btdn->btcn", aR, e3) + 3 * u * np.einsum("bcd,btdn->btcn", aR, st["y3"])
    ev = FP_SAFETY * ((e4 + u * np.abs(st["y4"] - mean)) / std + u * np.abs(st["v"]))
    pre_err = FP_SAFETY * max(float(e1.max()), float(e2.max()), float(e3.max()), float(e4.max()))
    return ev + half_ulp_bf16(st["v"], ev), pre_err


# ---- adjoint ----
def near(a):
    return (np.abs(a) <= GATE_MARGIN) | (np.abs(a - 1.0) <= GATE_MARGIN)


def shut(a):
    """robustly shut: outside [0, 1] by more than the margin (a NaN is shut in both arithmetics)."""
    return ~((a >= -GATE_MARGIN) & (a <= 1.0 + GATE_MARGIN))


def classify(st):
    """-> (near-gate elements, uncertain-for-s_c elements, gate-1-robustly-shut elements), bool [B,2,3,N] (module docstring)."""
    down = (near(st["pre3"]) | near(st["pre4"])).any(axis=2, keepdims=True)
    uncertain = ~shut(st["pre2"]) & (near(st["pre2"]) | down)
    shut1 = shut(st["pre1"])
    return ~shut1 & (near(st["pre1"]) | uncertain), uncertain, shut1


def bwd64(g, x, F, mean6=MEAN6, std6=STD6, round_s=True):
    """g, x float64 [B,6,224,224] -> (gx fp64 unrounded, per-element bound of |kernel's bf16 gx - gx|, near-gate mask, gate-1-shut mask), all
    [B,6,224,224]. round_s=False keeps s_c in fp64 (the header rounds it once to fp32): the exact derivative, for the comparison with autograd."""
    st = stages64(x, F, mean6, std6)
    delta, kappa, sigma, omk, oms, R = st["F"]
    mean, std = st["norm"]
    b4 = lambda v: v.reshape(-1, 1, 1, 1)
    w = W32.reshape(1, 1, 3, 1)
    u = U32
    near_gate, uncertain, shut1 = classify(st)
    aR = np.abs(R)
    G4 = np.asarray(g, np.float64).reshape(st["v"].shape) / std
    a4 = np.abs(G4)  # all gates open: the magnitude a flipped gate can let through
    G4 = np.where(gate(st["pre4"]), G4, 0.0)
    e4 = 2 * u * np.abs(G4)
    G3 = np.where(gate(st["pre3"]), np.einsum("bcd,btcn->btdn", R, G4), 0.0)
    e3 = np.einsum("bcd,btcn->btdn", aR, e4) + 3 * u * np.einsum("bcd,btcn->btdn", aR, np.abs(G4))
    a3 = np.einsum("bcd,btcn->btdn", aR, a4)
    G2 = np.where(gate(st["pre2"]), b4(sigma) * G3 + b4(oms) * w * G3.sum(axis=2, keepdims=True), 0.0)
    mag2 = lambda t: b4(np.abs(sigma)) * t + b4(np.abs(oms)) * w * t.sum(axis=2, keepdims=True)
    e2 = mag2(e3) + 4 * u * mag2(np.abs(G3))
    a2 = mag2(a3)
    s = G2.sum(axis=3, keepdims=True) / G2.shape[3]
    if round_s:
        s = s.astype(np.float32).astype(np.float64)
    es = e2.mean(axis=3, keepdims=True) + u * np.abs(s) + np.where(uncertain, a2, 0.0).sum(axis=3, keepdims=True) / G2.shape[3]
    kg = b4(omk) * s
    G1 = b4(kappa) * G2 + kg
    e1 = b4(np.abs(kappa)) * e2 + b4(np.abs(omk)) * es + u * np.abs(kg) + u * np.abs(G1)
    open1 = gate(st["pre1"])
    gx = np.where(open1, G1 * std, 0.0)
    ex = np.where(open1, FP_SAFETY * (e1 * std + u * np.abs(gx)), 0.0)
    bound = np.where(shut1, 0.0, ex + half_ulp_bf16(gx, ex))
    shape = np.shape(x)
    return gx.reshape(shape), bound.reshape(shape), near_gate.reshape(shape), shut1.reshape(shape)


# ---- the same forward in torch.float64 (autograd supplies the gradient) ----
def fwd_torch(x, F, mean6=MEAN6, std6=STD6):
    """x torch.float64 [B,6,H,W] (any H, W) -> out float64, differentiable. The mean is NOT rounded to fp32 here (a rounding has no derivative;
    the difference is below 1e-7 and is covered where the two are compared)."""
    F32 = torch.as_tensor(np.asarray(F, np.float32))
    Fd = F32.double()
    B = x.shape[0]
    mean = torch.tensor(np.asarray(mean6, np.float32), dtype=torch.float64).view(1, 2, 3, 1)
    std = torch.tensor(np.asarray(std6, np.float32), dtype=torch.float64).view(1, 2, 3, 1)
    w = torch.tensor(W32).view(1, 1, 3, 1)
    delta, kappa, sigma = (Fd[:, k].view(B, 1, 1, 1) for k in range(3))
    omk = (1.0 - F32[:, 1]).double().view(B, 1, 1, 1)
    oms = (1.0 - F32[:, 2]).double().view(B, 1, 1, 1)
    R = Fd[:, 3:].view(B, 3, 3)
    y1 = torch.clamp(x.reshape(B, 2, 3, -1) * std + mean + delta, 0.0, 1.0)
    y2 = torch.clamp(kappa * y1 + omk * y1.mean(dim=3, keepdim=True), 0.0, 1.0)
    y3 = torch.clamp(sigma * y2 + oms * (y2 * w).sum(dim=2, keepdim=True), 0.0, 1.0)
    y4 = torch.clamp(torch.einsum("bcd,btdn->btcn", R, y3), 0.0, 1.0)
    return ((y4 - mean) / std).reshape(x.shape)


# ---- the GPU tests' inputs (built once per process; the host tests check the near-gate share on exactly these) ----
def k1_like(u8):
    """uint8 frames [B,224,224,3] -> K1's planar pixel values as bf16 bits [B,6,224,224]: bf16((u/255 - mean)/std), both normalisations."""
    v = (u8.astype(np.float32) / np.float32(255.0)).transpose(0, 3, 1, 2)
    v = np.concatenate([v, v], axis=1)
    m = np.asarray(MEAN6, np.float32).reshape(1, 6, 1, 1)
    s = np.asarray(STD6, np.float32).reshape(1, 6, 1, 1)
    return f32_to_bf16_bits((v - m) / s)


CASES = ("generic", "constant", "saturated", "kappa0", "sigma0", "hue+0.5", "hue-0.5", "delta+1", "delta-1", "identity")
BATCHES = ((0, 3), (3, 6), (6, 9), (9, 10))  # the launches: three of B = 3 and one of B = 1
_inputs = None


def inputs():
    """-> (x bits [10,6,224,224], gout bits, factors float32 [10,12]); image k is CASES[k]."""
    global _inputs
    if _inputs is not None:
        return _inputs
    rs = np.random.RandomState(1234)
    n = len(CASES)
    u8 = rs.randint(0, 256, (n, 224, 224, 3)).astype(np.uint8)
    u8[1] = np.array([100, 150, 200], np.uint8)                                  # constant: the contrast mean equals every pixel
    u8[2] = np.where(rs.rand(224, 224, 3) < 0.5, 0, 255).astype(np.uint8)        # saturated at 0 and at 1
    for k in (7, 8):                                                             # delta = +-1: bytes 8..247, so p +- 1 leaves [0, 1] everywhere
        u8[k] = rs.randint(8, 248, (224, 224, 3)).astype(np.uint8)
    u8[9] = rs.randint(3, 253, (224, 224, 3)).astype(np.uint8)                   # identity: p inside (0, 1) ...
    idx = rs.choice(N, 100, replace=False)
    flat = u8[9].reshape(N, 3)
    flat[idx[:50]] = 0                                                           # ... except 100 pixels at the ends of the range, where the
    flat[idx[50:]] = 255                                                         #     identity factors put exact 0 / 1 on every later gate
    delta = [0.07, -0.05, -0.03, 0.04, -0.06, 0.03, -0.02, 1.0, -1.0, 0.0]
    kappa = [1.15, 0.85, 0.8, 0.0, 1.1, 0.9, 1.2, 0.9, 1.1, 1.0]
    sigma = [0.85, 1.2, 1.2, 1.1, 0.0, 1.15, 0.9, 1.1, 0.9, 1.0]
    hue = [0.04, -0.03, 0.05, 0.02, -0.05, 0.5, -0.5, 0.03, -0.04, 0.0]
    g = f32_to_bf16_bits((rs.randn(n, 6, 224, 224) * 1e-2).astype(np.float32))
    _inputs = (k1_like(u8), g, factors(delta, kappa, sigma, hue))
    return _inputs


_reference = None


def reference():
    """The fp64 reference on `inputs()`, computed once: dict(fwd, fwd_bound, pre_err, gx, gx_bound, near_gate, shut1)."""
    global _reference
    if _reference is None:
        xb, gb, F = inputs()
        x, g = bits_f32(xb).astype(np.float64), bits_f32(gb).astype(np.float64)
        st = stages64(x, F)
        fb, pre_err = fwd_bound(st)
        gx, gbound, ng, shut1 = bwd64(g, x, F)
        _reference = dict(fwd=st["v"].reshape(x.shape), fwd_bound=fb.reshape(x.shape), pre_err=pre_err, gx=gx, gx_bound=gbound, near_gate=ng, shut1=shut1)
    return _reference


def worst_ratio(got, want, bound, skip=None):
    """max over the compared elements of |got - want| / bound (0/0 = 0, x/0 = inf) and its flat index."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    if skip is not None:
        r = np.where(skip, 0.0, r)
    e = int(np.argmax(r))
    return float(r.ravel()[e]), e
