"""The fp64 patch-gradient reference (tests/patch_grad_ref.py) against independent CPU computations, and its bounds against injected faults.
No GPU: what the GPU tests of test_gpu_patch_grad_ref.py compare the kernels with is checked here on its own, for every case, no element excluded."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_grad_ref as R
from oracle import c_oracle

K2 = sorted(R.K2_CASES)
K2E = sorted(R.K2E_CASES)


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_constants_are_the_oracles():
    assert np.array_equal(R.STD6, c_oracle.STD6) and np.array_equal(R.MEAN6, c_oracle.MEAN6)


def test_grid_equals_torch_affine_grid_bit_for_bit():
    """Every theta of every case (and a seeded sweep of rotation / shear draws): base @ theta^T in fp32 is torch's own, bit for bit."""
    ths = [R.case_inputs(f, n)["theta"] for f in ("k2", "k2e") for n in R.CASES[f]]
    ths.append(R.placements(64, [(50, 50)] * 64, 5)[1])
    th = np.unique(np.concatenate(ths).reshape(-1, 6), axis=0)
    want = F.affine_grid(torch.from_numpy(th).view(-1, 2, 3), [len(th), 1, R.IMG, R.IMG], align_corners=False).numpy()
    for k, t in enumerate(th):
        gx, gy = R.grid32(t)
        assert np.array_equal(gx.view(np.uint32), want[k, :, :, 0].view(np.uint32)), t
        assert np.array_equal(gy.view(np.uint32), want[k, :, :, 1].view(np.uint32)), t


def test_fma32_is_correctly_rounded_where_the_plain_form_is_not():
    """a * b = 2^-14 (1 - 2^-46) exactly, c = 1024 + 2^-13 (odd last bit; fp32 spacing 2^-13): the true sum lies 2^-60 BELOW the midpoint
    c + 2^-14 and rounds to c. The plain fp64 expression rounds the sum onto the midpoint first and then to even, one ulp too high."""
    a, b, c = np.float32(2.0 ** -14 * (1 + 2.0 ** -23)), np.float32(1 - 2.0 ** -23), np.float32(1024 + 2.0 ** -13)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1024 + 2.0 ** -12)
    assert R.fma32(a, b, c) == c
    assert R.fma32(-a, b, -c) == -c
    rs = np.random.RandomState(0)  # and it agrees with the plain form where that is exact
    x, y, z = (rs.standard_normal(1000).astype(np.float32) for _ in range(3))
    assert np.array_equal(R.fma32(x, y, z), (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32))


def _k2_case(name):
    d = R.case_inputs("k2", name)
    return d, d["case"], R.case_ref("k2", name)


def _oracle_grad(d, f64):
    c = d["case"]
    g = _bits(d["g"])
    if d["pdesc"] is None:
        return c_oracle.patch_grad(g, d["patch"], d["xy"], d["theta"], c.geo, c.mask, f64=f64).ravel()
    out = np.zeros(len(d["patch"]), np.float32)
    for b, (h, w, off, _z) in enumerate(d["pdesc"]):  # the oracle's per-image form is its single-patch routine, image by image
        out[off : off + 3 * h * w] = c_oracle.patch_grad(g[b : b + 1], d["patch"][off : off + 3 * h * w].reshape(3, h, w), d["xy"][b : b + 1],
                                                         d["theta"][b : b + 1], c.geo, c.mask, f64=f64).ravel()
    return out


@pytest.mark.parametrize("name", K2)
def test_k2_oracle_routes_inside_the_bound(name):
    """The C oracle forms the same fp32 products. Its fp64-accumulated route must lie inside the K2 bound at every element; its fp32 route
    inside the bound plus its own summation term: an image's n_e contributions are added in scan order in fp32, then the B image sums —
    (n_e + B) u S_e (the standard recursive-summation bound, with the same safety factor)."""
    d, c, ref = _k2_case(name)
    assert ref.meta["cnt"].max() > 0
    assert np.all(ref.bound[ref.meta["cnt"] == 0] == 0) and np.all(ref.value[ref.meta["cnt"] == 0] == 0)
    r64 = R.compare(ref, _oracle_grad(d, True), f"oracle f64 {name}")
    scan = R.SAFETY * (ref.meta["cnt"] + c.B) * R.U * ref.meta["S"]
    r32 = R.compare(R.Ref(ref.value, ref.bound + scan, ref.meta), _oracle_grad(d, False), f"oracle f32 {name}")
    print(f"k2 {name}: oracle f64 {r64:.3f}, f32 {r32:.3f} of the bound")


def _box3(x, sz):
    """Sum over the 3x3 texel neighbourhood, per image and channel plane of the (packed) layout."""
    out = np.zeros_like(x)
    for (h, w, off) in {tuple(int(v) for v in r) for r in sz}:
        p = np.pad(x[off : off + 3 * h * w].reshape(3, h, w), ((0, 0), (1, 1), (1, 1)))
        out[off : off + 3 * h * w] = sum(p[:, a : a + h, b : b + w] for a in range(3) for b in range(3)).ravel()
    return out


def _torch_conv_chain(d, keep):
    """float64 autograd through paste -> warp -> fixed mask -> both normalisations -> F.conv2d(x, W[D,3,14,14], stride=14) of both towers,
    upstream gradient on the conv outputs (the formulation of test_patch_embed_grad_gather_vs_torch_conv_autograd)."""
    c = d["case"]
    p = torch.from_numpy(d["patch"]).double().requires_grad_(True)
    mean, std = torch.from_numpy(R.MEAN6).double(), torch.from_numpy(R.STD6).double()
    xs = []
    for b in range(c.B):
        h, w = (int(v) for v in d["sizes"][b])
        pb = p if d["pdesc"] is None else p[int(d["pdesc"][b][2]) :][: 3 * h * w].view(3, h, w)
        x, y = (int(v) for v in d["xy"][b])
        canvas = torch.full((3, R.IMG, R.IMG), -100.0, dtype=torch.float64)
        canvas[:, y : y + h, x : x + w] = pb
        if c.geo:
            grid = F.affine_grid(torch.from_numpy(d["theta"][b]).double()[None], [1, 3, R.IMG, R.IMG], align_corners=False)
            canvas = F.grid_sample(canvas[None], grid, align_corners=False, padding_mode="border")[0]
        im = torch.from_numpy(d["imgs"][b]).permute(2, 0, 1).double() / 255
        v = torch.where(torch.from_numpy(keep[b].reshape(3, R.IMG, R.IMG) != 0), canvas, im)
        xs.append(torch.cat([(v - mean[:3, None, None]) / std[:3, None, None], (v - mean[3:, None, None]) / std[3:, None, None]]))
    X = torch.stack(xs)
    outs, grads = [], []
    for k in range(2):
        D = d["w"][k].shape[0]
        outs.append(F.conv2d(X[:, 3 * k : 3 * k + 3], d["w"][k].double().view(D, 3, 14, 14), stride=14))
        grads.append(d["dy"][k].double().transpose(1, 2).reshape(c.B, D, 16, 16))  # token t = ty*16 + tx
    torch.autograd.backward(outs, grads)
    return p.grad.numpy().ravel()


@pytest.mark.parametrize("name", K2E)
def test_k2e_reference_vs_torch_float64_conv_autograd(name):
    """The K2' reference (unrounded form) against torch float64 autograd with the mask held fixed. Pins the (c, y, x) column order, the token order
    and the tower / channel split independently of the project's code. The two differ in the precision of the sample coordinates only:
    torch forms them in fp64 here, the reference in fp32 as the kernels do. fp32 error of a position: the base coordinate carries 3
    roundings of values <= 1 (3u); g = bx th0 + by th1 + th2 adds 3 roundings and passes the base errors on: <= 6 u M, M = |th0| + |th1| +
    |th2|; fl(g + 1) adds u (M + 1); times 112, plus the rounding of a position of at most 225:  ec = 112 u (7 M + 1) + 225 u.
    A corner weight is hat(ix - u) hat(iy - v) of the clamped position (1-Lipschitz in each, at most 1), so a contribution changes by at
    most 2 ec |G| and reaches only texels within one of the pixel's fp32 corners: 2 ec x (3x3 neighbourhood sum of R), R = sum of A over
    the pixels with a corner on the texel. fp64 summation on both sides: 2^-40 S covers a few thousand terms at 2^-53."""
    d = R.case_inputs("k2e", name)
    ref = R.case_ref("k2e", name, round_bf16=False)
    got = _torch_conv_chain(d, R.oracle_keep(d))
    M = np.abs(d["theta"]).sum(axis=(1, 2)).max() if d["case"].geo else 0.0
    ec = (112 * R.U * (7 * M + 1) + 225 * R.U) if d["case"].geo else 0.0
    bound = 2 * ec * _box3(ref.meta["R"], ref.meta["sz"]) + 2.0 ** -40 * ref.meta["S"]
    worst = R.compare(R.Ref(ref.value, bound, ref.meta), got, f"torch f64 {name}")
    print(f"k2e {name}: torch float64 chain at {worst:.3f} of the coordinate bound (ec = {ec:.2e})")
    assert np.abs(ref.value).max() > 0


@pytest.mark.parametrize("name", sorted(R.K0_CASES))
def test_k0_adjoint_reference(name):
    ref, gy, pdesc = R.case_ref("k0", name)
    ph, pw, _sizes = R.K0_CASES[name]
    # <A x, gy> == <x, A^T gy> in fp64
    x = torch.rand(1, 3, ph, pw, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    lhs = sum(float((R._aa(x, int(h), int(w))[0] * torch.from_numpy(gy[off : off + 3 * h * w]).double().view(3, int(h), int(w))).sum()) for (h, w, off, _z) in pdesc)
    rhs = float((x.numpy().ravel() * ref.value).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    worst = R.compare(ref, c_oracle.patch_resize_bwd(gy.astype(np.float32), pdesc, ph, pw), f"oracle resize_bwd {name}")
    print(f"k0 {name}: oracle at {worst:.3f} of the bound")


FAULTS = ["drop", "shift_x", "shift_y", "transpose", "swap_std", "zero_tile", "lose_row", "twice"]


def _reject(ref, got, tag):
    with pytest.raises(AssertionError, match="band"):
        R.compare(ref, got.astype(np.float32), tag)


def _self_test(ref, c, tag, bf16=False):
    base = ref.value.astype(np.float32)
    assert R.compare(ref, base, tag) <= 1.0  # the un-faulted result is in bound
    at = R.median_pixel(ref)
    img = int(ref.meta["rec"]["b"][at])
    br = ref.meta["band_rows"]
    h = int(ref.meta["sz"][img][0])
    # first row of the band the faulted pixel's texel lies in (of band 1 where the patch has one and the texel allows it)
    v = int(np.clip(ref.meta["rec"]["y0"][at] - ref.meta["xy"][img][1], 0, h - 1))
    row = (v // br) * br
    for kind in FAULTS:
        if kind == "transpose" and not c.geo:
            continue  # the un-warped paste forms no fractions (w = n = 0 in the kernel): there is no pair of weights to transpose
        _reject(ref, R.faulted(ref, kind, at=at, image=img, row=row), f"{tag} fault {kind}")
    if bf16:
        # Two bf16 ulps of ONE tile pixel against the sum over a batch cannot stand out of a per-element bound: a texel of the summed gradient
        # collects hundreds of tile pixels, some of them within the MFMA accumulation error of a bf16 rounding midpoint and so uncertain by an
        # ulp each. The finest result the kernels expose is the per-image one (the per-image forms; the partial tiles of a deferred reduce),
        # which the GPU tests compare as well: the fault is injected there.
        fine = ref if c.sizes else R.per_image(ref)
        assert R.compare(fine, fine.value.astype(np.float32), tag) <= 1.0
        _reject(fine, R.faulted(fine, "bf16_2ulp", at=R.bf16_fault_pixel(fine)), f"{tag} fault bf16_2ulp")


@pytest.mark.parametrize("name", K2)
def test_k2_bound_rejects_single_faults(name):
    """One defect at a time in an otherwise exact result, at a pixel whose |G| is the batch MEDIAN: a bound that lets one through is too loose."""
    d, c, ref = _k2_case(name)
    _self_test(ref, c, f"k2 {name}")


@pytest.mark.parametrize("name", K2E)
@pytest.mark.parametrize("rb", [True, False], ids=["bf16", "f32"])
def test_k2e_bound_rejects_single_faults(name, rb):
    ref = R.case_ref("k2e", name, round_bf16=rb)
    _self_test(ref, R.K2E_CASES[name], f"k2e {name} rb={rb}", bf16=rb)


def test_compare_names_texel_channel_image_and_band():
    ref = R.case_ref("k2", "multi")
    got = ref.value.copy()
    h, w, off = (int(v) for v in ref.meta["sz"][1])
    e = off + 2 * h * w + 20 * w + 3
    got[e] += 1.0
    with pytest.raises(AssertionError, match=r"channel 2 texel \(row 20, col 3\) image 1 \(61x61\), band 1 \(rows 16..31\)"):
        R.compare(ref, got, "named")
