"""The forward-paste reference (tests/paste_ref.py) on its own, no GPU: against the reference's recorded goldens, its fp32 torch route against its
fp64 route over the whole case table (the bound and the caps are sound), the C oracle against it by the same classes (the oracle restates the
kernels' coordinate chain; torch does not), and the comparison functions against injected faults. Run with -s for the per-case figures."""
import os
import zlib

import numpy as np
import pytest
import torch

import paste_ref as P
from conftest import GOLDEN, golden_files
from oracle import c_oracle, ref_port
from roboticattack_amd import synthetic

K1 = list(P.K1_CASES)
K5 = list(P.K5_CASES)


def _allowed(name):
    return int(P.listed_undecided(P.k1_case(name)).sum()) if name == "identity_threshold_texels" else 0


def test_constants_and_tile_layout():
    assert np.array_equal(P.STD6, c_oracle.STD6) and np.array_equal(P.MEAN6, c_oracle.MEAN6)
    x = np.arange(2 * 6 * P.NPIX, dtype=np.int32).reshape(2, 6, P.NPIX)
    t = P.to_tiles(x)
    assert t[1, 3 * 16 + 5, 4 * 196 + 2 * 14 + 7] == x[1, 4, (3 * 14 + 2) * 224 + 5 * 14 + 7]  # tile (ty 3, tx 5), channel 4, y 2, x 7
    assert np.array_equal(P.from_tiles(t, 6), x)
    k = (np.random.RandomState(0).rand(2, 3, P.NPIX) < 0.3).astype(np.uint8)
    w = P.keep_words(k)
    assert w[1, 2, 3 * 16 + 5, 2] >> 7 & 1 == k[1, 2, (3 * 14 + 2) * 224 + 5 * 14 + 7] and np.array_equal(P.keep_from_words(w), k)


def test_torch_skips_a_corner_beyond_the_frame():
    """grid_sample's bounds mask: at the clamped position (223, 223) the east, south and south-east corners (index 224) are not read. With the
    canvas's last texel infinite the frame corner beyond the central half (everything there clamps onto that texel) comes back infinite, not NaN:
    a corner read with weight 0 would give inf * 0. The fp64 route gives such a corner nothing."""
    c = torch.zeros(3, P.IMG, P.IMG)
    c[:, -1, -1] = float("inf")
    out = P.warp32(c, P.THETAS["s2"])
    assert torch.isinf(out[:, 180:, 180:]).all() and torch.isfinite(out[:, 100, 100]).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. goldens
# ---------------------------------------------------------------------------------------------------------------------------------
def _golden_check(exps, crc, keep_bits, tag):
    B = len(exps)
    outs = [P.route32(E) for E in exps]
    bits, keep = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    assert zlib.crc32(bits.reshape(B, 6, 224, 224).view(np.int16).tobytes()) == crc, f"{tag}: the fp32 torch route is not the reference's recorded bf16 tensor"
    kb = np.unpackbits(keep_bits, axis=-1)[:, :, : P.NPIX].astype(bool)
    assert np.array_equal(kb, keep), f"{tag}: keep bits of the fp32 route"
    for b, E in enumerate(exps):
        assert np.array_equal(kb[b][E["decided"]], E["keep"][E["decided"]]), f"{tag}: image {b}: the reference's keep bits on decided elements"
    if all(E["exact"].all() and E["decided"].all() for E in exps):
        ideal = np.stack([P.ideal(E)[0] for E in exps])
        assert zlib.crc32(ideal.reshape(B, 6, 224, 224).view(np.int16).tobytes()) == crc
    return P.check_k1(exps, bits, keep, tag=tag)


@pytest.mark.parametrize("f", golden_files("k1k2_"), ids=lambda f: os.path.basename(f)[5:-4])
def test_training_path_goldens(f):
    d = np.load(f)
    B = int(d["batch"])
    imgs = synthetic.synth_images(int(d["img_seed"]), B, str(d["img_kind"]))
    mm = 1 if str(d["fn"]) == "paste_patch_fix" else 0
    exps = [P.k1_image(imgs[b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"]), mm) for b in range(B)]
    st = _golden_check(exps, int(d["bf16_crc32"]), d["keep_bits"], os.path.basename(f))
    print(f"{os.path.basename(f)}: worst err/(bound + ulp) {st.worst:.3f}, undecided {st.und}, near-midpoint {st.near} of {st.foot} footprint pixels")


@pytest.mark.parametrize("f", golden_files("resize_"), ids=lambda f: os.path.basename(f)[:-4])
def test_resized_goldens(f):
    d = np.load(f)
    B = int(d["batch"])
    imgs = synthetic.synth_images(int(d["img_seed"]), B, str(d["img_kind"]))
    patch = torch.from_numpy(d["patch"])
    exps = [P.k1_image(imgs[b], ref_port.resize_patch(patch, int(h), int(w)).numpy(), d["xy"][b], d["theta"][b], 1, 0) for b, (h, w) in enumerate(d["sizes"])]
    _golden_check(exps, int(d["bf16_crc32"]), d["keep_bits"], os.path.basename(f))


def test_k5_port_goldens():
    d = np.load(os.path.join(GOLDEN, "sim_patch.npz"))
    imgs = synthetic.synth_images(int(d["img_seed"]), len(d["crc"]), "smooth")
    out = [P.simulation_random_patch(imgs[b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"][b])) for b in range(len(imgs))]
    assert [zlib.crc32(o.tobytes()) for o in out] == [int(c) for c in d["crc"]]
    exps = [P.k5_image(imgs[b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"][b])) for b in range(len(imgs))]
    P.check_k5(exps, np.stack(out), tag="sim_patch")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the reference's two routes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K1)
def test_k1_fp32_route_inside_the_fp64_bound(name):
    d = P.k1_case(name)
    worst = 0.0
    for b, E in enumerate(d["exps"]):
        err = np.abs(E["cv32"].astype(np.float64) - E["cv"])
        assert np.all(err <= E["bcv"]), f"{name} image {b}: canvas error {err.max():.3g} outside the bound"
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.where(err == 0, 0.0, err / E["bcv"]).max()))
        assert np.array_equal(E["keep32"][E["decided"]], E["keep"][E["decided"]]), f"{name} image {b}: keep decisions on decided elements"
        oerr = np.abs(E["o32"].astype(np.float64) - E["o"])
        assert np.all(oerr <= E["bo"]), f"{name} image {b}: normalised value outside its bound"
    outs = [P.route32(E) for E in d["exps"]]
    st = P.check_k1(d["exps"], np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), tag=name)
    allowed = _allowed(name)
    if allowed:
        und = np.stack([~E["decided"] for E in d["exps"]])
        assert np.array_equal(und, P.listed_undecided(d)), "the undecided elements are not exactly the blends of on-threshold texels"
    P.check_caps(st, name, allowed)
    print(f"{name}: canvas err/bound {worst:.3f}, undecided {st.und} ({allowed} listed), near-midpoint {st.near}, footprint {st.foot}")


@pytest.mark.parametrize("name", K5)
def test_k5_fp32_route_inside_the_fp64_classes(name):
    d = P.k5_case(name)
    out = np.stack([P.simulation_random_patch(d["imgs"][b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"][b])) for b in range(d["B"])])
    st = P.check_k5(d["exps"], out, tag=name)
    P.check_caps(st, name)
    print(f"k5 {name}: allowances {st.und}, footprint {st.foot}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the C oracle against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
ORACLE_DIFF = {}


def _oracle_k1(d):
    c = d["case"]
    if d["pdesc"] is None:
        return c_oracle.patch_apply_fwd(d["imgs"], d["patch"], d["xy"], d["theta"], c.geo, c.mask)
    return c_oracle.patch_apply_fwd_multi(d["imgs"], d["packed"], d["pdesc"], d["xy"], d["theta"], c.geo, c.mask)


@pytest.mark.parametrize("name", K1)
def test_c_oracle_k1_against_the_torch_built_reference(name):
    d = P.k1_case(name)
    o32, ob, keep = _oracle_k1(d)
    st = P.check_k1(d["exps"], ob.reshape(d["B"], 6, P.NPIX), keep, tag=f"oracle {name}")
    worst, diff, n = 0.0, 0, 0
    for b, E in enumerate(d["exps"]):
        k6 = np.concatenate([keep[b], keep[b]]).astype(bool)
        o = o32[b].reshape(6, P.NPIX)
        err = np.abs(o.astype(np.float64) - E["o"])[k6]
        assert np.all(err <= E["bo"][k6]), f"oracle {name} image {b}: a kept fp32 value outside its bound"
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(err == 0, 0.0, err / E["bo"][k6]).max()))
        both = k6 & np.concatenate([E["keep32"], E["keep32"]])
        diff += int((o.view(np.uint32)[both] != E["o32"].view(np.uint32)[both]).sum())
        n += int(both.sum())
    ORACLE_DIFF[name] = (diff, n)
    tot = [sum(v[i] for v in ORACLE_DIFF.values()) for i in (0, 1)]
    print(f"oracle {name}: worst fp32 err/bound {worst:.3f}; kept values that differ in bits from torch's fp32 route: {diff} of {n} (so far {tot[0]} of {tot[1]})")


@pytest.mark.parametrize("name", K5)
def test_c_oracle_k5_against_the_torch_built_reference(name):
    d = P.k5_case(name)
    out = c_oracle.patch_apply_eval(d["imgs"], d["patch"], d["xy"], d["theta"], d["geometry"])
    P.check_k5(d["exps"], out, tag=f"oracle {name}")
    t = np.stack([P.simulation_random_patch(d["imgs"][b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"][b])) for b in range(d["B"])])
    print(f"oracle k5 {name}: bytes that differ from torch's fp32 route: {int((t != out).sum())}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. perturbation self-test: every injected fault must be flagged
# ---------------------------------------------------------------------------------------------------------------------------------
def _ideal_batch(d):
    outs = [P.ideal(E) for E in d["exps"]]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def _kept_row(E):
    """(row, first column, last column) of the middle row that holds decided kept pixels of channel 0."""
    k = (E["keep"][0] & E["decided"][0]).reshape(P.IMG, P.IMG)
    rows = np.nonzero(k.any(axis=1))[0]
    i = int(rows[len(rows) // 2])
    cols = np.nonzero(k[i])[0]
    return i, int(cols[0]), int(cols[-1])


@pytest.mark.parametrize("name", ["shipped_50_corners", "shipped_50_edge_smear", "under_one_item_15x17", "paste_lt_threshold_texels"])
def test_injected_faults_are_flagged(name):
    d = P.k1_case(name)
    bits, keep = _ideal_batch(d)
    P.check_k1(d["exps"], bits, keep, tag="ideal")
    P.check_k1(d["exps"], bits, None, tag="ideal, no keep buffer")
    E = d["exps"][0]
    i, j0, j1 = _kept_row(E)

    def flagged(b2, k2, what, word=None):
        for kk in (k2, None):
            with pytest.raises(AssertionError) as ei:
                P.check_k1(d["exps"], b2, kk, tag=what)
            if word and kk is not None:
                assert word in str(ei.value), str(ei.value)

    # a footprint item (16 aligned pixels) left as camera pixels
    b2, k2 = bits.copy(), keep.copy()
    it = (j0 + j1) // 2 // 16 * 16
    sl = slice(i * P.IMG + it, i * P.IMG + it + 16)
    b2[0, :, sl], k2[0, :, sl] = E["cam"][:, sl], False
    flagged(b2, k2, "item left as camera pixels", "COMPLETENESS")
    # one row's span shortened by one pixel
    b2, k2 = bits.copy(), keep.copy()
    p = i * P.IMG + j1
    b2[0, :, p], k2[0, :, p] = E["cam"][:, p], False
    flagged(b2, k2, "span shortened by one pixel", "COMPLETENESS")
    # the keep mask shifted by one pixel (values untouched)
    with pytest.raises(AssertionError):
        P.check_k1(d["exps"], bits, np.roll(keep, 1, axis=2), tag="keep mask shifted")
    # values sampled one pixel off
    with pytest.raises(AssertionError):
        P.check_k1(d["exps"], np.roll(bits, 1, axis=2), keep, tag="values shifted")
    # one tile's flag cleared / set
    t0, t1 = P.to_tiles(bits[:, :3]), P.to_tiles(bits[:, 3:])
    words, flags = P.keep_words(keep), P.tile_any(keep).astype(np.uint32)
    P.check_tiles(d["exps"], t0, t1, words, flags, tag="ideal tiles")
    f2 = flags.copy()
    f2[0, int(np.nonzero(flags[0])[0][0])] = 0
    with pytest.raises(AssertionError, match="tile flag"):
        P.check_tiles(d["exps"], t0, t1, words, f2, tag="flag cleared")
    f2 = flags.copy()
    f2[0, int(np.nonzero(flags[0] == 0)[0][0])] = 1
    with pytest.raises(AssertionError, match="tile flag"):
        P.check_tiles(d["exps"], t0, t1, words, f2, tag="flag set")


def test_a_paste_without_the_border_clamp_is_flagged():
    """A corner beyond the frame given -100 instead of torch's value (the border texel): the smear of a patch on the frame edge disappears."""
    d = P.k1_case("shipped_50_edge_smear")
    c = d["case"]
    for b in range(4):  # the four scale-2 placements on an edge or a corner
        F_ = P.k1_image(d["imgs"][b], d["patch"], d["xy"][b], d["theta"][b], c.geo, c.mask, fault="no_border")
        bits, keep = P.ideal(F_)
        with pytest.raises(AssertionError, match="COMPLETENESS"):
            P.check_k1([d["exps"][b]], bits[None], keep[None], tag="no border clamp")
        with pytest.raises(AssertionError):
            P.check_k1([d["exps"][b]], bits[None], None, tag="no border clamp")


def test_k5_rounded_bytes_and_a_touched_background_are_flagged():
    d = P.k5_case("mixed_flags_50_smooth")
    ideal = np.stack([P.simulation_random_patch(d["imgs"][b], d["patch"], d["xy"][b], d["theta"][b], int(d["geometry"][b])) for b in range(d["B"])])
    P.check_k5(d["exps"], ideal, tag="ideal")
    E = d["exps"][0]
    r = np.where(E["cv"] >= 0, np.clip(np.rint(E["cv"]), 0, 255), E["frame"]).T.reshape(P.IMG, P.IMG, 3).astype(np.uint8)
    bad = ideal.copy()
    bad[0] = r
    with pytest.raises(AssertionError, match="outside their class"):
        P.check_k5(d["exps"], bad, tag="rounded")
    q = P.k5_case("truncation_texels_b3")  # the quantisation of the patch rounded instead of truncated
    rq = np.stack([P.simulation_random_patch(q["imgs"][b], (np.rint(q["patch"] * 255.0) + 0.25) / 255.0, q["xy"][b], q["theta"][b], 0) for b in range(q["B"])])
    with pytest.raises(AssertionError, match="outside their class"):
        P.check_k5(q["exps"], rq, tag="patch rounded")
    bad = ideal.copy()
    bad[1, 200, 200, 1] ^= 1  # image 1: un-warped paste in the top-left corner; (200, 200) is background
    with pytest.raises(AssertionError, match="changed set"):
        P.check_k5(d["exps"], bad, tag="background touched")
