"""GPU tests of the forward paste kernels (K1: vaa_patch_apply_fwd, _tiles, _multi; K5: vaa_patch_apply_eval) against tests/paste_ref.py, the
reference built from torch's own CPU ops (its docstring derives the bound and the element classes). Every case of paste_ref.K1_CASES /
K5_CASES runs through the raw C entry points on guarded, pre-filled outputs: every element must be written, by class; completeness (a decided
kept pixel must be kept) is reported on its own; a second call must give the same bits. Run with -s for the per-case figures."""
import numpy as np
import pytest
import torch

import paste_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD, CANARY = 256, 0x7B
SENTINEL = 0x7FC1  # a NaN: no normalised value has these bf16 bits

WORST = {}  # form -> (worst error / (bound + ulp), undecided, near-midpoint) over the session


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """n elements of `dtype` pre-filled with `fill` (an integer bit pattern) between two canaries."""

    def __init__(self, n, dtype, fill):
        size = torch.empty((), dtype=dtype).element_size()
        self.flat = torch.full((n * size + 2 * PAD,), CANARY, dtype=torch.uint8, device=DEV)
        self.view = self.flat[PAD : PAD + n * size].view(dtype)
        self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self, what):
        torch.cuda.synchronize()
        f = self.flat.cpu().numpy()
        assert (f[:PAD] == CANARY).all() and (f[-PAD:] == CANARY).all(), f"{what}: bytes written outside the output"
        return self.view.cpu().numpy()


def _inputs(d, reps=None):
    """Device inputs of a case; reps: the images repeated cyclically to that batch size -> (args, idx)."""
    B = d["B"] if reps is None else reps
    idx = [b % d["B"] for b in range(B)]
    a = dict(B=B, imgs=_t(d["imgs"][idx]), xy=_t(d["xy"][idx], torch.int32), th=_t(d["theta"][idx].reshape(-1, 6)))
    if d.get("pdesc") is not None:
        a["patch"], a["pdesc"], (a["ph"], a["pw"]) = _t(d["packed"]), _t(d["pdesc"][idx]), d["max_hw"]
    else:
        a["patch"], a["pdesc"], a["ph"], a["pw"] = _t(d["patch"]), None, int(d["patch"].shape[1]), int(d["patch"].shape[2])
    return a, idx


def _consts():
    from roboticattack_amd import _lib

    return _lib, _lib.lib(), _lib.f32x(P.MEAN6), _lib.f32x(P.STD6)


def _planar(a, c, want_keep):
    """vaa_patch_apply_fwd / _multi on guarded buffers -> (bits uint16 [B,6,NPIX], keep 0/1 [B,3,NPIX] or None)."""
    _lib, L, mean, std = _consts()
    B = a["B"]
    out = Guarded(B * 6 * P.NPIX, torch.int16, SENTINEL)
    keep = Guarded(B * 3 * P.NPIX // 8, torch.uint8, 0xFF) if want_keep else None
    kp = keep.ptr() if want_keep else None
    if a["pdesc"] is None:
        rc = L.vaa_patch_apply_fwd(a["imgs"].data_ptr(), a["patch"].data_ptr(), a["xy"].data_ptr(), a["th"].data_ptr(), B, a["ph"], a["pw"], c.geo, c.mask,
                                   mean, std, out.ptr(), kp, _stream())
    else:
        rc = L.vaa_patch_apply_fwd_multi(a["imgs"].data_ptr(), a["patch"].data_ptr(), a["pdesc"].data_ptr(), a["xy"].data_ptr(), a["th"].data_ptr(), B,
                                         a["ph"], a["pw"], c.geo, c.mask, mean, std, out.ptr(), kp, _stream())
    _lib.check(rc, "vaa_patch_apply_fwd")
    bits = out.numpy("out").view(np.uint16).reshape(B, 6, P.NPIX)
    assert not (bits == SENTINEL).any(), f"{int((bits == SENTINEL).sum())} output elements were never written"
    k = np.unpackbits(keep.numpy("keep").reshape(B, 3, -1), axis=-1, bitorder="little") if want_keep else None
    return bits, k


def _tiles(a, c):
    _lib, L, mean, std = _consts()
    B = a["B"]
    o0, o1 = Guarded(B * 256 * 588, torch.int16, SENTINEL), Guarded(B * 256 * 588, torch.int16, SENTINEL)
    kt, fl = Guarded(B * 3 * 256 * 14, torch.int16, -1), Guarded(B * 256, torch.int32, -1)
    rc = L.vaa_patch_apply_fwd_tiles(a["imgs"].data_ptr(), a["patch"].data_ptr(), a["pdesc"].data_ptr() if a["pdesc"] is not None else None,
                                     a["xy"].data_ptr(), a["th"].data_ptr(), B, a["ph"], a["pw"], c.geo, c.mask, mean, std, o0.ptr(), o1.ptr(), kt.ptr(),
                                     fl.ptr(), _stream())
    _lib.check(rc, "vaa_patch_apply_fwd_tiles")
    r = [o0.numpy("out0").view(np.uint16).reshape(B, 256, 588), o1.numpy("out1").view(np.uint16).reshape(B, 256, 588),
         kt.numpy("keep_t").view(np.uint16).reshape(B, 3, 256, 14), fl.numpy("flags").view(np.uint32).reshape(B, 256)]
    assert not (r[0] == SENTINEL).any() and not (r[1] == SENTINEL).any(), "tile-major output elements were never written"
    return r


def _note(form, name, st, allowed=0):
    w = WORST.get(form, (0.0, 0, 0))
    WORST[form] = (max(w[0], st.worst), w[1] + st.und, w[2] + st.near)
    print(f"{form} {name}: worst err/(bound + ulp) {st.worst:.3f}, undecided {st.und} ({allowed} listed), near-midpoint {st.near}, footprint {st.foot} pixels, "
          f"decided kept elements missed {st.missing}; session {({k: (float(f'{v[0]:.3g}'), v[1], v[2]) for k, v in sorted(WORST.items())})}")


def _allowed(name, d):
    return int(P.listed_undecided(d).sum()) if name == "identity_threshold_texels" else 0


@pytest.mark.parametrize("name", list(P.K1_CASES))
def test_k1_planar_and_per_image_forms(ops, name):
    """vaa_patch_apply_fwd (vaa_patch_apply_fwd_multi for the per-image-size cases), with and without a keep buffer."""
    d = P.k1_case(name)
    c = d["case"]
    form = "K1 multi" if d["pdesc"] is not None else "K1 planar"
    for reps in (None,) + tuple(c.reps[:1]):  # reps[0]: the batch size beyond which the planar launcher halves fsplit
        a, idx = _inputs(d, reps)
        bits, keep = _planar(a, c, True)
        st = P.check_k1(d["exps"], bits, keep, idx, f"{form} {name} B={a['B']}")
        P.check_caps(st, name, _allowed(name, d))
        _note(form, f"{name} B={a['B']}", st, _allowed(name, d))
        bits_nk, _ = _planar(a, c, False)
        assert np.array_equal(bits_nk, bits), "the values depend on whether a keep buffer is given"
        P.check_k1(d["exps"], bits_nk, None, idx, f"{form} {name} without keep")
        bits2, keep2 = _planar(a, c, True)
        assert np.array_equal(bits2, bits) and np.array_equal(keep2, keep), "a second call gave different bits"


@pytest.mark.parametrize("name", list(P.K1_CASES))
def test_k1_tile_major_form(ops, name):
    """vaa_patch_apply_fwd_tiles: out0 / out1, keep words and tile flags."""
    d = P.k1_case(name)
    c = d["case"]
    for reps in (None,) + tuple(c.reps[1:2]):  # reps[1]: the batch size beyond which the tile-major launcher halves fsplit
        a, idx = _inputs(d, reps)
        o0, o1, kt, fl = _tiles(a, c)
        st = P.check_tiles(d["exps"], o0, o1, kt, fl, idx, f"K1 tiles {name} B={a['B']}")
        P.check_caps(st, name, _allowed(name, d))
        _note("K1 tiles", f"{name} B={a['B']}", st, _allowed(name, d))
        # the derived tile-major expectations, where the reference leaves no choice
        if all(E["decided"].all() and E["exact"][np.concatenate([E["keep"], E["keep"]])].all() for E in d["exps"]):
            ideal = [P.ideal(d["exps"][i]) for i in idx]
            bits, keep = np.stack([x[0] for x in ideal]), np.stack([x[1] for x in ideal])
            assert np.array_equal(o0, P.to_tiles(bits[:, :3])) and np.array_equal(o1, P.to_tiles(bits[:, 3:]))
            assert np.array_equal(kt, P.keep_words(keep)) and np.array_equal(fl != 0, P.tile_any(keep))
        again = _tiles(a, c)
        assert all(np.array_equal(x, y) for x, y in zip((o0, o1, kt, fl), again)), "a second call gave different bits"
        bits_p, keep_p = _planar(a, c, True)  # and the two forms agree with each other
        assert np.array_equal(P.from_tiles(np.concatenate([o0, o1], axis=2), 6), bits_p) and np.array_equal(P.keep_from_words(kt), keep_p)


@pytest.mark.parametrize("name", list(P.K5_CASES))
def test_k5_eval_paste(ops, name):
    """vaa_patch_apply_eval: bytes by class; every byte outside the reference's changed set equals the input frame."""
    d = P.k5_case(name)
    _lib, L, _m, _s = _consts()
    B = d["B"]
    imgs, patch, xy, th, geo = _t(d["imgs"]), _t(d["patch"]), _t(d["xy"], torch.int32), _t(d["theta"].reshape(-1, 6)), _t(d["geometry"], torch.int32)
    outs = []
    for _rep in range(2):
        out = Guarded(B * P.NPIX * 3, torch.uint8, 0xA5)
        _lib.check(L.vaa_patch_apply_eval(imgs.data_ptr(), patch.data_ptr(), xy.data_ptr(), th.data_ptr(), geo.data_ptr(), B, d["case"].h, d["case"].w,
                                          out.ptr(), _stream()), "vaa_patch_apply_eval")
        outs.append(out.numpy("out").reshape(B, P.IMG, P.IMG, 3))
    st = P.check_k5(d["exps"], outs[0], tag=f"K5 {name}")
    P.check_caps(st, name)
    assert np.array_equal(outs[0], outs[1]), "a second call gave different bytes"
    got = ops.patch_apply_eval(imgs, patch, xy, th, geo).cpu().numpy()
    assert np.array_equal(got, outs[0])
    print(f"K5 {name}: +-1 byte / either-source allowances {st.und} of {st.foot} footprint pixels")
