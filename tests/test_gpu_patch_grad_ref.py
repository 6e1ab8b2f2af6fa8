"""GPU tests of the patch-gradient kernels (K2, K2', the K0 adjoint) against tests/patch_grad_ref.py: the fp64 reference with a bound per
output element (its docstring derives the terms). Every kernel form the launcher can select (grad_sched, band_rows_for, launch_scatter_reduce,
launch_scatter_multi, launch_embed_tiles in csrc/vaa_patch_grad.hip) has a case in patch_grad_ref.CASES whose comment names the launcher
condition that selects it; every result goes through patch_grad_ref.compare, element by element. The keep mask is K1's, asserted equal to
the C oracle's bits (pinned to the reference goldens) before it is used.
Out of scope here (test_gpu_kernels.py keeps them): non-finite gradients, the 2^40 scale range, the 16,000-image flush, bitwise repeatability."""
import numpy as np
import pytest
import torch

import patch_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

WORST = {}  # form -> worst error / bound seen in this session (printed by the tests: pytest -s)


@pytest.fixture(scope="module")
def ops():
    from roboticattack_amd import ops as _ops

    _ops.device_check()
    return _ops


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _compare(ref, got, form, tag):
    torch.cuda.synchronize()
    r = R.compare(ref, got, f"{form} {tag}")
    WORST[form] = max(WORST.get(form, 0.0), r)
    return r


def _report():
    print("worst error / bound so far:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})


def _keep_unpack(keep_bits):
    return np.unpackbits(keep_bits.cpu().numpy(), axis=-1, bitorder="little")


def _keep_words(keep01, B):
    """0/1 [B,3,50176] -> the tile-major words [B,3,256,14] (bit x of word (c, tile, y))."""
    bits = keep01.reshape(B, 3, 16, 14, 16, 14)  # [b,c,ty,y,tx,x]
    w = (bits.astype(np.uint32) << np.arange(14, dtype=np.uint32)).sum(axis=5)
    return w.transpose(0, 1, 2, 4, 3).reshape(B, 3, 256, 14).astype(np.uint16)


def _placed(d):
    c = d["case"]
    a = dict(imgs=_t(d["imgs"]), patch=_t(d["patch"]), xy=_t(d["xy"], torch.int32), th=_t(d["theta"].reshape(-1, 6)), geo=bool(c.geo), mask=c.mask)
    if d["pdesc"] is not None:
        a["pdesc"] = _t(d["pdesc"])
        a["mh"] = (int(d["sizes"][:, 0].max()), int(d["sizes"][:, 1].max()))
    return a


def _k1_keep(ops, d, a):
    """K1's keep bits, equal to the oracle's."""
    if d["pdesc"] is None:
        _, keep = ops.patch_apply_fwd(a["imgs"], a["patch"], a["xy"], a["th"], a["geo"], a["mask"])
    else:
        _, keep = ops.patch_apply_fwd_multi(a["imgs"], a["patch"], a["pdesc"], a["mh"], a["xy"], a["th"], a["geo"], a["mask"])
    assert np.array_equal(_keep_unpack(keep), R.oracle_keep(d)), "K1's keep bits differ from the oracle's"
    return keep


@pytest.mark.parametrize("name", sorted(R.K2_CASES))
def test_k2_every_form_vs_fp64_reference(ops, name):
    """vaa_patch_grad_gather[_multi], stored mask and keep_bits=None (the mask re-derived from the patch must be the same mask)."""
    d = R.case_inputs("k2", name)
    ref = R.case_ref("k2", name)
    a = _placed(d)
    keep = _k1_keep(ops, d, a)
    g = d["g"].to(DEV)
    for kp, mk in ((keep, "stored"), (None, "rederived")):
        if d["pdesc"] is None:
            got = ops.patch_grad_gather(g, a["patch"], a["xy"], a["th"], kp, a["geo"], a["mask"])
            form = "K2 3ch" if 3 * d["case"].ph * d["case"].pw * 8 <= 65536 else "K2 1ch"
        else:
            got = ops.patch_grad_gather_multi(g, a["patch"], a["pdesc"], a["mh"], a["xy"], a["th"], kp, a["geo"], a["mask"])
            form = "K2 multi"
        _compare(ref, got, form, f"{name} mask {mk}")
    _report()


def _k2e_inputs(ops, d):
    dy = [t.to(DEV) for t in d["dy"]]
    wp = [ops.pack_embed_weights(w.t().contiguous().to(DEV)) for w in d["w"]]  # W^T [588,D]
    return dy, wp


def _run_k2e(ops, name, f32_pairs=False):
    d = R.case_inputs("k2e", name)
    a = _placed(d)
    c = d["case"]
    keep = _k1_keep(ops, d, a)
    dy, wp = _k2e_inputs(ops, d)
    multi = d["pdesc"] is not None
    kw = dict(pdesc=a["pdesc"], max_hw=a["mh"]) if multi else {}
    _o0, _o1, keep_t, flags = ops.patch_apply_fwd_tiles(a["imgs"], a["patch"], a["xy"], a["th"], a["geo"], a["mask"], **kw)
    want = R.oracle_keep(d)
    assert np.array_equal(keep_t.cpu().numpy().view(np.uint16), _keep_words(want, c.B)), "K1's tile-major keep words differ from the oracle's bits"
    assert np.array_equal(flags.cpu().numpy() != 0, R.kept_tiles(want))
    Dmax = max(c.D0, c.D1)
    kern = "global" if 64 * (Dmax + 8) * 2 > 150 * 1024 else "lds"
    for rb in (True, False):
        ref = R.case_ref("k2e", name, round_bf16=rb)
        form = f"K2' {kern} {'bf16' if rb else 'f32'}{' f32pairs' if f32_pairs else ''}{' multi' if multi else ''}"
        if multi:
            got_p = ops.patch_embed_grad_gather_multi(dy[0], dy[1], wp[0], wp[1], a["patch"], a["pdesc"], a["mh"], a["xy"], a["th"], keep, a["geo"], a["mask"], round_bf16=rb)
            got_t = ops.patch_embed_grad_gather_multi_tiles(dy[0], dy[1], wp[0], wp[1], a["patch"], a["pdesc"], a["mh"], a["xy"], a["th"], keep_t, flags, a["geo"],
                                                            a["mask"], round_bf16=rb)
        else:
            got_p = ops.patch_embed_grad_gather(dy[0], dy[1], wp[0], wp[1], a["patch"], a["xy"], a["th"], keep, a["geo"], a["mask"], round_bf16=rb)
            got_t = ops.patch_embed_grad_gather_tiles(dy[0], dy[1], wp[0], wp[1], a["patch"], a["xy"], a["th"], keep_t, flags, a["geo"], a["mask"], round_bf16=rb)
        _compare(ref, got_p, form, f"{name} planar mask")
        _compare(ref, got_t, form, f"{name} tile-major mask")
        if not multi:  # defer_reduce: the partial tiles, summed here in fp64 (the final fp32 rounding is then absent)
            parts = ops.patch_embed_grad_gather_tiles(dy[0], dy[1], wp[0], wp[1], a["patch"], a["xy"], a["th"], keep_t, flags, a["geo"], a["mask"], round_bf16=rb,
                                                      defer_reduce=True)
            torch.cuda.synchronize()
            _compare(ref, parts.double().sum(dim=0), form + " deferred", f"{name} defer_reduce")
            # B < 512: partial tile p is image p's own gradient — each against the per-image reference (a few contributions per texel)
            assert parts.shape[0] == c.B
            _compare(R.per_image(ref), parts, form + " per image", f"{name} partial tiles")
    _report()


@pytest.mark.parametrize("name", sorted(R.K2E_CASES))
def test_k2e_every_form_vs_fp64_reference(ops, name):
    """vaa_patch_embed_grad_gather{,_tiles,_multi,_multi_tiles}: round_bf16 on and off, planar and tile-major mask, defer_reduce."""
    _run_k2e(ops, name)


@pytest.mark.parametrize("name", ["split_nb1", "split_nb3"])
def test_k2e_f32_pairs_switch_vs_fp64_reference(ops, monkeypatch, name):
    """VAA_K2E_F32_PAIRS=1: the split tile kernel leaves fp32 {tower 0, tower 1} pairs instead of two bf16 planes; same arithmetic, same bound."""
    monkeypatch.setenv("VAA_K2E_F32_PAIRS", "1")
    _run_k2e(ops, name, f32_pairs=True)


@pytest.mark.parametrize("name", sorted(R.K0_CASES))
def test_k0_adjoint_vs_fp64_reference(ops, name):
    """vaa_patch_resize_bwd per element, on the size lists of test_patch_resize_kernel_vs_torch_cpu."""
    ref, gy, pdesc = R.case_ref("k0", name)
    ph, pw, _sizes = R.K0_CASES[name]
    got = ops.patch_resize_bwd(_t(gy.astype(np.float32)), _t(pdesc), ph, pw)
    _compare(ref, got, "K0 adjoint", name)
    _report()
