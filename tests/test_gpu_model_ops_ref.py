"""The streaming and norm kernels of vaa_model_ops.hip against torch double computed from the same bf16 inputs, at the shapes where they can go
wrong: the second trip of the grid-stride loop (stream_grid caps the grid at 8192 x 256 threads), narrow and odd widths, the LayerNorm
dispatch edges and its 4-rows-per-workgroup tail, __expf overflow in SwiGLU.

Bounds. Every output is ONE bf16 rounding of an fp32 evaluation: |err| <= 2^-8 |ref| elementwise (half a bf16 ulp, relative to the value)
plus the fp32 evaluation error in front of the rounding, which only matters where terms cancel and is bounded per operator from the
magnitudes of its terms (2^-24 per fp32 operation) — always far inside the 2^-8 max|ref| the existing tests grant. Norm gradients also keep
the existing ceiling 2^-5 max|ref|.

    python tests/test_gpu_model_ops_ref.py layernorm      (the LayerNorm cases in this process: what the VAA_LN_WAVE=0 child runs)
"""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
TRIP = 8192 * 256  # vectors of one pass of the grid-stride loop
U = 2.0 ** -8      # one bf16 rounding, relative


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale + shift).to(BF)


def _within(got, ref, slack):
    """|got - ref| <= 2^-8 |ref| + slack elementwise (slack: tensor or number), everything finite."""
    err = (got.double() - ref).abs()
    ok = bool(torch.isfinite(got).all()) and bool((err <= U * ref.abs() + slack).all())
    return ok, float((err - U * ref.abs() - slack).max())


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- RoPE ----------------------------------------------------------------
def _tables(T, hd):
    ang = torch.outer(torch.arange(T, device=DEV, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=DEV, dtype=torch.float32) / hd)))
    return ang.cos().contiguous(), ang.sin().contiguous()


def _rope64(x, cos, sin, sign):
    """fp64 HF rotate_half with the kernel's fp32 tables; also the fp32-evaluation slack: three fp32 roundings on |x1 c| + |x2 s|."""
    half = x.shape[-1] // 2
    x1, x2 = x.double()[..., :half], x.double()[..., half:]
    c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :] * sign
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return ref, mag * 2.0 ** -21


@pytest.mark.parametrize("hd", [16, 48, 64, 128])
def test_rope_vs_fp64_layouts_and_adjoint(hd):
    from roboticattack_amd import model_ops

    B, T, H = 2, 37, 3
    g = _gen(hd)
    cos, sin = _tables(T, hd)
    x = _randn(g, B, T, H, hd)
    ref, slack = _rope64(x, cos, sin, 1.0)
    out = model_ops._rope_launch(x, cos, sin, 1.0)
    assert out.shape == x.shape and out.is_contiguous()
    assert _within(out, ref, slack)[0], _within(out, ref, slack)
    # [B,H,T,hd] memory viewed as [B,T,H,hd], and the q slice of a packed [B,T,3,H,hd] buffer: the same bits
    xt = x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    qkv = torch.stack([x, _randn(g, B, T, H, hd), _randn(g, B, T, H, hd)], 2).contiguous()
    assert xt.stride(2) > xt.stride(1) and qkv[:, :, 0].stride(1) == 3 * H * hd
    assert torch.equal(model_ops._rope_launch(xt, cos, sin, 1.0), out) and torch.equal(model_ops._rope_launch(qkv[:, :, 0], cos, sin, 1.0), out)
    # sin_sign = -1 is the exact adjoint: against fp64, and <rope(x), y> == <x, rope^T(y)> within the roundings of the two outputs
    y = _randn(g, B, T, H, hd)
    refb, slackb = _rope64(y, cos, sin, -1.0)
    outb = model_ops._rope_launch(y, cos, sin, -1.0)
    assert _within(outb, refb, slackb)[0], _within(outb, refb, slackb)
    lhs, rhs = (out.double() * y.double()).sum(), (x.double() * outb.double()).sum()
    bound = ((U * ref.abs() + slack) * y.double().abs()).sum() + ((U * refb.abs() + slackb) * x.double().abs()).sum()
    assert abs(float(lhs - rhs)) <= float(bound)
    assert abs(float((ref * y.double()).sum() - (x.double() * refb).sum())) <= 1e-9 * float(bound)  # the reference itself is an adjoint pair


def test_rope_second_grid_trip():
    """Just above 8192 x 256 vectors (67 MB): the tokens of the second grid-stride trip against fp64, like the first and the last of the first."""
    from roboticattack_amd import model_ops

    B, T, H, hd = 1, 4097, 64, 128
    assert B * T * H * hd // 16 > TRIP and B * (T - 1) * H * hd // 16 == TRIP  # token 4096 is exactly the second trip
    g = _gen(7)
    cos, sin = _tables(T, hd)
    x = _randn(g, B, T, H, hd)
    out = model_ops._rope_launch(x, cos, sin, 1.0)
    ref, slack = _rope64(x, cos, sin, 1.0)
    ok, worst = _within(out, ref, slack)
    assert ok, worst
    assert _within(out[:, T - 1:], ref[:, T - 1:], slack[:, T - 1:])[0] and float(out[:, T - 1].float().abs().max()) > 0


# ---------------------------------------------------------------- SwiGLU ----------------------------------------------------------------
def _swiglu_check(gate, up, dy):
    from roboticattack_amd import _lib

    n = gate.numel()
    y, dg, du = torch.empty_like(gate), torch.empty_like(gate), torch.empty_like(gate)
    _lib.check(_lib.lib().vaa_model_swiglu_fwd(gate.data_ptr(), up.data_ptr(), y.data_ptr(), n, _stream()), "vaa_model_swiglu_fwd")
    _lib.check(_lib.lib().vaa_model_swiglu_bwd(dy.data_ptr(), gate.data_ptr(), up.data_ptr(), dg.data_ptr(), du.data_ptr(), n, _stream()), "vaa_model_swiglu_bwd")
    g64, u64, d64 = gate.double(), up.double(), dy.double()
    sig = torch.sigmoid(g64)
    silu = g64 * sig
    # fp32 evaluation: __expf (|rel| <= 2^-18 for |g| <= 104: the argument's scaling by log2 e is rounded), a division and a few products,
    # all relative to the terms -> 2^-16 of them; 2^-116: where __expf overflows (g < -88.72) the kernel returns 0 for |silu| <= 2.6e-37
    tiny = 2.0 ** -116
    ok_y = _within(y, silu * u64, 2.0 ** -16 * (silu * u64).abs() + tiny)
    ok_u = _within(du, d64 * silu, 2.0 ** -16 * (d64 * silu).abs() + tiny)
    lead = (d64 * u64 * sig).abs()
    ok_g = _within(dg, d64 * u64 * sig * (1.0 + g64 * (1.0 - sig)), 2.0 ** -16 * lead * (1.0 + g64.abs()) + tiny)  # 1 + g (1 - sig) cancels near g = -1.28
    assert ok_y[0] and ok_u[0] and ok_g[0], (ok_y, ok_u, ok_g)
    return y, dg, du


def test_swiglu_one_vector_and_gate_range():
    g = _gen(1)
    _swiglu_check(_randn(g, 8, scale=2.0), _randn(g, 8), _randn(g, 8))
    # gates spanning +-104: __expf(104) overflows to inf, __expf(-104) underflows to 0; silu and its derivative stay finite and right
    gate = torch.cat([torch.linspace(-104.0, 104.0, 4081, device=DEV), torch.tensor([-104.0, 104.0, -89.0, 89.0, -88.0, 88.0, 0.0], device=DEV)]).to(BF)
    assert gate.numel() % 8 == 0 and float(gate.min()) == -104.0 and float(gate.max()) == 104.0
    y, dg, du = _swiglu_check(gate, _randn(g, gate.numel()), _randn(g, gate.numel()))
    assert all(bool(torch.isfinite(t).all()) for t in (y, dg, du))


def test_swiglu_second_grid_trip():
    """n = 8 (8192 x 256 + 1): the second trip of the grid-stride loop is ONE vector; it and everything before it against fp64."""
    g = _gen(2)
    n = 8 * (TRIP + 1)
    y, dg, du = _swiglu_check(_randn(g, n, scale=2.0), _randn(g, n), _randn(g, n))
    assert all(float(t[-8:].float().abs().min()) > 0 for t in (y, dg, du))  # the last vector was written


# ---------------------------------------------------------------- scale_add ----------------------------------------------------------------
def _scale_add_c(x, a, ls):
    from roboticattack_amd import _lib

    D = a.shape[-1]
    out = torch.empty_like(a)
    _lib.check(_lib.lib().vaa_model_scale_add(x.data_ptr() if x is not None else None, a.data_ptr(), ls.data_ptr(), out.data_ptr(), a.numel() // D, D, _stream()),
               "vaa_model_scale_add")
    return out


@pytest.mark.parametrize("rows,D", [(5, 8), (7, 1032), ((TRIP + 1) // 129, 1032)])
def test_scale_add_bitwise_with_and_without_x(rows, D):
    """out = x + a ls and, x == NULL, out = a ls: the fp32 value (a bf16 x bf16 product is exact in fp32, so one fp32 rounding with or without an
    FMA) rounded once to bf16, bit for bit. D / 8 = 1 and 129 (`v % dvec` wraps at no power of two); the last case is 8192 x 256 + 1 vectors."""
    assert rows * (D // 8) == TRIP + 1 or rows < 8
    g = _gen(rows + D)
    x, a, ls = _randn(g, rows, D), _randn(g, rows, D), _randn(g, D, scale=0.1)
    assert torch.equal(_scale_add_c(x, a, ls), (x.float() + a.float() * ls.float()).to(BF))
    assert torch.equal(_scale_add_c(None, a, ls), (a.float() * ls.float()).to(BF))
    assert torch.equal(_scale_add_c(x, a, ls), torch.addcmul(x.float(), a.float(), ls.float()).to(BF))


# ---------------------------------------------------------------- RMSNorm ----------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 2048, 2056, 4096, 5120, 8192])
@pytest.mark.parametrize("rows", [1, 5])
def test_rmsnorm_vs_fp64(D, rows):
    from roboticattack_amd import _lib

    L, eps = _lib.lib(), 1e-6
    g = _gen(D + rows)
    x, w = _randn(g, rows, D, scale=1.5), _randn(g, D, scale=0.1, shift=1.0)
    gh, gp = _randn(g, rows, D, shift=0.5), _randn(g, rows, D)
    h, rstd = torch.empty_like(x), torch.empty(rows, dtype=torch.float32, device=DEV)
    _lib.check(L.vaa_model_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), h.data_ptr(), rstd.data_ptr(), rows, D, eps, _stream()), "vaa_model_rmsnorm_fwd")
    x64 = x.double().requires_grad_(True)
    r64 = torch.rsqrt(x64.square().mean(-1, keepdim=True) + eps)
    assert ((rstd.double() - r64.detach()[:, 0]).abs() <= 1e-6 * r64.detach()[:, 0]).all()
    # HF LlamaRMSNorm rounds twice: (x * rstd).to(bf16) * w. Given its own (just checked) fp32 rstd the kernel's h is determined bit for bit ...
    assert torch.equal(h, ((x.float() * rstd[:, None]).to(BF).float() * w.float()).to(BF))
    # ... and against fp64 alone: the final rounding (2^-8) plus one ulp of the intermediate (2^-7) where fp32 and fp64 round x * rstd apart
    ref_h = (x64.detach() * r64.detach()).to(BF).double() * w.double()
    assert _within(h, ref_h, 2.0 ** -7 * ref_h.abs())[0]
    smooth = x64 * r64 * w.double()
    (smooth * gh.double() + x64 * gp.double()).sum().backward()
    terms = gp.double().abs().max() + 2 * (r64.detach() * gh.double() * w.double()).abs().max()
    for gpass, ref in ((gp, x64.grad), (None, x64.grad - gp.double())):
        gx = torch.empty_like(x)
        _lib.check(L.vaa_model_rmsnorm_bwd(gh.data_ptr(), gpass.data_ptr() if gpass is not None else None, x.data_ptr(), w.data_ptr(), rstd.data_ptr(),
                                           gx.data_ptr(), rows, D, _stream()), "vaa_model_rmsnorm_bwd")
        assert _within(gx, ref, 2.0 ** -16 * float(terms))[0], (D, rows, gpass is None, _within(gx, ref, 2.0 ** -16 * float(terms)))
        assert (gx.double() - ref).abs().max() <= 2.0 ** -5 * ref.abs().max()


def test_rmsnorm_rejects_rows_wider_than_8192():
    from roboticattack_amd import _lib

    t = torch.zeros(8200, dtype=BF, device=DEV)
    r = torch.zeros(1, dtype=torch.float32, device=DEV)
    assert _lib.lib().vaa_model_rmsnorm_fwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), r.data_ptr(), 1, 8200, 1e-6, _stream()) == -1  # VAA_E_INVALID
    assert _lib.lib().vaa_model_rmsnorm_bwd(t.data_ptr(), None, t.data_ptr(), t.data_ptr(), r.data_ptr(), t.data_ptr(), 1, 8200, _stream()) == -1


# ---------------------------------------------------------------- LayerNorm ----------------------------------------------------------------
LN_D = (8, 512, 1024, 1032, 1536, 1544, 8192)  # the wave kernels' edges (<= 1024: 2 vectors per lane, <= 1536: 3) and the workgroup kernel
LN_ROWS = (1, 2, 3, 4, 5)                      # the 4-rows-per-workgroup tail


def layernorm_failures():
    """Every (D, rows) of LN_D x LN_ROWS, gpass NULL and not, in this process's dispatch; a list of messages."""
    from roboticattack_amd import _lib

    L, eps, bad = _lib.lib(), 1e-6, []
    for D in LN_D:
        for rows in LN_ROWS:
            g = _gen(D * 8 + rows)
            x = _randn(g, rows, D, shift=100.0)  # mean 100, spread 1 (bf16 steps of 0.5 there): the variance needs its second pass
            w, b = _randn(g, D, scale=0.1, shift=1.0), _randn(g, D, scale=0.1)
            gh, gp = _randn(g, rows, D, shift=0.5), _randn(g, rows, D)
            h, stats = torch.empty_like(x), torch.empty((rows, 2), dtype=torch.float32, device=DEV)
            _lib.check(L.vaa_model_layernorm_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), h.data_ptr(), stats.data_ptr(), rows, D, eps, _stream()),
                       "vaa_model_layernorm_fwd")
            x64 = x.double().requires_grad_(True)
            mean = x64.mean(-1, keepdim=True)
            r64 = torch.rsqrt((x64 - mean).square().mean(-1, keepdim=True) + eps)
            ref_h = (x64 - mean) * r64 * w.double() + b.double()
            # statistics: at most ~42 fp32 roundings on the way to a row sum (32 adds per lane, the reduction tree, a division, rsqrt): 1e-6 relative
            want = torch.cat([mean, r64], -1).detach()
            if not bool(((stats.double() - want).abs() <= 1e-6 * want.abs()).all()):
                bad.append("D=%d rows=%d: {mean, rstd} off by %.3e relative" % (D, rows, float(((stats.double() - want).abs() / want.abs()).max())))
            # h: one rounding; the statistics' error (1e-6 x 100 through rstd w ~ 1) and the fp32 cancellation of x - mean stay below 2^-12 max|h|
            ok, worst = _within(h, ref_h.detach(), 2.0 ** -12 * float(ref_h.detach().abs().max()))
            if not ok:
                bad.append("D=%d rows=%d: h exceeds its bound by %.3e" % (D, rows, worst))
            (ref_h * gh.double() + x64 * gp.double()).sum().backward()
            terms = float(gp.double().abs().max() + 3 * (r64.detach() * gh.double() * w.double()).abs().max())
            for gpass, ref in ((gp, x64.grad), (None, x64.grad - gp.double())):
                gx = torch.empty_like(x)
                _lib.check(L.vaa_model_layernorm_bwd(gh.data_ptr(), gpass.data_ptr() if gpass is not None else None, x.data_ptr(), w.data_ptr(),
                                                     stats.data_ptr(), gx.data_ptr(), rows, D, _stream()), "vaa_model_layernorm_bwd")
                ok, worst = _within(gx, ref, 2.0 ** -14 * terms)  # xhat carries the mean's error: 1e-6 x 100 x rstd, times |dot| <= ~1
                if not ok or not bool((gx.double() - ref).abs().max() <= 2.0 ** -5 * ref.abs().max()):
                    bad.append("D=%d rows=%d gpass=%s: gx exceeds its bound by %.3e" % (D, rows, gpass is not None, worst))
    return bad


def test_layernorm_vs_fp64_default_dispatch():
    assert os.environ.get("VAA_LN_WAVE", "1") != "0"
    bad = layernorm_failures()
    assert not bad, "\n".join(bad)


def test_layernorm_vs_fp64_workgroup_kernels_at_every_width():
    """VAA_LN_WAVE=0 (read once per process): the one-workgroup-per-row kernels at the narrow widths too, in one fresh process."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "layernorm"], env=dict(os.environ, VAA_LN_WAVE="0"), cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "layernorm ok: %d cases" % (len(LN_D) * len(LN_ROWS)) in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


if __name__ == "__main__":
    assert sys.argv[1:] == ["layernorm"], sys.argv
    failed = layernorm_failures()
    print("\n".join(failed) if failed else "layernorm ok: %d cases" % (len(LN_D) * len(LN_ROWS)))
    sys.exit(1 if failed else 0)
