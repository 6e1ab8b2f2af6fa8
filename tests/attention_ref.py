"""What the attention tests share (a plain module, not a conftest): an fp64 reference of vaa_model_attention_{fwd,bwd}, the eager bf16
formulation the kernels replace (the error yardstick), the named case groups of test_gpu_attention_ref.py, and the runners that push a case
through the kernels and report its errors.

    python tests/attention_ref.py GROUP [GROUP ...]      (or python -m attention_ref from tests/)

prints one JSON line per case. VAA_ATTN_G is read once per process, so a forced grouping needs a fresh process: `run_child` starts one
(one at a time, one attempt, under a time limit).

Tolerances (the hard ceilings are those of test_gpu_model_ops.py):
    o       max error <= 2^-7 max|ref| + 1e-3
    lse     max error <= 1e-4
    grads   max error <= 2e-2 max|ref| + 1e-5
and, because a max ceiling lets one wrong key through in a 193-key row, per tensor
    rms(kernel - fp64) <= RMS_FACTOR * rms(eager bf16 - fp64) + RMS_FLOOR
on the same inputs. Both sides round P and every output to bf16 once and round dS before its two products; the factor 2 pays for summation
order and for rounding the un-normalised exp instead of the normalised P. RMS_FLOOR covers the tensors whose fp64 value is identically zero
(dq, dk with a single visible key): the eager softmax backward gives an exact 0 there, the kernels recompute P = exp2(s - lse) from the fp32
lse and leave an fp32-epsilon residue (2^-23 x |dP| |k| ~ 1e-6); the floor is the absolute term the max ceiling already grants gradients.
lse has no eager yardstick (its 1e-4 ceiling is absolute), and the fused-RoPE cases do not assert it: the kernels see q, k rotated AND
rounded to bf16, the fp64 reference rotates without rounding, which moves a logit by 2^-9 |q||k| scale ~ 1e-3.
"""
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
BF = torch.bfloat16
RMS_FACTOR = 2.0
RMS_FLOOR = 1e-5
SENTINEL16 = 0x4B4B  # bf16 1.33e7: finite, not a value any case produces
SENTINEL32 = 0x4B4B4B4B
PACKED_LENS = [1, 63, 64, 65, 130, 17]


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def case(B, H, T, hd, causal, lens=None, rope=False, amp=1.0, seed=0):
    """One case: dense [B,T,H,hd], or packed (lens: the samples' lengths, B = len(lens), T = max). amp scales q and k."""
    return dict(B=B, H=H, T=T, hd=hd, causal=bool(causal), lens=lens, rope=bool(rope), amp=float(amp), seed=int(seed))


def family(hd):
    """The <KS,NT> instantiation launch_fwd / launch_bwd pick for a head width."""
    return "2,4" if hd <= 64 else "3,5" if hd <= 80 else "3,6" if hd <= 96 else "4,8"


DENSE_HD = (8, 40, 64, 72, 80, 88, 96, 104, 128)
DENSE_T = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193)
DENSE_BH = ((1, 1), (7, 1), (3, 3), (1, 17))  # B*H = 1, 7, 9, 17: below, at and across the 8-pair XCD grouping of block_to_pair


def group(name):
    """The named case groups."""
    if name == "dense":  # every instantiation: two widths per family (padded and exact), wave / tile / G=2-block edges of T
        return [case(B, H, T, hd, c, seed=1) for hd in DENSE_HD for c in (True, False) for T in DENSE_T for B, H in DENSE_BH]
    if name == "packed":
        out = [case(len(PACKED_LENS), 2, max(PACKED_LENS), hd, c, lens=PACKED_LENS, seed=2) for hd in (64, 72, 128) for c in (True, False)]
        return out + [case(len(PACKED_LENS), 2, max(PACKED_LENS), hd, c, lens=PACKED_LENS, rope=True, seed=3) for hd in (64, 128) for c in (True, False)]
    if name == "rope":
        return [case(2, 3, T, hd, c, rope=True, seed=4) for hd in (64, 128) for T in (17, 75, 129) for c in (True, False)]
    if name == "range":  # scale q.k spans about +-60 (sigma 15, 4 sigma over ~10^4 logits): running-max rescale, exp2 underflow to zero
        return [case(2, 2, 193, hd, c, amp=15.0 ** 0.5, seed=5) for hd in (64, 72, 128) for c in (True, False)]
    if name == "cpu":  # one small case per family of the yardstick's own test (no GPU)
        return ([case(2, 2, 65, hd, c, seed=6) for hd in (40, 72, 88, 104) for c in (True, False)]
                + [case(3, 2, 65, 64, True, lens=[1, 65, 17], seed=6), case(3, 2, 65, 64, False, lens=[1, 65, 17], rope=True, seed=6),
                   case(2, 2, 33, 128, True, rope=True, seed=6), case(1, 2, 97, 64, False, amp=15.0 ** 0.5, seed=6)])
    raise KeyError(name)


def key(c):
    return "hd%d_%s_T%d_B%dH%d%s%s%s" % (c["hd"], "causal" if c["causal"] else "full", c["T"], c["B"], c["H"], "_packed" if c["lens"] else "",
                                         "_rope" if c["rope"] else "", "_amp" if c["amp"] != 1.0 else "")


def make_inputs(c):
    """bf16 q, k, v, dout on the CPU ([B,T,H,hd], packed: [1,sum,H,hd]) and the fp32 rotary tables the kernel gets (packed: one row per token)."""
    g = torch.Generator().manual_seed(c["seed"] * 1000003 + c["T"] * 131 + c["hd"] * 7 + c["B"] * 3 + c["H"] + 17 * c["causal"])
    shape = (1, sum(c["lens"]), c["H"], c["hd"]) if c["lens"] else (c["B"], c["T"], c["H"], c["hd"])
    q, k, v, do = [torch.randn(shape, generator=g) for _ in range(4)]
    inp = dict(q=(q * c["amp"]).to(BF), k=(k * c["amp"]).to(BF), v=v.to(BF), do=do.to(BF), cos=None, sin=None)
    if c["rope"]:
        hd = c["hd"]
        ang = torch.outer(torch.arange(c["T"], dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd)))
        cos, sin = ang.cos(), ang.sin()
        if c["lens"]:
            pos = torch.cat([torch.arange(n) for n in c["lens"]])
            cos, sin = cos.index_select(0, pos), sin.index_select(0, pos)
        inp["cos"], inp["sin"] = cos.contiguous(), sin.contiguous()
    return inp


def segments(c):
    """(batch index or None, first token, length) of every sample."""
    if not c["lens"]:
        return [(None, 0, c["T"])]
    out, s = [], 0
    for n in c["lens"]:
        out.append((None, s, n))
        s += n
    return out


# ---------------------------------------------------------------- references ----------------------------------------------------------------
def _rope(x, cos, sin):
    """HF rotate_half on [B,T,H,hd] with tables [T,hd/2]."""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    c, s = cos[None, :, None, :].to(x.dtype), sin[None, :, None, :].to(x.dtype)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _round_bf16(x):
    return x.to(BF).to(x.dtype)  # autograd rounds the gradient on the way back as well


def _attend(q, k, v, causal, scale, cos, sin, rnd):
    """softmax(scale q k^T [causal]) v on [B,T,H,hd]; rnd = identity (fp64 reference) or one bf16 rounding where the eager bf16 formulation
    has one: the rotated q / k, Q K^T, P, P V. Returns o [B,T,H,hd] and the natural-log lse [B,H,T]."""
    if cos is not None:
        q, k = rnd(_rope(q, cos, sin)), rnd(_rope(k, cos, sin))
    qh, kh, vh = [x.permute(0, 2, 1, 3) for x in (q, k, v)]
    s = rnd(qh @ kh.transpose(-1, -2)) * scale
    if causal:
        T = s.shape[-1]
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    o = rnd(rnd(torch.softmax(s, -1)) @ vh)
    return o.permute(0, 2, 1, 3), torch.logsumexp(s, -1)


def _run_graph(c, inp, dtype, rnd):
    q, k, v = [inp[n].to(dtype).requires_grad_(True) for n in "qkv"]
    scale = float(c["hd"]) ** -0.5
    os_, lses = [], []
    for _, s0, n in segments(c):  # the packed form is a loop over samples
        sl = slice(s0, s0 + n) if c["lens"] else slice(None)
        cs = (inp["cos"][sl], inp["sin"][sl]) if c["lens"] and c["rope"] else (inp["cos"], inp["sin"])
        o, lse = _attend(rnd(q[:, sl]), rnd(k[:, sl]), rnd(v[:, sl]), c["causal"], scale, cs[0], cs[1], rnd)
        os_.append(o)
        lses.append(lse)
    o = torch.cat(os_, 1)
    o.backward(inp["do"].to(dtype))
    if c["lens"]:  # lse as the kernel lays it out: [B,H,Tmax], positions >= len unset (NaN here)
        lse = torch.full((len(lses), c["H"], c["T"]), float("nan"), dtype=dtype)
        for b, l in enumerate(lses):
            lse[b, :, :l.shape[-1]] = l[0]
    else:
        lse = lses[0]
    return dict(o=o.detach().double(), lse=lse.detach().double(), dq=q.grad.double(), dk=k.grad.double(), dv=v.grad.double())


def ref_fp64(c, inp):
    """fp64 on the CPU from the same bf16 inputs; gradients by autograd, through the rotation (dq, dk w.r.t. the UN-rotated tensors)."""
    return _run_graph(c, inp, torch.float64, lambda x: x)


def eager_bf16(c, inp):
    """The formulation the kernels replace: bf16 Q K^T, fp32 softmax, P cast to bf16, bf16 P V, autograd backward. A bf16 GEMM is computed as
    the fp32 product of the bf16 values rounded once (fp32 accumulation, like the device GEMMs), which is deterministic on any host."""
    return _run_graph(c, inp, torch.float32, _round_bf16)


# ---------------------------------------------------------------- the kernels ----------------------------------------------------------------
def _str3(x):
    assert x.stride(3) == 1
    return (ctypes.c_int64 * 3)(x.stride(0), x.stride(1), x.stride(2))


def _ptr(x):
    return x.data_ptr() if x is not None else None


def c_fwd(q, k, v, o, lse, causal, scale, cu=None, B=None, T=None):
    """vaa_model_attention_fwd on caller-owned outputs (any views)."""
    from roboticattack_amd import _lib

    Bq, Tq, H, hd = q.shape
    rc = _lib.lib().vaa_model_attention_fwd(q.data_ptr(), _str3(q), k.data_ptr(), _str3(k), v.data_ptr(), _str3(v), o.data_ptr(), _str3(o), lse.data_ptr(),
                                            _ptr(cu), B or Bq, H, T or Tq, hd, int(causal), float(scale), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "vaa_model_attention_fwd")


def c_bwd(q, k, v, o, do, lse, dsum, dq, dk, dv, causal, scale, rope=None, cu=None, B=None, T=None):
    """vaa_model_attention_bwd on caller-owned outputs (any views)."""
    from roboticattack_amd import _lib

    Bq, Tq, H, hd = q.shape
    rc = _lib.lib().vaa_model_attention_bwd(q.data_ptr(), _str3(q), k.data_ptr(), _str3(k), v.data_ptr(), _str3(v), o.data_ptr(), _str3(o), do.data_ptr(),
                                            _str3(do), lse.data_ptr(), dsum.data_ptr(), dq.data_ptr(), _str3(dq), dk.data_ptr(), _str3(dk), dv.data_ptr(),
                                            _str3(dv), _ptr(rope[0]) if rope else None, _ptr(rope[1]) if rope else None, _ptr(cu), B or Bq, H, T or Tq, hd,
                                            int(causal), float(scale), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "vaa_model_attention_bwd")


def _cu(c):
    import numpy as np

    return torch.tensor([0] + list(np.cumsum(c["lens"])), dtype=torch.int32, device=DEV) if c["lens"] else None


def kernel_run(c, inp):
    """The case through model_ops.attention_fwd / attention_bwd (the fused-RoPE form: model_ops' own rotation, then the adjoint inside the
    backward). Device tensors: o, lse, dq, dk, dv."""
    from roboticattack_amd import model_ops

    q, k, v, do = [inp[n].to(DEV) for n in ("q", "k", "v", "do")]
    scale = float(c["hd"]) ** -0.5
    cu, rope = _cu(c), None
    if c["rope"]:
        rope = (inp["cos"].to(DEV), inp["sin"].to(DEV))
        q, k = model_ops._rope_launch(q, rope[0], rope[1], 1.0), model_ops._rope_launch(k, rope[0], rope[1], 1.0)
    o, lse = model_ops.attention_fwd(q, k, v, c["causal"], scale, cu, c["T"] if c["lens"] else 0)
    dq, dk, dv = model_ops.attention_bwd(q, k, v, o, lse, do, c["causal"], scale, rope=rope, cu_seqlens=cu, max_len=c["T"] if c["lens"] else 0)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _err(x, ref):
    d = (x.double() - ref)
    return float(d.abs().max()), float(d.square().mean().sqrt())


_REFS = {}


def references(c):
    """(inputs, fp64 reference, eager bf16 errors against it), computed once per case and process and left unchanged."""
    kk = key(c)
    if kk not in _REFS:
        inp = make_inputs(c)
        ref = ref_fp64(c, inp)
        base = eager_bf16(c, inp)
        _REFS[kk] = (inp, ref, {n: _err(base[n], ref[n]) for n in ("o", "dq", "dk", "dv")})
    return _REFS[kk]


def run_cases(cases):
    """Every case through the kernels; per tensor the max and RMS error against fp64 of the kernel and of the eager bf16 baseline."""
    out = []
    for c in cases:
        inp, ref, base = references(c)
        got = {n: t.cpu() for n, t in kernel_run(c, inp).items()}
        r = dict(case=key(c), family=family(c["hd"]), rope=c["rope"], finite=all(bool(torch.isfinite(got[n]).all()) for n in ("o", "dq", "dk", "dv")))
        for n in ("o", "dq", "dk", "dv"):
            mx, rms = _err(got[n], ref[n])
            r[n] = dict(max=mx, rms=rms, base_max=base[n][0], base_rms=base[n][1], ref_max=float(ref[n].abs().max()))
        valid = ~torch.isnan(ref["lse"])  # packed: positions < len
        r["lse"] = dict(max=float((got["lse"].double() - ref["lse"])[valid].abs().max()), finite=bool(torch.isfinite(got["lse"][valid]).all()))
        out.append(r)
    return out


def failures(r):
    """The bounds of the module docstring on one result of run_cases; a list of messages (empty: the case passes)."""
    bad = []
    if not (r["finite"] and r["lse"]["finite"]):
        bad.append("non-finite output")
    for n in ("o", "dq", "dk", "dv"):
        e = r[n]
        ceil = 2.0 ** -7 * e["ref_max"] + 1e-3 if n == "o" else 2e-2 * e["ref_max"] + 1e-5
        if not e["max"] <= ceil:
            bad.append("%s max %.3e > %.3e" % (n, e["max"], ceil))
        if not e["rms"] <= RMS_FACTOR * e["base_rms"] + (RMS_FLOOR if n != "o" else 0.0):
            bad.append("%s rms %.3e > %g x eager %.3e" % (n, e["rms"], RMS_FACTOR, e["base_rms"]))
    if not r["rope"] and not r["lse"]["max"] <= 1e-4:
        bad.append("lse max %.3e > 1e-4" % r["lse"]["max"])
    return ["%s: %s" % (r["case"], b) for b in bad]


def worst_ratios(results):
    """{(family, tensor): worst kernel-rms / eager-rms} over the results whose eager error is not zero (the table of DESIGN.md)."""
    w = {}
    for r in results:
        for n in ("o", "dq", "dk", "dv"):
            if r[n]["base_rms"] > 0:
                kf = (r["family"], n)
                w[kf] = max(w.get(kf, 0.0), r[n]["rms"] / r[n]["base_rms"])
    return w


# ---------------------------------------------------------------- bitwise groups ----------------------------------------------------------------
def _bits(x):
    return x.contiguous().view(torch.int16)


def _plain(c, inp):
    q, k, v, do = [inp[n].to(DEV) for n in ("q", "k", "v", "do")]
    return (q, k, v, do), kernel_run(dict(c, rope=False), inp)


def run_layouts():
    """Slices of one [B,T,3,H,hd] buffer with a packed gradient, and [B,H,T,hd] memory viewed as [B,T,H,hd] (head stride > token stride) for q,
    k, v and dout, against three contiguous tensors: bit for bit."""
    from roboticattack_amd import model_ops

    out = []
    for hd, T, causal in [(64, 65, True), (72, 129, False), (88, 17, True), (128, 130, False), (40, 64, True)]:
        c = case(2, 3, T, hd, causal, seed=7)
        inp = make_inputs(c)
        (q, k, v, do), ref = _plain(c, inp)
        scale = float(hd) ** -0.5
        qkv = torch.stack([q, k, v], 2).contiguous()
        o1, l1 = model_ops.attention_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], causal, scale)
        buf = model_ops.attention_bwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], o1, l1, do, causal, scale, packed_grad=True)
        same1 = all(torch.equal(_bits(a), _bits(b)) for a, b in zip((o1, buf[:, :, 0], buf[:, :, 1], buf[:, :, 2]), (ref["o"], ref["dq"], ref["dk"], ref["dv"])))
        same1 = same1 and torch.equal(l1, ref["lse"])
        qt, kt, vt, dot = [x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for x in (q, k, v, do)]
        assert qt.stride(2) > qt.stride(1)
        o2, l2 = model_ops.attention_fwd(qt, kt, vt, causal, scale)
        g2 = model_ops.attention_bwd(qt, kt, vt, o2, l2, dot, causal, scale)
        same2 = all(torch.equal(_bits(a), _bits(b)) for a, b in zip((o2,) + tuple(g2), (ref["o"], ref["dq"], ref["dk"], ref["dv"]))) and torch.equal(l2, ref["lse"])
        out.append(dict(case=key(c), packed_qkv_equal=bool(same1), bhtd_view_equal=bool(same2)))
    return out


def run_independence():
    """A (b,h) slice computed inside a B*H = 17 batch against the same slice run alone as B = H = 1: bit for bit (hd = 72: the padded columns of
    a slice read its neighbour head)."""
    out = []
    for hd, T, causal in [(72, 65, True), (72, 129, False), (64, 63, True), (104, 17, False), (128, 129, True)]:
        c = case(1, 17, T, hd, causal, seed=8)
        inp = make_inputs(c)
        _, full = _plain(c, inp)
        same = True
        for h in (0, 7, 8, 16):
            one = {n: (t[:, :, h:h + 1].contiguous() if t is not None else None) for n, t in inp.items() if n in ("q", "k", "v", "do")}
            one.update(cos=None, sin=None)
            got = kernel_run(case(1, 1, T, hd, causal), one)
            same = same and all(torch.equal(_bits(got[n]), _bits(full[n][:, :, h:h + 1])) for n in ("o", "dq", "dk", "dv"))
            same = same and torch.equal(got["lse"], full["lse"][:, h:h + 1])
        out.append(dict(case=key(c), slice_equal=bool(same)))
    return out


def run_single_key():
    """Causal row 0 sees one key: o[:,0] == v[:,0] bit for bit, lse[:,:,0] == scale q0.k0 to 1e-4."""
    out = []
    for hd in (8, 64, 72, 88, 128):
        c = case(2, 3, 65, hd, True, seed=9)
        inp = make_inputs(c)
        got = kernel_run(c, inp)
        s00 = (inp["q"][:, 0].double() * inp["k"][:, 0].double()).sum(-1) * float(hd) ** -0.5  # [B,H]
        out.append(dict(case=key(c), o0_is_v0=bool(torch.equal(_bits(got["o"][:, 0]), _bits(inp["v"][:, 0].to(DEV)))),
                        lse0_err=float((got["lse"][:, :, 0].cpu().double() - s00).abs().max())))
    return out


def _sentinel_view(shape_bthd, slack_rows=130):
    """A [B,T,H,hd] view of a sentinel-filled [B,T+3,H,hd+8] buffer followed by slack_rows more sentinel rows (more than a padded column or a
    tile row past the view could reach), and the flat int16 storage."""
    B, T, H, hd = shape_bthd
    n = B * (T + 3) * H * (hd + 8)
    flat = torch.full((n + slack_rows * H * (hd + 8),), SENTINEL16, dtype=torch.int16, device=DEV)
    return flat[:n].view(BF).view(B, T + 3, H, hd + 8)[:, :T, :, :hd], flat


def _sentinel_f32(n, slack=256):
    flat = torch.full((n + slack,), SENTINEL32, dtype=torch.int32, device=DEV)
    return flat[:n].view(torch.float32), flat


def _untouched(view, flat, valid=None):
    """Every element of the storage outside the view (and, packed form, view rows outside `valid` tokens) still holds the sentinel."""
    B, T, H, hd = view.shape
    n = B * (T + 3) * H * (hd + 8)
    own = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    m = own[:n].view(B, T + 3, H, hd + 8)
    m[:, :T if valid is None else valid, :, :hd] = True
    return bool((flat[~own] == SENTINEL16).all())


def run_writes():
    """o, dq, dk, dv as [..., :hd] views of larger sentinel-filled buffers (packed form: a gap of untouched tokens after the last sample), lse
    and dsum with a sentinel tail: every sentinel survives and the viewed region is the ordinary call's, bit for bit."""
    out = []
    lens = [17, 65, 64, 1]
    todo = [case(2, 3, T, hd, c, seed=10) for hd in (72, 88, 104) for T, c in ((17, True), (65, False), (129, True))]
    todo += [case(len(lens), 2, max(lens), hd, c, lens=lens, seed=10) for hd, c in ((72, True), (88, False), (104, True))]
    for c in todo:
        inp = make_inputs(c)
        (q, k, v, do), ref = _plain(c, inp)
        hd, H, scale, cu = c["hd"], c["H"], float(c["hd"]) ** -0.5, _cu(c)
        gap = 70 if c["lens"] else 0
        tot = q.shape[1]
        shape = (q.shape[0], tot + gap, H, hd)
        (o, fo), (dq, fq), (dk, fk), (dv, fv) = [_sentinel_view(shape) for _ in range(4)]
        nl = c["B"] * H * c["T"]
        (lse, fl), (dsum, fd) = _sentinel_f32(nl), _sentinel_f32(nl)
        kw = dict(cu=cu, B=c["B"], T=c["T"]) if c["lens"] else {}
        c_fwd(q, k, v, o, lse, c["causal"], scale, **kw)
        c_bwd(q, k, v, o[:, :tot], do, lse, dsum, dq, dk, dv, c["causal"], scale, **kw)  # o stays the strided view
        torch.cuda.synchronize()
        valid = tot if c["lens"] else None
        clean = all(_untouched(t, f, valid) for t, f in ((o, fo), (dq, fq), (dk, fk), (dv, fv)))
        clean = clean and bool((fl[nl:] == SENTINEL32).all()) and bool((fd[nl:] == SENTINEL32).all())
        same = all(torch.equal(_bits(t[:, :tot]), _bits(ref[n])) for t, n in ((o, "o"), (dq, "dq"), (dk, "dk"), (dv, "dv")))
        lse_k, lse_r = lse.view(c["B"], H, c["T"]), ref["lse"]
        if c["lens"]:  # positions >= len are nobody's
            for b, n in enumerate(c["lens"]):
                same = same and torch.equal(lse_k[b, :, :n], lse_r[b, :, :n])
                clean = clean and bool((lse_k[b, :, n:].view(torch.int32) == SENTINEL32).all())
        else:
            same = same and torch.equal(lse_k, lse_r)
        out.append(dict(case=key(c), sentinels_intact=bool(clean), view_equals_plain=bool(same)))
    return out


BITWISE = dict(layouts=run_layouts, independence=run_independence, single_key=run_single_key, writes=run_writes)


def run_group(name):
    return BITWISE[name]() if name in BITWISE else run_cases(group(name))


def run_child(groups, attn_g=None, timeout=300):
    """The groups in one fresh process (VAA_ATTN_G = attn_g: the forced grouping is read once per process): {group: [result, ...]}."""
    env = dict(os.environ)
    env.pop("VAA_ATTN_G", None)
    if attn_g:
        env["VAA_ATTN_G"] = attn_g
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(groups), env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    out = {g: [] for g in groups}
    for line in p.stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            out[d.pop("group")].append(d)
    return out


def main(argv):
    for name in argv:
        for r in run_group(name):
            print(json.dumps(dict(r, group=name)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
