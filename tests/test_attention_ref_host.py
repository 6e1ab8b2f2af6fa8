"""CPU-only: the yardstick of test_gpu_attention_ref.py is sane without a GPU — the fp64 reference agrees with the closed-form gradients of
softmax attention, and the eager bf16 baseline's error against it is finite and non-zero for every case family."""
import math

import torch

import attention_ref as A


def test_eager_baseline_error_is_finite_and_nonzero_for_every_family():
    seen = set()
    for c in A.group("cpu"):
        _, ref, base = A.references(c)
        seen.add((A.family(c["hd"]), bool(c["lens"]), c["rope"], c["amp"] != 1.0))
        for n in ("o", "dq", "dk", "dv"):
            mx, rms = base[n]
            assert math.isfinite(rms) and math.isfinite(mx) and 0.0 < rms <= mx, (A.key(c), n, base[n])
            assert mx <= 2e-2 * float(ref[n].abs().max()) + 1e-2 or c["amp"] != 1.0, (A.key(c), n, base[n])  # bf16 noise, not a wrong formula
    assert {f for f, _, _, _ in seen} == {"2,4", "3,5", "3,6", "4,8"}
    assert any(p for _, p, _, _ in seen) and any(r for _, _, r, _ in seen) and any(a for _, _, _, a in seen)


def test_fp64_reference_matches_closed_form():
    """Autograd's dq / dk / dv == the textbook expressions (dV = P^T dO, dS = P o (dP - rowsum(dP o P)), dQ = scale dS K, dK = scale dS^T Q),
    lse == log sum exp, causal row 0 == v[0]; the packed form == its samples run alone; the RoPE form == plain attention on rotated inputs."""
    c = A.case(2, 2, 37, 40, True, seed=11)
    inp = A.make_inputs(c)
    ref = A.ref_fp64(c, inp)
    q, k, v, do = [inp[n].double().permute(0, 2, 1, 3) for n in ("q", "k", "v", "do")]
    scale = 40 ** -0.5
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(37, 37, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(s, -1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    for name, want in (("o", p @ v), ("dv", p.transpose(-1, -2) @ do), ("dq", ds @ k * scale), ("dk", ds.transpose(-1, -2) @ q * scale)):
        assert (ref[name] - want.permute(0, 2, 1, 3)).abs().max() < 1e-12, name
    assert (ref["lse"] - torch.logsumexp(s, -1)).abs().max() < 1e-12
    assert torch.equal(ref["o"][:, 0], inp["v"][:, 0].double())
    # packed == per sample
    lens = [5, 1, 33]
    cp = A.case(3, 2, 33, 64, False, lens=lens, rope=True, seed=12)
    ip = A.make_inputs(cp)
    rp = A.ref_fp64(cp, ip)
    s0 = 0
    for b, n in enumerate(lens):
        one = {m: (t[:, s0:s0 + n] if m in ("q", "k", "v", "do") else t[s0:s0 + n]) for m, t in ip.items()}
        r1 = A.ref_fp64(A.case(1, 2, n, 64, False, rope=True), one)
        for name in ("o", "dq", "dk", "dv"):
            assert (rp[name][:, s0:s0 + n] - r1[name]).abs().max() < 1e-12
        assert (rp["lse"][b, :, :n] - r1["lse"][0]).abs().max() < 1e-12 and bool(torch.isnan(rp["lse"][b, :, n:]).all())
        s0 += n
    # RoPE form: the rotation is orthogonal, so dq w.r.t. the un-rotated q is the inverse rotation of the gradient w.r.t. the rotated one
    cr = A.case(1, 2, 19, 64, True, rope=True, seed=13)
    ir = A.make_inputs(cr)
    rr = A.ref_fp64(cr, ir)
    rot = dict(ir, q=A._rope(ir["q"].double(), ir["cos"], ir["sin"]), k=A._rope(ir["k"].double(), ir["cos"], ir["sin"]), cos=None, sin=None)
    r0 = A._run_graph(dict(cr, rope=False), rot, torch.float64, lambda x: x)
    assert (rr["o"] - r0["o"]).abs().max() < 1e-12
    assert (rr["dq"] - A._rope(r0["dq"], ir["cos"], -ir["sin"])).abs().max() < 1e-12 and (rr["dk"] - A._rope(r0["dk"], ir["cos"], -ir["sin"])).abs().max() < 1e-12
