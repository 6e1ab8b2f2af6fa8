"""The int8 path without a GPU: quant.quantize_q8 and the torch formulation of q8_linear against quant8_ref's numpy restatement (exact), the
activation rule's edges, the fp32 restatement against fp64 within its derived bound, a perturbation self-test of the comparison itself, the
argument guards of the two entry points, quantize_llm(model, "int8") on tiny_cfg(), and the new flags of the eval_patch parser."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import quant8_ref as R
from conftest import ROOT
from roboticattack_amd import _lib, quant

ROW_MAX = 2.0  # far above the 0.05-scale entries: the +-max of its row


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _weights(N, K, seed):
    """Random bf16 rows with the edge cases written in: a zero row (with a negative zero), a single-spike row, a row holding +max and -max."""
    rs = np.random.RandomState(seed)
    w = R.random_bf16(rs, (N, K), 0.05)
    w[0] = 0.0
    w[0, 5] = -0.0
    if N > 1:
        w[1] = 0.0
        w[1, 17] = -0.375
    if N > 2:
        w[2, 3], w[2, 4] = ROW_MAX, -ROW_MAX
    return w


@pytest.mark.parametrize("shape", [(1, 64), (3, 128), (5, 192)])
def test_quantize_q8_equals_the_reference(shape):
    N, K = shape
    w = _weights(N, K, seed=N * 1000 + K)
    q, ws = R.quantise_w(w)
    codes, wscale = quant.quantize_q8(_bf16(w))
    assert codes.dtype == torch.int8 and tuple(codes.shape) == (N, K) and wscale.dtype == torch.float32 and tuple(wscale.shape) == (N,)
    assert np.array_equal(wscale.numpy().view(np.uint32), ws.view(np.uint32)) and np.array_equal(codes.numpy(), q)
    assert (q[0] == 0).all() and ws[0] == 0  # the zero row
    if N > 1:
        assert q[1, 17] == -127 and (np.delete(q[1], 17) == 0).all()  # the single spike is its row's scale
    if N > 2:
        assert q[2, 3] == 127 and q[2, 4] == -127 and ws[2] == np.float32(ROW_MAX)
    c2, s2 = quant.quantize_q8(torch.from_numpy(w), rows_per_pass=2)  # fp32 input of the same values, another pass size
    assert torch.equal(c2, codes) and torch.equal(s2, wscale)
    wdq = quant.dequantize_q8(codes, wscale)
    assert wdq.dtype == torch.bfloat16 and np.array_equal(_bits(wdq), R.f32_to_bf16_bits(R.dequantise_w(q, ws)))
    # dequantise - requantise is idempotent: the row's +-127 entry dequantises to the (bf16) scale itself, and |127 wdq / wscale - q| <=
    # 127 * 2^-9 < 1/2, so wdq has the codes and the scales it came from
    c3, s3 = quant.quantize_q8(wdq)
    assert torch.equal(c3, codes) and torch.equal(s3, wscale) and np.array_equal(_bits(quant.dequantize_q8(c3, s3)), _bits(wdq))
    with pytest.raises(ValueError):
        quant.quantize_q8(torch.zeros(2, 96))


def _torch_act(x, t):
    xq, ascale, outl = quant.q8_act_quant_torch(_bf16(x), t)
    return xq.numpy().astype(np.int8), ascale.numpy(), np.flatnonzero(outl.numpy()).astype(np.int32)


def _same_act(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_activation_rule_edges():
    """`>=`, not `>`: an entry equal to 6.0 makes its column an outlier, the bf16 just below 6.0 does not; t = 0 gives none; a row whose every
    column is an outlier has ascale 0 and zero codes; the list is ascending; the torch formulation equals the restatement exactly."""
    K = 128
    x = np.clip(R.random_bf16(np.random.RandomState(1), (4, K)), -5, 5).astype(np.float32)
    x[2, 40] = 6.0
    x[1, 9] = -7.5
    x[3, 77] = R.BF16_ULP_BELOW_6
    assert float(R.BF16_ULP_BELOW_6) == 5.96875 and float(R.round_bf16(R.BF16_ULP_BELOW_6)) == 5.96875
    xq, ascale, idx = R.act_quant(x, 6.0)
    assert idx.tolist() == [9, 40] and (xq[:, [9, 40]] == 0).all()
    assert ascale[3] == R.BF16_ULP_BELOW_6 and xq[3, 77] == 127  # the largest ordinary entry is its row's scale
    assert _same_act(_torch_act(x, 6.0), (xq, ascale, idx))
    assert R.act_quant(x, 6.0, strict=True)[2].tolist() == [9]  # what `>` would give
    xq0, as0, idx0 = R.act_quant(x, 0.0)
    assert idx0.size == 0 and as0[1] == 7.5 and xq0[1, 9] == -127 and _same_act(_torch_act(x, 0.0), (xq0, as0, idx0))
    xa, _ = R.acts_case(3, K, -1, seed=2)
    xqa, asa, idxa = R.act_quant(xa, 6.0)
    assert idxa.tolist() == list(range(K)) and (asa == 0).all() and (xqa == 0).all() and _same_act(_torch_act(xa, 6.0), (xqa, asa, idxa))
    for n_out in (0, 1, 5):
        xc, _ = R.acts_case(7, 192, n_out, seed=3)
        got = R.act_quant(xc, 6.0)
        assert got[2].size == n_out and (np.diff(got[2]) > 0).all() and _same_act(_torch_act(xc, 6.0), got)


@pytest.mark.parametrize("M,N,K,n_out", [(1, 17, 64, 0), (7, 33, 128, 1), (16, 17, 1088, 5), (33, 16, 192, 5), (3, 8, 128, -1)])
def test_restatement_bound_and_the_torch_formulation(M, N, K, n_out):
    """The fp32 restatement stays within quant8_ref.bound (derived there) of the fp64 evaluation of the same quantised model, with and
    without res; q8_linear's torch formulation on the CPU gives the restatement's bits; an all-zero row of x gives y = res."""
    q, ws = R.weights_case(N, K, seed=1)
    x, res = R.acts_case(M, K, n_out, seed=1, N=N)
    xq, ascale, idx = R.act_quant(x, 6.0)
    for r in (None, res):
        bits = R.y32_bits(x, xq, ascale, idx, q, ws, r)
        err = np.abs(R.bf16_bits_to_f32(bits).astype(np.float64) - R.y64(x, xq, ascale, idx, q, ws, r))
        assert (err <= R.bound(x, xq, ascale, idx, q, ws, r)).all()
        lin = quant.Q8Linear(torch.from_numpy(q), torch.from_numpy(ws), 6.0)
        y = quant.q8_linear(_bf16(x), lin, None if r is None else _bf16(r))
        assert y.dtype == torch.bfloat16 and np.array_equal(_bits(y), bits)
        if M > 1:
            want = np.zeros(N, np.float32) if r is None else r[-1]
            assert np.array_equal(R.bf16_bits_to_f32(bits[-1]), want)  # the zero row: ascale 0, integer part 0, y = res


def test_the_comparison_notices_each_perturbation():
    """Flip one code, drop one outlier column, `>` for `>=`, the scales multiplied in the other order: each changes the restatement's bits
    on this case, so a kernel (or a formulation) that made the mistake would fail the bit comparison."""
    M, N, K = 7, 33, 192
    q, ws = R.weights_case(N, K, seed=4)
    x, res = R.acts_case(M, K, 5, seed=4, N=N)
    xq, ascale, idx = R.act_quant(x, 6.0)
    good = R.y32_bits(x, xq, ascale, idx, q, ws, res)
    assert np.array_equal(good, R.y32_bits(x, xq, ascale, idx, q, ws, res))
    q2 = q.copy()
    q2[3, 10] = -q2[3, 10] if q2[3, 10] else 1
    assert not np.array_equal(good, R.y32_bits(x, xq, ascale, idx, q2, ws, res))
    assert not np.array_equal(good, R.y32_bits(x, xq, ascale, idx[1:], q, ws, res))
    strict = R.act_quant(x, 6.0, strict=True)  # the column whose maximum is exactly 6.0 stays in the integer part
    assert strict[2].size == idx.size - 1 and not np.array_equal(good, R.y32_bits(x, *strict, q, ws, res))
    # The order of the scales moves an fp32 result by an ulp, which one bf16 rounding in 2^16 shows. What tells the two orders apart for
    # certain is range: activations of 2^118 with weight scales of 2^-118 (t = 0: no split). ascale * wscale is of order 1, while
    # float(acc) * ascale overflows.
    xb, wb = R.big_scales(x, ws)
    ab = R.act_quant(xb, 0.0)
    goodb = R.y32_bits(xb, *ab, q, wb, res)
    assert np.isfinite(R.bf16_bits_to_f32(goodb)).all()
    with np.errstate(over="ignore", invalid="ignore"):
        assert not np.array_equal(goodb, R.y32_bits(xb, *ab, q, wb, res, swap_scales=True))


def test_entry_point_guards_without_gpu():
    """NULL, K = 96, K beyond the int32 range, a bad threshold, a bad form, M = 17 in the split-K form, M = 0 and misaligned bases: every one
    is answered before any launch (host buffers stand in for the operands)."""
    L = _lib.lib()
    raw = (ctypes.c_uint8 * 8192)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    p = lambda off=0: ctypes.c_void_p(base + off)
    act = lambda x, M, K, t, xq, a, o: L.vaa_model_q8_act_quant(x, M, K, t, xq, a, o, None)
    mm = lambda xq, a, o, x, M, q, ws, N, K, res, y, form=0: L.vaa_model_q8_matmul(xq, a, o, x, M, q, ws, N, K, res, y, form, None)
    assert {"vaa_model_q8_act_quant", "vaa_model_q8_matmul"} <= set(_lib.MODEL_OP_EXPORTS)
    assert act(None, 0, 64, 6.0, None, None, None) == 0 and mm(None, None, None, None, 0, None, None, 4, 64, None, None) == 0
    good_a = [p(0), 1, 64, 6.0, p(512), p(1024), p(1536)]
    for i in (0, 4, 5, 6):
        a = list(good_a)
        a[i] = None
        assert act(*a) == -1 and b"null pointer" in L.vaa_last_error()
    assert act(p(0), -1, 64, 6.0, p(512), p(1024), p(1536)) == -1 and act(p(0), 1, 32, 6.0, p(512), p(1024), p(1536)) == -1
    for t in (-1.0, float("nan"), float("inf")):
        assert act(p(0), 1, 64, t, p(512), p(1024), p(1536)) == -1 and b"threshold" in L.vaa_last_error()
    assert act(p(0), 1, 96, 6.0, p(512), p(1024), p(1536)) == -2 and b"multiple of 64" in L.vaa_last_error()
    assert act(p(0), 1, 133184, 6.0, p(512), p(1024), p(1536)) == -2 and b"2^31" in L.vaa_last_error()
    for i, off in ((0, 8), (4, 520), (5, 1026), (6, 1538)):
        a = list(good_a)
        a[i] = p(off)
        assert act(*a) == -2 and b"aligned" in L.vaa_last_error()
    good_m = [p(0), p(512), p(1024), p(1536), 1, p(2048), p(2560), 4, 64, p(3072), p(3584)]
    assert mm(*good_m, form=3) == -1 and mm(*good_m, form=-1) == -1
    for i in (0, 1, 2, 3, 5, 6, 10):
        a = list(good_m)
        a[i] = None
        assert mm(*a) == -1 and b"null pointer" in L.vaa_last_error()
    for i, v in ((4, -1), (7, 0), (8, 32)):
        a = list(good_m)
        a[i] = v
        assert mm(*a) == -1
    a = list(good_m)
    a[8] = 96
    assert mm(*a) == -2
    a[8] = 133184
    assert mm(*a) == -2 and b"2^31" in L.vaa_last_error()
    a = list(good_m)
    a[4] = 17
    assert mm(*a, form=1) == -2 and b"at most 16" in L.vaa_last_error()
    for i, off in ((0, 8), (1, 514), (2, 1026), (3, 1544), (5, 2056), (6, 2562), (9, 3080), (10, 3592)):
        a = list(good_m)
        a[i] = p(off)
        assert mm(*a) == -2 and b"aligned" in L.vaa_last_error()


def test_quantize_llm_int8_on_the_tiny_model():
    import decode_ref
    from roboticattack_amd.openvla_model import build_openvla, tiny_cfg

    cfg = tiny_cfg()
    model = build_openvla(cfg, device="cpu", dtype=torch.bfloat16, seed=5)
    model.layers[0]._wt("q_proj")
    d, mlp = cfg.llm_dim, cfg.llm_mlp
    per_layer, rows_per_layer = 4 * d * d + 3 * d * mlp, 4 * d + 2 * mlp + d
    before = quant.llm_weight_bytes(model)
    others = {n: p.detach().clone() for n, p in model.named_parameters() if not n.startswith("layers.") or "layernorm" in n}
    ref_w = {(i, n): R.dequantise_w(*R.quantise_w(getattr(l, n).weight.float().numpy())) for i, l in enumerate(model.layers) for n in quant.PROJECTIONS}
    assert quant.quantize_llm(model, "int8", threshold=6.0) is model and model.quant_type == "int8"
    for i, layer in enumerate(model.layers):
        for n in quant.PROJECTIONS:
            lin = getattr(layer, n)
            assert isinstance(lin, quant.Q8Linear) and not hasattr(lin, "weight") and not list(lin.parameters()) and lin.threshold == 6.0
            assert lin.codes.dtype == torch.int8 and lin.wscale.dtype == torch.float32
            assert np.array_equal(lin.dequantize().float().numpy(), ref_w[(i, n)])  # each projection's own codes, fused or not
        assert isinstance(layer.q_proj, quant.Q8LinearRows) and layer.qkv_q8.out_features == 3 * d and layer.gate_up_q8.out_features == 2 * mlp
        assert not layer._wt_cache and layer.quant_type == "int8"
        assert sum(b.numel() * b.element_size() for b in layer.buffers()) == per_layer + rows_per_layer * 4  # codes + scales, held once
    after = quant.llm_weight_bytes(model)
    assert after == cfg.llm_layers * (per_layer + rows_per_layer * 4 + 2 * d * 2) and after < before
    now = dict(model.named_parameters())
    assert sorted(now) == sorted(others) and all(torch.equal(now[n], v) for n, v in others.items())
    assert isinstance(model.lm_head, torch.nn.Linear) and isinstance(model.fc1, torch.nn.Linear)
    ids = torch.randint(3, 1000, (1, 6))
    pix = torch.zeros((1, 6, 224, 224), dtype=torch.bfloat16)
    labels = torch.full((1, 6), -100)
    labels[0, 3:] = 31900
    x = torch.zeros((1, 4, d), dtype=torch.bfloat16)
    for call in (lambda: model(ids, pixel_values=pix, labels=labels), lambda: model.forward_rows(ids, pix, labels),
                 lambda: model.hidden_states(ids, pix), lambda: model.hidden_rows(ids, pix, model.label_row_index(labels)),
                 lambda: model.layers[0](x, None, None)):
        with pytest.raises(RuntimeError, match="int8 by quantize_llm"):
            call()
    with pytest.raises(ValueError, match="quantised already"):
        quant.quantize_llm(model, "int8")
    with pytest.raises(ValueError, match="threshold"):
        quant.quantize_llm(build_openvla(cfg, device="cpu", dtype=torch.bfloat16, seed=5), "int8", threshold=-1.0)
    batch = decode_ref.prompt_batch(2, (5, 8), torch.bfloat16)
    tokens, actions = model.predict_action(*batch)
    assert tuple(tokens.shape) == (2, 7) and torch.equal(tokens, model.predict_action(*batch)[0])
    # a layer call is q8_linear on each projection: the fused qkv rows are the three projections' own results
    h = _bf16(R.acts_case(3, d, 1, seed=6)[0])
    layer = model.layers[0]
    fused = quant.q8_linear(h, layer.qkv_q8)
    assert torch.equal(fused, torch.cat([layer.q_proj(h), layer.k_proj(h), layer.v_proj(h)], 1))


def test_eval_patch_parser_takes_the_int8_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "VLAAttacker"))
    try:
        import eval_patch
    finally:
        sys.path.pop(0)
    a = eval_patch.arg_parser(["--patch", "p.pt"])
    assert a.llm_int8 is False and a.llm_int8_threshold == 6.0
    a = eval_patch.arg_parser(["--patch", "p.pt", "--llm_int8", "--llm_int8_threshold", "4.5"])
    assert a.llm_int8 is True and a.llm_int8_threshold == 4.5 and a.load_in_4bit is False
    assert eval_patch.arg_parser(["--patch", "p.pt", "--llm_int8", "true"]).llm_int8 is True
    assert eval_patch.arg_parser(["--patch", "p.pt", "--llm_int8", "false"]).llm_int8 is False
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--llm_int8", "--load_in_4bit"])
    assert "exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--llm_int8", "--llm_int8_threshold", "-1"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--load_in_8bit"])
    err = capsys.readouterr().err
    assert "--load_in_8bit is not supported" in err and "--llm_int8" in err
