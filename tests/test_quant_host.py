"""The 4-bit path without a GPU: quant.quantize_q4 against quant_ref's exhaustive restatement (exact), the round-trip bound and the nibble
order, the argument guards of the two entry points, quantize_llm on tiny_cfg(), and the new flags of the eval_patch parser."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import quant_ref
from conftest import ROOT
from roboticattack_amd import _lib, quant

TABLE_NAMES = ("nf4", "fp4")
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _weights(shape, table, seed):
    """Random bf16 rows with the edge cases written into their blocks: an all-zero block, a block with a single non-zero element,
    negative zero, the largest finite bf16 (the tie rule has a test of its own below)."""
    N, K = shape
    rs = np.random.RandomState(seed)
    w = quant_ref.random_bf16(rs, (N, K), 0.05)
    w[0, :64] = 0.0                       # all-zero block
    w[0, 5] = -0.0
    if K >= 128:
        w[0, 64:128] = 0.0                # a single non-zero element
        w[0, 64 + 17] = -0.375
    w[N - 1, K - 1] = -0.0
    if N > 1:
        w[1, 3] = BF16_MAX                # the largest finite bf16 is its block's absmax
        w[1, 4] = -BF16_MAX
    return w


@pytest.mark.parametrize("name", TABLE_NAMES)
@pytest.mark.parametrize("shape", [(1, 64), (3, 128), (5, 192)])
def test_quantize_q4_equals_the_reference(name, shape):
    table = quant_ref.TABLES[name]
    assert np.array_equal(np.array(quant.TABLES[name], dtype=np.float32).view(np.uint32), table.view(np.uint32))  # incl. the sign of fp4's -0
    w = _weights(shape, table, seed=shape[0] * 1000 + shape[1])
    q, absmax = quant_ref.quantise(w, table)
    codes, am = quant.quantize_q4(_bf16(w), name)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (shape[0], shape[1] // 2)
    assert am.dtype == torch.float32 and tuple(am.shape) == (shape[0], shape[1] // 64)
    assert np.array_equal(am.numpy().view(np.uint32), absmax.view(np.uint32))
    assert np.array_equal(codes.numpy(), quant_ref.pack(q))
    zero = int(np.flatnonzero(table == 0)[0])
    assert (q[0, :64] == zero).all() and q[shape[0] - 1, shape[1] - 1] == zero  # the zero block, and negative zero
    # fp32 input of the same values and the custom-table spelling give the same codes
    c2, a2 = quant.quantize_q4(torch.from_numpy(w), [float(v) for v in table])
    assert torch.equal(c2, codes) and torch.equal(a2, am)
    # dequantize_q4 is the reference's wq, bit for bit
    wq = quant.dequantize_q4(codes, am, name)
    assert wq.dtype == torch.bfloat16
    assert np.array_equal(wq.view(torch.int16).numpy().view(np.uint16), quant_ref.f32_to_bf16_bits(quant_ref.dequantise(q, absmax, table)))


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_a_quotient_midway_between_two_entries_takes_the_smaller_index(name):
    """The tie rule. No midpoint of either table is a bf16 number (their entries are fp32 roundings of thirds, 192ths and normal quantiles),
    so a bf16 weight in a block of absmax 1 cannot sit on one; the fp32 spelling of W can: every midpoint that is an fp32 number goes into a
    block whose absmax is 1.0, where the quotient is the value itself. Also fp4's two zeros: 0 takes index 0, never index 8."""
    table = quant_ref.TABLES[name]
    t = np.sort(np.unique(table.astype(np.float64)))
    mids = [m for m in ((a + b) / 2 for a, b in zip(t[:-1], t[1:])) if float(np.float32(m)) == m]
    assert len(mids) >= 2
    w = np.zeros((2, 64), dtype=np.float32)
    w[0, 0] = 1.0
    w[0, 1:1 + len(mids)] = mids
    w[1] = w[0, ::-1]  # the same values on the other parity of the nibbles
    q, absmax = quant_ref.quantise(w, table)
    codes, am = quant.quantize_q4(torch.from_numpy(w), name)
    assert np.array_equal(codes.numpy(), quant_ref.pack(q)) and np.array_equal(am.numpy(), absmax)
    got = quant_ref.unpack(codes.numpy())
    for i, m in enumerate(mids):
        d = np.abs(table.astype(np.float64) - m)
        near = np.flatnonzero(d == d.min())
        assert len(near) >= 2 and got[0, 1 + i] == near.min() and got[1, 62 - i] == near.min()
        # one fp32 step to either side leaves the tie
        for v in (np.nextafter(np.float32(m), np.float32(2)), np.nextafter(np.float32(m), np.float32(-2))):
            w1 = w[:1].copy()
            w1[0, 1 + i] = v
            assert np.array_equal(quant.quantize_q4(torch.from_numpy(w1), name)[0].numpy(), quant_ref.pack(quant_ref.quantise(w1, table)[0]))
    assert got[0, 63] == int(np.flatnonzero(table == 0)[0])


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_round_trip_bound_and_nibble_order(name):
    table = quant_ref.TABLES[name]
    g = float(np.diff(np.sort(table.astype(np.float64))).max())  # the table's largest gap
    rs = np.random.RandomState(3)
    w = quant_ref.random_bf16(rs, (7, 256), 0.3)
    codes, am = quant.quantize_q4(_bf16(w), name)
    wq = quant.dequantize_q4(codes, am, name).double().numpy()
    absmax = np.repeat(am.double().numpy(), 64, axis=1)
    assert (np.abs(w.astype(np.float64) - wq) <= absmax * (g / 2) + 2.0 ** -8 * np.abs(wq)).all()
    # a hand-written 64-element row: 1.0, -1.0, then zeros with 0.5 at element 62 and -0.5 at element 63 (absmax 1: the quotient is the value)
    code = {"nf4": {1.0: 15, -1.0: 0, 0.0: 7}, "fp4": {1.0: 3, -1.0: 11, 0.0: 0, 0.5: 5, -0.5: 13}}[name]
    row = np.zeros((1, 64), dtype=np.float32)
    row[0, 0], row[0, 1] = 1.0, -1.0
    if name == "fp4":
        row[0, 62], row[0, 63] = 0.5, -0.5
    c, a = quant.quantize_q4(_bf16(row), name)
    want = [code[float(v)] for v in row[0]]
    assert c[0].tolist() == [(want[2 * i] << 4) | want[2 * i + 1] for i in range(32)]  # element 2i in the HIGH nibble
    assert c[0, 0].item() == (code[1.0] << 4 | code[-1.0]) and float(a[0, 0]) == 1.0
    hand = torch.tensor([[0x7F] + [0] * 31], dtype=torch.uint8)  # element 0 = code 7 (high nibble), element 1 = code 15
    wq = quant.dequantize_q4(hand, torch.tensor([[2.0]]), name).float()
    assert float(wq[0, 0]) == float(quant_ref.round_bf16(np.float32(table[7] * np.float32(2.0)))) and float(wq[0, 1]) == float(
        quant_ref.round_bf16(np.float32(table[15] * np.float32(2.0)))) and float(wq[0, 2]) == float(quant_ref.round_bf16(np.float32(table[0] * np.float32(2.0))))


def test_entry_point_guards_without_gpu():
    """NULL, K = 96, M = 17, M = 0 and a misaligned base: every one is answered before any launch (host buffers stand in for the operands)."""
    L = _lib.lib()
    raw = (ctypes.c_uint8 * 4096)()
    base = (ctypes.addressof(raw) + 63) // 64 * 64
    p = lambda off=0: ctypes.c_void_p(base + off)
    tab = _lib.f32x(quant.TABLES["nf4"])
    gemv = lambda x, M, c, a, N, K, res, y, t=tab: L.vaa_model_q4_gemv(x, M, c, a, t, N, K, res, y, None)
    deq = lambda c, a, N, K, out, t=tab: L.vaa_model_q4_dequant(c, a, t, N, K, out, None)
    assert _lib.MODEL_OP_EXPORTS[-2:] == ("vaa_model_q4_dequant", "vaa_model_q4_gemv")
    # M == 0: nothing to do, nothing validated
    assert gemv(None, 0, None, None, 4, 64, None, None) == 0
    # NULL pointers and sizes
    for args in ((None, 1, p(256), p(512), 4, 64, None, p(1024)), (p(), 1, None, p(512), 4, 64, None, p(1024)),
                 (p(), 1, p(256), None, 4, 64, None, p(1024)), (p(), 1, p(256), p(512), 4, 64, None, None)):
        assert gemv(*args) == -1 and b"null pointer" in L.vaa_last_error()
    assert L.vaa_model_q4_gemv(p(), 1, p(256), p(512), None, 4, 64, None, p(1024), None) == -1
    assert gemv(p(), -1, p(256), p(512), 4, 64, None, p(1024)) == -1
    assert gemv(p(), 1, p(256), p(512), 0, 64, None, p(1024)) == -1
    assert gemv(p(), 1, p(256), p(512), 4, 32, None, p(1024)) == -1
    assert deq(None, p(512), 4, 64, p(1024)) == -1 and deq(p(), None, 4, 64, p(1024)) == -1 and deq(p(), p(512), 4, 64, None) == -1
    assert L.vaa_model_q4_dequant(p(), p(512), None, 4, 64, p(1024), None) == -1
    assert deq(p(), p(512), 0, 64, p(1024)) == -1 and deq(p(), p(512), 4, 0, p(1024)) == -1
    # valid requests the kernels do not cover
    assert gemv(p(), 1, p(256), p(512), 4, 96, None, p(1024)) == -2 and b"multiple of the 64-element block" in L.vaa_last_error()
    assert deq(p(), p(512), 4, 96, p(1024)) == -2
    assert gemv(p(), 17, p(256), p(512), 4, 64, None, p(1024)) == -2 and b"at most 16" in L.vaa_last_error()
    for bad in range(5):  # x, codes, absmax, res, y: one misaligned base at a time
        ptrs = [p(0), p(256), p(512), p(768), p(1024)]
        ptrs[bad] = p(256 * bad + 8)
        assert gemv(ptrs[0], 1, ptrs[1], ptrs[2], 4, 64, ptrs[3], ptrs[4]) == -2 and b"16-byte aligned" in L.vaa_last_error()
    for bad in range(3):
        ptrs = [p(0), p(512), p(1024)]
        ptrs[bad] = p(512 * bad + 2)
        assert deq(ptrs[0], ptrs[1], 4, 64, ptrs[2]) == -2 and b"16-byte aligned" in L.vaa_last_error()
    with pytest.raises(_lib.VaaError):
        _lib.check(-2, "vaa_model_q4_gemv")
    # the host layer's own checks
    with pytest.raises(ValueError):
        quant.quantize_q4(torch.zeros(2, 96), "nf4")
    with pytest.raises(ValueError):
        quant.table_values("int4")
    with pytest.raises(ValueError):
        quant.table_values([0.0] * 15)


def _param_bytes(m):
    return sum(p.numel() * p.element_size() for p in m.parameters())


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_quantize_llm_on_the_tiny_model(name):
    from roboticattack_amd.openvla_model import build_openvla, tiny_cfg

    cfg = tiny_cfg()
    model = build_openvla(cfg, device="cpu", dtype=torch.bfloat16, seed=5)
    model.layers[0]._wt("q_proj")  # a cached transposed copy must not survive either
    d, mlp = cfg.llm_dim, cfg.llm_mlp
    per_layer = 4 * d * d + 3 * d * mlp  # elements of the seven projections
    before_all, before_llm = _param_bytes(model), sum(_param_bytes(l) for l in model.layers)
    others = {n: p.detach().clone() for n, p in model.named_parameters() if not n.startswith("layers.") or "layernorm" in n}
    wq = {(i, n): quant_ref.dequantise(*quant_ref.quantise(getattr(l, n).weight.float().numpy(), quant_ref.TABLES[name]), quant_ref.TABLES[name])
          for i, l in enumerate(model.layers) for n in quant.PROJECTIONS}
    assert quant.quantize_llm(model, name) is model and model.quant_type == name
    for i, layer in enumerate(model.layers):
        for n in quant.PROJECTIONS:
            lin = getattr(layer, n)
            assert isinstance(lin, quant.Q4Linear) and not hasattr(lin, "weight") and not list(lin.parameters())
            assert lin.codes.dtype == torch.uint8 and lin.absmax.dtype == torch.float32
            assert np.array_equal(lin.dequantize().float().numpy(), wq[(i, n)])  # each projection's own codes, fused or not
        assert not layer._wt_cache and layer.quant_type == name
        assert sorted(n for n, _ in layer.named_parameters()) == ["input_layernorm.weight", "post_attention_layernorm.weight"]
        assert sum(b.numel() * b.element_size() for b in layer.buffers()) == per_layer // 2 + per_layer // 64 * 4  # codes + scales, held once
    # no bf16 copy is left: the Llama stack's parameters are its norms, everything else keeps its bytes and its values
    assert sum(_param_bytes(l) for l in model.layers) == before_llm - cfg.llm_layers * per_layer * 2 == cfg.llm_layers * 2 * d * 2
    assert _param_bytes(model) == before_all - cfg.llm_layers * per_layer * 2
    assert quant.llm_weight_bytes(model) == cfg.llm_layers * (per_layer // 2 + per_layer // 64 * 4 + 2 * d * 2)
    now = dict(model.named_parameters())
    assert sorted(now) == sorted(others) and all(torch.equal(now[n], v) for n, v in others.items())
    assert isinstance(model.lm_head, torch.nn.Linear) and isinstance(model.fc1, torch.nn.Linear) and isinstance(model.featurizer.blocks[0].qkv, torch.nn.Linear)
    # the training entry points say what happened instead of failing on a missing attribute
    ids = torch.randint(3, 1000, (1, 6))
    pix = torch.zeros((1, 6, 224, 224), dtype=torch.bfloat16)
    labels = torch.full((1, 6), -100)
    labels[0, 3:] = 31900
    x = torch.zeros((1, 4, d), dtype=torch.bfloat16)
    for call in (lambda: model(ids, pixel_values=pix, labels=labels), lambda: model.forward_rows(ids, pix, labels),
                 lambda: model.hidden_states(ids, pix), lambda: model.hidden_rows(ids, pix, model.label_row_index(labels)),
                 lambda: model.layers[0](x, None, None)):
        with pytest.raises(RuntimeError, match="quantize_llm"):
            call()
    with pytest.raises(ValueError, match="quantised already"):
        quant.quantize_llm(model, name)
    # predict_action runs on the quantised model (the CPU formulation of the same graph) and equals the bf16 model carrying wq
    import decode_ref

    ref = build_openvla(cfg, device="cpu", dtype=torch.bfloat16, seed=5)
    with torch.no_grad():
        for i, layer in enumerate(ref.layers):
            for n in quant.PROJECTIONS:
                getattr(layer, n).weight.copy_(torch.from_numpy(wq[(i, n)]))
    batch = decode_ref.prompt_batch(2, (5, 8), torch.bfloat16)
    tq, tr = model.predict_action(*batch)[0], ref.predict_action(*batch)[0]
    assert tuple(tq.shape) == (2, 7) and torch.equal(tq, tr)


def test_eval_patch_parser_takes_the_quantisation_flags(capsys):
    sys.path.insert(0, os.path.join(ROOT, "VLAAttacker"))
    try:
        import eval_patch
    finally:
        sys.path.pop(0)
    a = eval_patch.arg_parser(["--patch", "p.pt"])
    assert a.load_in_4bit is False and a.load_in_8bit is False and a.bnb_4bit_quant_type == "fp4"
    a = eval_patch.arg_parser(["--patch", "p.pt", "--load_in_4bit", "--bnb_4bit_quant_type", "nf4"])
    assert a.load_in_4bit is True and a.bnb_4bit_quant_type == "nf4"
    assert eval_patch.arg_parser(["--patch", "p.pt", "--load_in_4bit", "True"]).load_in_4bit is True
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--bnb_4bit_quant_type", "int4"])
    with pytest.raises(SystemExit):
        eval_patch.arg_parser(["--patch", "p.pt", "--load_in_8bit"])
    assert "--load_in_8bit is not supported" in capsys.readouterr().err
