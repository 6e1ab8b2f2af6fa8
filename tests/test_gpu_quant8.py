"""The int8 kernels on the GPU against quant8_ref: vaa_model_q8_act_quant bit for bit (codes, row scales, the outlier count and list),
vaa_model_q8_matmul bit for bit against the fp32 restatement and within the derived bound of fp64, their fixed properties (untouched memory,
determinism, row independence at t = 0, the two matmul forms agreeing), predict_action on an int8 tiny model through the kernels against
the torch formulation of the same arithmetic, and evaluate_patch with an int8 quant_model."""
import copy

import numpy as np
import pytest
import torch

import decode_ref
import quant8_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = 0x7B
PAD = 64  # canary bytes on each side of an output (a multiple of 16: the view stays 16-byte aligned)


def _dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _guarded(n, dtype):
    """(flat uint8 storage filled with the canary, the n-element view of `dtype` in its middle)."""
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    flat = torch.full((nbytes + 2 * PAD,), CANARY, dtype=torch.uint8, device=DEV)
    return flat, flat[PAD:PAD + nbytes].view(dtype)


def _intact(flat):
    return bool((flat[:PAD] == CANARY).all()) and bool((flat[-PAD:] == CANARY).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _act_raw(dx, t):
    """The raw entry point on outputs with canaries around each: (xq int8 [M,K], ascale [M], outliers int32 [K+1], canaries intact)."""
    from roboticattack_amd import _lib

    M, K = dx.shape
    fx, xq = _guarded(M * K, torch.int8)
    fa, ascale = _guarded(M, torch.float32)
    fo, outl = _guarded(K + 1, torch.int32)
    _lib.check(_lib.lib().vaa_model_q8_act_quant(dx.data_ptr(), M, K, float(t), xq.data_ptr(), ascale.data_ptr(), outl.data_ptr(), _stream()),
               "vaa_model_q8_act_quant")
    torch.cuda.synchronize()
    return xq.view(M, K), ascale, outl, _intact(fx) and _intact(fa) and _intact(fo)


def _matmul_raw(xq, ascale, outl, dx, dq, dws, dres, form=0):
    from roboticattack_amd import _lib

    (M, K), N = dx.shape, dq.shape[0]
    fy, y = _guarded(M * N, torch.bfloat16)
    _lib.check(_lib.lib().vaa_model_q8_matmul(xq.data_ptr(), ascale.data_ptr(), outl.data_ptr(), dx.data_ptr(), M, dq.data_ptr(), dws.data_ptr(), N, K,
                                              dres.data_ptr() if dres is not None else None, y.data_ptr(), form, _stream()), "vaa_model_q8_matmul")
    torch.cuda.synchronize()
    return y.view(M, N), _intact(fy)


def _act_equal(got, want):
    """Device (xq, ascale, outliers) against the restatement's (xq, ascale, idx): every bit, the count and the list."""
    xq, ascale, outl = got[:3]
    rq, ra, idx = want
    o = outl.cpu().numpy()
    return (np.array_equal(xq.cpu().numpy(), rq) and np.array_equal(ascale.cpu().numpy().view(np.uint32), ra.view(np.uint32))
            and int(o[0]) == idx.size and np.array_equal(o[1:1 + idx.size], idx))


@pytest.mark.parametrize("t", [0.0, 6.0])
@pytest.mark.parametrize("shape", [(1, 64), (3, 128), (16, 1088), (17, 64), (80, 192)])
def test_act_quant_is_the_reference_bit_for_bit(shape, t):
    """M <= 16 is the one-launch form, 17 and 80 the three-launch form (80 = 5 row lanes of the flag kernel); K = 1088 is 136 column vectors,
    not a multiple of the 16 a flag workgroup owns nor of the 256 threads of a row workgroup. Data without outliers, with one outlier column
    (its largest entry exactly 6.0), with five, and with every column an outlier."""
    M, K = shape
    for n_out in (0, 1, 5, -1):
        x, _ = R.acts_case(M, K, n_out, seed=11)
        want = R.act_quant(x, t)
        assert want[2].size == (0 if t == 0 else (K if n_out < 0 else n_out))
        dx = _dev_bf16(x)
        got = _act_raw(dx, t)
        assert got[3] and _act_equal(got, want)
        again = _act_raw(dx, t)
        assert again[3] and torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]) and _act_equal(again, want)


def _check_matmul(M, N, K, n_out, with_res, seed=0, t=6.0, big=False):
    q, ws = R.weights_case(N, K, seed)
    x, res = R.acts_case(M, K, n_out, seed, N=N)
    if big:
        x, ws = R.big_scales(x, ws)
    r = res if with_res else None
    want = R.act_quant(x, t)
    bits = R.y32_bits(x, *want, q, ws, r)
    ref = R.y64(x, *want, q, ws, r)
    bound = R.bound(x, *want, q, ws, r)
    dx, dq, dws = _dev_bf16(x), torch.from_numpy(q).to(DEV), torch.from_numpy(ws).to(DEV)
    dres = _dev_bf16(r) if with_res else None
    act = _act_raw(dx, t)
    assert act[3] and _act_equal(act, want)
    y, intact = _matmul_raw(*act[:3], dx, dq, dws, dres)
    got = _bits(y)
    err = np.abs(R.bf16_bits_to_f32(got).astype(np.float64) - ref)
    print("q8 matmul M=%d N=%d K=%d outliers=%d res=%d: %d of %d elements differ from the restatement, max err/bound %.3f"
          % (M, N, K, want[2].size, int(with_res), int((got != bits).sum()), got.size, float((err / np.maximum(bound, 1e-300)).max())))
    assert intact
    assert np.array_equal(got, bits)
    assert (err <= bound).all()
    y2, intact2 = _matmul_raw(*act[:3], dx, dq, dws, dres)
    assert intact2 and np.array_equal(_bits(y2), got)  # the same arguments give the same bits
    return dx, dq, dws, dres, act, y


@pytest.mark.parametrize("n_out", [0, 1, 5])
@pytest.mark.parametrize("K", [64, 128, R.GEMV_CHUNK_K + 64])
def test_matmul_bit_for_bit_and_against_fp64(K, n_out):
    """Both forms (M <= 16: split-K; 17, 33, 80: the tiled GEMM, one and two 64-row tiles of m with a ragged one) against the fp32 restatement,
    bit for bit, and within quant8_ref.bound of fp64. N = 17 and 33 are one more than whole 16-row tiles, 272 is two 128-row GEMM tiles plus a
    16-row tile; K = 1088 is one round of the split-K workgroup's 8 waves x 128 elements plus a ragged tile (64 of 128) in the second round."""
    for M in (1, 2, 7, 16, 17, 33, 80):
        for N in (1, 17, 33, 272):
            for with_res in (False, True):
                _check_matmul(M, N, K, n_out, with_res)


def test_matmul_at_a_7b_row_length():
    """M = 8, N = 256, K = 11008 (down_proj's K: 86 tiles over 8 waves, an uneven split; |acc| reaches 2^27), five outlier columns, with and
    without res; the same call through the GEMM form gives the same bits."""
    for with_res in (False, True):
        dx, dq, dws, dres, act, y = _check_matmul(8, 256, 11008, 5, with_res, seed=1)
        y2, intact = _matmul_raw(*act[:3], dx, dq, dws, dres, form=2)
        assert intact and np.array_equal(_bits(y2), _bits(y))


def test_scale_order_and_every_column_an_outlier():
    """Activations of 2^118 against weight scales of 2^-118 at t = 0 (float(acc) * ascale would overflow: the scales are multiplied first),
    and a call whose every column is an outlier (the integer part is 0, the whole product is the bf16 sum) in both forms."""
    for M in (7, 33):
        _check_matmul(M, 33, 192, 5, True, seed=4, t=0.0, big=True)
        _check_matmul(M, 33, 128, -1, True, seed=5)


def test_rows_are_independent_without_the_outlier_split():
    """t = 0: row m of an M-row call equals the M = 1 call of that row, bit for bit, from either form (with a threshold the outlier columns
    are a property of the whole call, so this holds at t = 0 only)."""
    for M in (8, 33):
        dx, dq, dws, dres, act, y = _check_matmul(M, 33, 1088, 5, True, seed=2, t=0.0)
        for m in (0, 5, M - 2):
            x1, r1 = dx[m:m + 1].clone(), dres[m:m + 1].clone()  # copies: a row of res starts at a multiple of 66 bytes, not of 16
            a1 = _act_raw(x1, 0.0)
            one, intact = _matmul_raw(*a1[:3], x1, dq, dws, r1)
            assert a1[3] and intact and np.array_equal(_bits(one[0]), _bits(y[m]))


@pytest.mark.parametrize("n_out", [0, 5])
def test_the_two_matmul_forms_agree(n_out, monkeypatch):
    """The same 16-row call through the split-K form and through the tiled GEMM: the same bits, at the entry point (form 1 against form 2) and
    through q8_linear with the row limit monkeypatched to 0."""
    from roboticattack_amd import quant

    for N, K in ((33, 192), (272, 1088)):
        dx, dq, dws, dres, act, y = _check_matmul(16, N, K, n_out, True, seed=3)
        y1, i1 = _matmul_raw(*act[:3], dx, dq, dws, dres, form=1)
        y2, i2 = _matmul_raw(*act[:3], dx, dq, dws, dres, form=2)
        assert i1 and i2 and np.array_equal(_bits(y1), _bits(y)) and np.array_equal(_bits(y2), _bits(y))
        lin = quant.Q8Linear(dq, dws, 6.0)
        a = quant.q8_linear(dx, lin, dres)
        monkeypatch.setattr(quant, "Q8_GEMV_MAX_ROWS", 0)
        b = quant.q8_linear(dx, lin, dres, scratch=quant.Q8Scratch())
        monkeypatch.undo()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(a), _bits(y)) and np.array_equal(_bits(b), _bits(y))
        monkeypatch.setattr(quant, "Q8_TORCH_ROUTE", True)  # and the torch formulation on the GPU
        c = quant.q8_linear(dx, lin, dres)
        monkeypatch.undo()
        assert np.array_equal(_bits(c), _bits(y))


# ---------------------------------------------------------------- model level ----------------------------------------------------------------
# The seed was chosen on a CPU run of the int8 tiny model alone, through q8_linear's torch formulation (decode_ref.tiny_model(seed) converted with
# MODEL_THRESHOLD, prompt_batch(seed), bf16, stock ops; seeds 1 .. 40 scanned). With logits of magnitude 4 .. 8 one ulp is 3.125e-2, so a step
# is excluded when its top-2 margin is <= 6.25e-2. MODEL_THRESHOLD is 3.0, not 6.0: the tiny model's normalised activations rarely reach 6, and
# at 3.0 most calls carry outlier columns, so the model test runs the outlier sum as well.
# Smallest top-2 margins of that CPU run at seed 25 (largest |logit| 4.3 / 4.5): B = 1 1.5625e-1, B = 3 9.375e-2 — no step of either run is
# excluded, and one step of the B = 3 run lies between 6.25e-2 and 1.25e-1. (Seed 38 was the only other seed of the 40 without an excluded step.)
MODEL_SEED = 25
MODEL_THRESHOLD = 3.0


def _decode(model, batch, no_cache=False):
    from roboticattack_amd import predict

    t, l = predict.greedy_decode(model, *batch, 7, no_cache=no_cache)
    torch.cuda.synchronize()
    return t.cpu(), l.cpu()


def test_predict_action_on_the_int8_model(monkeypatch):
    """predict_action on the int8 tiny model through the kernels against the same model through q8_linear's torch formulation on the GPU (the
    route monkeypatched), by the margin rule of test_gpu_quant.py: tolerance = the larger of one bf16 ulp of the largest logit and the
    difference between the bf16 model's cached and no-cache routes measured in the same run; logits within it wherever both answered the same
    question, tokens equal wherever the reference's top-2 margin exceeds 2 x tolerance, at most 1 step excluded. B = 1 (decode steps of one
    row, the prefill through the GEMM form) and B = 3 with lens (5, 9, 12)."""
    from roboticattack_amd import quant

    for k in ("VAA_NO_FUSED_MODEL_OPS", "VAA_NO_FUSED_ATTENTION", "VAA_PREDICT_NO_CACHE"):
        monkeypatch.delenv(k, raising=False)
    bf = decode_ref.tiny_model(MODEL_SEED, torch.bfloat16, DEV)
    q = quant.quantize_llm(copy.deepcopy(bf), "int8", threshold=MODEL_THRESHOLD)
    for lens in ((7,), (5, 9, 12)):
        batch = decode_ref.prompt_batch(MODEL_SEED, lens, torch.bfloat16, DEV)
        tb, lb = _decode(bf, batch)
        tn, ln = _decode(bf, batch, no_cache=True)
        monkeypatch.setattr(quant, "Q8_TORCH_ROUTE", True)
        tr, lr = _decode(q, batch)
        monkeypatch.undo()
        ulp = 2.0 ** (int(np.floor(np.log2(float(lr.abs().max())))) - 7)
        route = float((lb - ln).abs().amax(-1)[decode_ref.same_prefix(tb, tn)].max())
        tol = max(ulp, route)
        tq, lq = _decode(q, batch)
        same = decode_ref.same_prefix(tq, tr)
        diff = float((lq - lr).abs().amax(-1)[same].max())
        decided = decode_ref.top2_margin(lr) > 2 * tol
        print("int8 B=%d: one logit ulp %.4e, bf16 cached vs no-cache %.4e -> tolerance %.4e; max |logit difference| %.4e, smallest top-2 margin "
              "of the torch route %.4e, %d of %d steps excluded, tokens differ at %d"
              % (len(lens), ulp, route, tol, diff, float(decode_ref.top2_margin(lr).min()), int((~decided).sum()), decided.numel(), int((tq != tr).sum())))
        assert decided.numel() == 7 * len(lens)
        assert diff <= tol
        assert int((~decided).sum()) <= 1
        assert torch.equal(tq[decided], tr[decided])
        tokens, actions = q.predict_action(*batch)
        assert torch.equal(tokens.cpu(), tq)


def test_evaluate_patch_reports_the_int8_model():
    """Four synthetic frames, two placements, bs = 3: the report holds the bf16 model's and the int8 model's rates, quant_type reads "int8",
    and clean_agreement equals what a hand-composed loop over predict_action gives (the same batches: an int8 call's outlier columns and a
    bf16 GEMM's rounding both depend on the batch)."""
    import eval_ref
    from roboticattack_amd import quant
    from roboticattack_amd.attack.evaluate import evaluate_patch, summarise
    from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
    from roboticattack_amd.transform import RandomPatchTransform

    mean, std = [MEAN0, MEAN1], [STD0, STD1]
    t = RandomPatchTransform(DEV)
    model = decode_ref.tiny_model(4, torch.bfloat16, DEV)
    qmodel = quant.quantize_llm(copy.deepcopy(model), "int8", threshold=MODEL_THRESHOLD)
    ids, mask, _ = decode_ref.prompt_batch(11, lens=(5, 9, 12, 9), device=DEV)
    fr = eval_ref.frames("smooth", batch=4, seed=9)
    patch = torch.rand((3, 50, 50), generator=torch.Generator().manual_seed(1))
    placements = [(True, 10.0, 0.1, 0.1, 0, 0), (False, 0.0, 0.0, 0.0, 87, 60)]
    F, P, bs = 4, 2, 3
    rep = evaluate_patch(model, t, fr, ids, mask, patch, placements, center_crop=True, crop_scale=0.9, mean=mean, std=std, bs=bs, quant_model=qmodel)
    assert rep["quantised"]["quant_type"] == "int8"
    clean = {0: [], 1: []}
    frames = t.stage_images(torch.as_tensor(np.asarray(fr)))
    for i in range(0, F, bs):
        rows = torch.arange(i, min(i + bs, F), device=DEV)
        pix = t.eval_pixel_values(frames[rows], mean, std, True, 0.9)
        for j, m in enumerate((model, qmodel)):
            clean[j].append(m.predict_action(ids[rows], mask[rows], pix)[0].cpu())
    c0, c1 = torch.cat(clean[0]), torch.cat(clean[1])
    assert torch.equal(rep["tokens_clean"], c0) and torch.equal(rep["quantised"]["tokens_clean"], c1)
    same = c0 == c1
    assert rep["clean_agreement"] == {"frames": float(same.all(1).double().mean()), "tokens": float(same.double().mean())}
    for r, c in ((rep, c0), (rep["quantised"], c1)):
        assert tuple(r["tokens_patched"].shape) == (P, F, 7) and len(r["per_placement"]) == P
        s = summarise(c, r["tokens_patched"])
        assert r["overall"]["any_flip_rate"] == s["overall"]["any_flip_rate"] and torch.equal(r["overall"]["token_flip_rate"], s["overall"]["token_flip_rate"])
    plain = evaluate_patch(model, t, fr, ids, mask, patch, placements[:1], center_crop=True, crop_scale=0.9, mean=mean, std=std, bs=bs)
    assert "quantised" not in plain and "clean_agreement" not in plain and torch.equal(plain["tokens_clean"], c0)
    assert sorted(plain) == sorted(k for k in rep if k not in ("quantised", "clean_agreement"))  # the keys it always had
