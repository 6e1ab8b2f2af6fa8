"""The 4-bit kernels on the GPU against quant_ref: vaa_model_q4_dequant bit for bit, vaa_model_q4_gemv within a derived bound of fp64 plus its
exact properties (determinism, row independence, untouched memory), the two routes of q4_linear, predict_action on a quantised tiny model
against a bf16 copy that carries the same dequantised weights, and evaluate_patch with both models."""
import copy

import numpy as np
import pytest
import torch

import decode_ref
import quant_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TABLE_NAMES = ("nf4", "fp4")
CANARY = 0x7B7B
PAD = 64  # canary elements on each side of an output (a multiple of 8: the view stays 16-byte aligned)


def _dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _guarded(n):
    """(flat int16 storage filled with the canary, the n-element bf16 view in its middle)."""
    flat = torch.full((n + 2 * PAD,), CANARY, dtype=torch.int16, device=DEV)
    return flat, flat[PAD:PAD + n].view(torch.bfloat16)


def _canary_intact(flat, n):
    return bool((flat[:PAD] == CANARY).all()) and bool((flat[PAD + n:] == CANARY).all())


def _gemv_raw(x, codes, absmax, name, res, M, N, K):
    """The raw entry point on an output with canaries around it: (y bf16 [M,N] on the device, canary intact)."""
    from roboticattack_amd import _lib, quant

    flat, y = _guarded(M * N)
    rc = _lib.lib().vaa_model_q4_gemv(x.data_ptr(), M, codes.data_ptr(), absmax.data_ptr(), _lib.f32x(quant.TABLES[name]), N, K,
                                      res.data_ptr() if res is not None else None, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "vaa_model_q4_gemv")
    torch.cuda.synchronize()
    return y.view(M, N), _canary_intact(flat, M * N)


@pytest.mark.parametrize("name", TABLE_NAMES)
@pytest.mark.parametrize("shape", [(1, 64), (17, 128), (272, 192)])
def test_dequant_kernel_is_the_reference_bit_for_bit(name, shape):
    from roboticattack_amd import _lib, quant

    N, K = shape
    table = quant_ref.TABLES[name]
    _, codes, absmax, wq, _ = quant_ref.gemv_case(1, N, K, table, seed=3)
    c, a = torch.from_numpy(codes).to(DEV), torch.from_numpy(absmax).to(DEV)
    flat, out = _guarded(N * K)
    rc = _lib.lib().vaa_model_q4_dequant(c.data_ptr(), a.data_ptr(), _lib.f32x(quant.TABLES[name]), N, K, out.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "vaa_model_q4_dequant")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.view(N, K)), quant_ref.f32_to_bf16_bits(wq))
    assert _canary_intact(flat, N * K)
    assert np.array_equal(_bits(quant.q4_dequant(c, a, name)), quant_ref.f32_to_bf16_bits(wq))  # the host layer's call
    assert np.array_equal(_bits(quant.dequantize_q4(c, a, name)), quant_ref.f32_to_bf16_bits(wq))  # and the torch formulation on the GPU


def _check_gemv(name, M, N, K, with_res, seed=0):
    table = quant_ref.TABLES[name]
    x, codes, absmax, wq, res = quant_ref.gemv_case(M, N, K, table, seed)
    ref = quant_ref.y64(x, wq, res if with_res else None)
    bound = quant_ref.gemv_bound(x, wq, ref)
    dx, dc, da = _dev_bf16(x), torch.from_numpy(codes).to(DEV), torch.from_numpy(absmax).to(DEV)
    dr = _dev_bf16(res) if with_res else None
    y, intact = _gemv_raw(dx, dc, da, name, dr, M, N, K)
    err = np.abs(y.double().cpu().numpy() - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("gemv %s M=%d N=%d K=%d res=%d: max |err| %.3e, max err/bound %.3f" % (name, M, N, K, int(with_res), float(err.max()), worst))
    assert intact
    assert bool(torch.isfinite(y.float()).all()) and (err <= bound).all()
    if M > 1 and not with_res:  # the all-zero row of x
        assert bool((y[-1].float() == 0).all())
    y2, intact2 = _gemv_raw(dx, dc, da, name, dr, M, N, K)
    assert intact2 and np.array_equal(_bits(y2), _bits(y))  # the same arguments give the same bits
    return dx, dc, da, dr, y


@pytest.mark.parametrize("name", TABLE_NAMES)
@pytest.mark.parametrize("K", [64, 128, quant_ref.GEMV_CHUNK_K + 64])
def test_gemv_against_fp64(name, K):
    """Every element within 2^-8 |y64| + K 2^-23 sum |x wq| of fp64. N = 17 and 33 are one more than a whole number of the 16 rows a workgroup
    owns; K = 1088 is one round of the workgroup's 8 waves plus a ragged tile (64 of 128 elements) in the second round."""
    for M in (1, 2, 7, 8, 16):
        for N in (1, 17, 33, 272):
            for with_res in (False, True):
                _check_gemv(name, M, N, K, with_res)


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_gemv_at_a_7b_row_length_and_row_independence(name):
    """M = 8, N = 256, K = 11008 (down_proj's K: 86 tiles over 8 waves, an uneven split). Rows 0 and 5 of the M = 8 call equal the same rows
    run as M = 1 calls, bit for bit, with and without res."""
    for with_res in (False, True):
        dx, dc, da, dr, y = _check_gemv(name, 8, 256, 11008, with_res, seed=1)
        for m in (0, 5):
            one, intact = _gemv_raw(dx[m:m + 1].contiguous(), dc, da, name, dr[m:m + 1].contiguous() if with_res else None, 1, 256, 11008)
            assert intact and np.array_equal(_bits(one[0]), _bits(y[m]))


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_both_routes_of_a_tiny_layer_against_fp64(name):
    """The four projection shapes of one tiny_cfg() layer (qkv 192x64, o 64x64, gate+up 256x64, down 64x128) at M = 3: the GEMV and dequant +
    stock GEMM (through a scratch smaller than the fused groups, so the row-range loop runs) are each within the GEMV bound of fp64."""
    from roboticattack_amd import quant
    from roboticattack_amd.openvla_model import tiny_cfg

    cfg = tiny_cfg()
    d, mlp = cfg.llm_dim, cfg.llm_mlp
    scratch = quant.Q4Scratch(mlp * d)
    table = quant_ref.TABLES[name]
    for N, K, with_res in ((3 * d, d, False), (d, d, True), (2 * mlp, d, False), (d, mlp, True)):
        x, codes, absmax, wq, res = quant_ref.gemv_case(3, N, K, table, seed=2)
        ref = quant_ref.y64(x, wq, res if with_res else None)
        bound = quant_ref.gemv_bound(x, wq, ref)
        lin = quant.Q4Linear(torch.from_numpy(codes).to(DEV), torch.from_numpy(absmax).to(DEV), name)
        dx, dr = _dev_bf16(x), (_dev_bf16(res) if with_res else None)
        for gemv in (True, False):
            y = quant.q4_linear(dx, lin, dr, scratch, gemv)
            torch.cuda.synchronize()
            err = np.abs(y.double().cpu().numpy() - ref)
            print("%s N=%d K=%d %s: max err/bound %.3f" % (name, N, K, "gemv" if gemv else "dequant+gemm", float((err / bound.clip(1e-300)).max())))
            assert tuple(y.shape) == (3, N) and (err <= bound).all()


# ---------------------------------------------------------------- model level ----------------------------------------------------------------
# Seeds chosen on a CPU run of the bf16 copy alone (decode_ref.tiny_model(seed) with every Llama projection replaced by its dequantised weight,
# prompt_batch(seed), bf16, stock ops; seeds 1 .. 89 scanned, one seed per table because the bf16 copy differs with the table). With logits of
# magnitude 4 .. 8 one ulp is 3.125e-2, so a step is excluded when its top-2 margin is <= 6.25e-2. Smallest no-cache margins of the CPU run:
#   nf4, seed 25: B = 1 6.25e-2 (that one step excluded, the next margin is above 1.25e-1), B = 3 7.81e-2 (none excluded)
#   fp4, seed 40: B = 1 1.875e-1, B = 3 1.094e-1 (none excluded)
# and the cached route differed from the no-cache route by 1.56e-2 at most in all four runs.
MODEL_SEEDS = {"nf4": 25, "fp4": 40}


def _models(name):
    """(quantised model, bf16 copy carrying the same dequantised weights), both on the device."""
    from roboticattack_amd import quant

    ref = decode_ref.tiny_model(MODEL_SEEDS[name], torch.bfloat16, DEV)
    q = quant.quantize_llm(copy.deepcopy(ref), name)
    with torch.no_grad():
        for lq, lr in zip(q.layers, ref.layers):
            for n in quant.PROJECTIONS:
                getattr(lr, n).weight.copy_(getattr(lq, n).dequantize())
    return q, ref


def _decode(model, batch, no_cache=False):
    from roboticattack_amd import predict

    t, l = predict.greedy_decode(model, *batch, 7, no_cache=no_cache)
    torch.cuda.synchronize()
    return t.cpu(), l.cpu()


def _agree(what, tq, lq, tr, lr, tol, steps):
    same = decode_ref.same_prefix(tq, tr)
    diff = float((lq - lr).abs().amax(-1)[same].max())
    decided = decode_ref.top2_margin(lr) > 2 * tol
    print("%s: max |logit difference| %.4e (tolerance %.4e), smallest top-2 margin of the bf16 copy %.4e, %d of %d steps excluded, tokens differ at %d"
          % (what, diff, tol, float(decode_ref.top2_margin(lr).min()), int((~decided).sum()), decided.numel(), int((tq != tr).sum())))
    assert decided.numel() == steps
    assert diff <= tol
    assert int((~decided).sum()) <= 1
    assert torch.equal(tq[decided], tr[decided])


@pytest.mark.parametrize("name", TABLE_NAMES)
def test_predict_action_on_the_quantised_model(name, monkeypatch):
    """predict_action on the quantised tiny model against the bf16 copy whose Llama weights are the same wq, by the margin rule of
    test_gpu_decode.py: tolerance = the larger of one bf16 ulp of the largest logit and the difference between the bf16 copy's cached and
    no-cache routes measured in the same run; logits within it wherever both answered the same question, tokens equal wherever the bf16
    copy's top-2 margin exceeds 2 x tolerance, at most 1 of the 21 steps (B = 3; 7 at B = 1) excluded. B = 1 and B = 3 through the GEMV, and
    B = 3 again through dequant + GEMM with the row limit monkeypatched to 0.
    The seeds and the margins they gave on the CPU run of the bf16 copy are recorded next to MODEL_SEEDS."""
    from roboticattack_amd import quant

    for k in ("VAA_NO_FUSED_MODEL_OPS", "VAA_NO_FUSED_ATTENTION", "VAA_PREDICT_NO_CACHE"):
        monkeypatch.delenv(k, raising=False)
    q, ref = _models(name)
    for lens in ((7,), (5, 9, 12)):
        batch = decode_ref.prompt_batch(MODEL_SEEDS[name], lens, torch.bfloat16, DEV)
        tr, lr = _decode(ref, batch)
        tn, ln = _decode(ref, batch, no_cache=True)
        ulp = 2.0 ** (int(np.floor(np.log2(float(lr.abs().max())))) - 7)
        route = float((lr - ln).abs().amax(-1)[decode_ref.same_prefix(tr, tn)].max())
        tol = max(ulp, route)
        print("B=%d: one logit ulp %.4e, bf16 copy cached vs no-cache %.4e -> tolerance %.4e" % (len(lens), ulp, route, tol))
        tq, lq = _decode(q, batch)
        _agree("%s B=%d gemv" % (name, len(lens)), tq, lq, tr, lr, tol, 7 * len(lens))
        tokens, actions = q.predict_action(*batch)
        assert torch.equal(tokens.cpu(), tq)
        if len(lens) == 3:
            monkeypatch.setattr(quant, "GEMV_MAX_ROWS", 0)
            td, ld = _decode(q, batch)
            monkeypatch.undo()
            _agree("%s B=3 dequant + gemm" % name, td, ld, tr, lr, tol, 21)


def test_evaluate_patch_reports_both_models():
    """Four synthetic frames, two placements, bs = 3: the report holds the bf16 model's and the quantised model's rates, and clean_agreement
    equals what a hand-composed loop over predict_action gives (the same batches: a bf16 GEMM's rounding may depend on its batch)."""
    import eval_ref
    from roboticattack_amd import quant
    from roboticattack_amd.attack.evaluate import evaluate_patch, summarise
    from roboticattack_amd.constants import MEAN0, MEAN1, STD0, STD1
    from roboticattack_amd.transform import RandomPatchTransform

    mean, std = [MEAN0, MEAN1], [STD0, STD1]
    t = RandomPatchTransform(DEV)
    model = decode_ref.tiny_model(4, torch.bfloat16, DEV)
    qmodel = quant.quantize_llm(copy.deepcopy(model), "nf4")
    ids, mask, _ = decode_ref.prompt_batch(11, lens=(5, 9, 12, 9), device=DEV)
    fr = eval_ref.frames("smooth", batch=4, seed=9)
    patch = torch.rand((3, 50, 50), generator=torch.Generator().manual_seed(1))
    placements = [(True, 10.0, 0.1, 0.1, 0, 0), (False, 0.0, 0.0, 0.0, 87, 60)]
    F, P, bs = 4, 2, 3
    rep = evaluate_patch(model, t, fr, ids, mask, patch, placements, center_crop=True, crop_scale=0.9, mean=mean, std=std, bs=bs, quant_model=qmodel)
    assert rep["quantised"]["quant_type"] == "nf4"
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
    # without a quantised model the report has the keys it always had
    plain = evaluate_patch(model, t, fr, ids, mask, patch, placements[:1], center_crop=True, crop_scale=0.9, mean=mean, std=std, bs=bs)
    assert "quantised" not in plain and "clean_agreement" not in plain and torch.equal(plain["tokens_clean"], c0)
