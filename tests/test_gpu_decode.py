"""vaa_model_attention_decode on the GPU against decode_ref's fp64 restatement, its exact properties (cache slot bits, untouched memory,
determinism, batch independence, the out-of-range guard), and the KV-cached predict_action against the no-cache one on tiny_cfg() in bf16."""
import pytest
import torch

import decode_ref
from decode_ref import DEV, RMS_FACTOR, RMS_FLOOR, SENTINEL16, TMAX

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.contiguous().view(torch.int16)


def _rotated_by_rope_kernel(k_new, pos, cos, sin):
    """vaa_model_rope's rotation of k_new [B,H,hd] at pos[b]: the rope kernel on [B,1,H,hd] with a one-row table per b."""
    from roboticattack_amd import model_ops

    return torch.stack([model_ops._rope_launch(k_new[b:b + 1, None], cos[p:p + 1].contiguous(), sin[p:p + 1].contiguous(), 1.0)[0, 0]
                        for b, p in enumerate(pos)])


def _storage_mask(view_shape, flat, slots=None):
    """bool over the flat storage of decode_ref.sentinel_view(view_shape): True at the elements the kernel may write — the whole view, or
    (slots: one cache slot per row, None = none) just those rows."""
    full = list(view_shape)
    full[1] += 3
    full[-1] += 8
    n = 1
    for s in full:
        n *= s
    own = torch.zeros(flat.numel(), dtype=torch.bool, device=DEV)
    m = own[:n].view(*full)
    if slots is None:
        m[:, :view_shape[1], ..., :view_shape[-1]] = True
    else:
        for b, p in enumerate(slots):
            if p is not None:
                m[b, p, :, :view_shape[-1]] = True
    return own


@pytest.mark.parametrize("c", decode_ref.cases(), ids=decode_ref.case_id)
def test_kernel_against_fp64(c):
    """o within the eager-bf16 yardstick's error of fp64; the cache slot, every other byte of the three storages, pos = 0 and a second run:
    exact."""
    H, hd, pos = c
    B = len(pos)
    inp, ref, (base_max, base_rms) = decode_ref.references(c)
    d = decode_ref.device_case(inp)
    k_before, v_before = d["fk"].clone(), d["fv"].clone()
    decode_ref.run_kernel(d)
    o = d["o"].cpu().double()
    err = o - ref["o"]
    mx, rms, ref_max = float(err.abs().max()), float(err.square().mean().sqrt()), float(ref["o"].abs().max())
    print("%s: o max %.3e rms %.3e | eager bf16 max %.3e rms %.3e" % (decode_ref.case_id(c), mx, rms, base_max, base_rms))
    assert bool(torch.isfinite(o).all())
    assert rms <= RMS_FACTOR * base_rms + RMS_FLOOR
    assert mx <= 2.0 ** -7 * ref_max + 1e-3
    # cache slot pos[b]: vaa_model_rope's bits of k_new, v_new unchanged
    rows = torch.arange(B, device=DEV)
    slot = torch.tensor(pos, device=DEV)
    assert torch.equal(_bits(d["kc"][rows, slot]), _bits(_rotated_by_rope_kernel(d["k"], pos, d["cos"], d["sin"])))
    assert torch.equal(_bits(d["vc"][rows, slot]), _bits(d["v"]))
    # every other element of the cache storages (earlier keys, later slots, padding columns, slack rows) keeps its bits
    may = _storage_mask((B, TMAX, H, hd), d["fk"], slots=pos)
    assert torch.equal(d["fk"][~may], k_before[~may]) and torch.equal(d["fv"][~may], v_before[~may])
    # nothing written around the o view
    assert bool((d["fo"][~_storage_mask((B, H, hd), d["fo"])] == SENTINEL16).all())
    # a row at position 0 sees one key: o = v_new
    for b, p in enumerate(pos):
        if p == 0:
            assert torch.equal(_bits(d["o"][b]), _bits(d["v"][b]))
    # the same arguments give the same bits (the second run appends the same slot again)
    o1 = d["o"].clone()
    decode_ref.run_kernel(d)
    assert torch.equal(_bits(d["o"]), _bits(o1))


@pytest.mark.parametrize("H,hd", decode_ref.HEADS)
def test_batch_equals_its_rows_one_at_a_time(H, hd):
    for pos in decode_ref.POS_ROWS:
        inp = decode_ref.references((H, hd, pos))[0]
        d = decode_ref.device_case(inp)
        decode_ref.run_kernel(d)
        for b, p in enumerate(pos):
            one = decode_ref.device_case({k: (v[b:b + 1] if k in ("qkv", "kc", "vc", "pos") else v) for k, v in inp.items()})
            decode_ref.run_kernel(one)
            assert torch.equal(_bits(one["o"][0]), _bits(d["o"][b]))
            assert torch.equal(_bits(one["kc"][0]), _bits(d["kc"][b])) and torch.equal(_bits(one["vc"][0]), _bits(d["vc"][b]))


def test_wrapper_matches_the_raw_call_and_the_stock_formulation(monkeypatch):
    """model_ops.attention_decode: the kernel by default (the raw call's bits), the stock formulation under VAA_NO_FUSED_ATTENTION=1 (within
    the kernel test's bound of fp64)."""
    from roboticattack_amd import model_ops

    c = (5, 128, (63, 256, 0))
    inp, ref, (_, base_rms) = decode_ref.references(c)
    d = decode_ref.device_case(inp)
    decode_ref.run_kernel(d)
    monkeypatch.delenv("VAA_NO_FUSED_ATTENTION", raising=False)
    monkeypatch.delenv("VAA_NO_FUSED_MODEL_OPS", raising=False)
    w = decode_ref.device_case(inp)
    o = model_ops.attention_decode(w["q"], w["k"], w["v"], w["kc"], w["vc"], w["pos"], w["cos"], w["sin"])
    assert torch.equal(_bits(o), _bits(d["o"])) and torch.equal(w["fk"], d["fk"]) and torch.equal(w["fv"], d["fv"])
    monkeypatch.setenv("VAA_NO_FUSED_ATTENTION", "1")
    s = decode_ref.device_case(inp)
    os_ = model_ops.attention_decode(s["q"], s["k"], s["v"], s["kc"], s["vc"], s["pos"], s["cos"], s["sin"])
    rms = float((os_.cpu().double() - ref["o"]).square().mean().sqrt())
    assert rms <= RMS_FACTOR * base_rms + RMS_FLOOR
    rows, slot = torch.arange(3, device=DEV), torch.tensor(c[2], device=DEV)
    assert torch.equal(_bits(s["vc"][rows, slot]), _bits(s["v"]))


def test_out_of_range_pos_is_skipped_and_reported():
    """pos = -1 and pos = Tmax: the launch succeeds, those rows' o is zero and their caches keep every bit, the failure word reports the new
    code once, and the row between them is what it is alone. (The guard doing its job: no memory outside the views is touched.)"""
    from roboticattack_amd import _lib, ops

    ops.async_error_check()
    for H, hd in ((5, 128), (3, 16)):
        inp = decode_ref.make_inputs((H, hd, (-1, 64, TMAX)))
        d = decode_ref.device_case(inp)
        k_before, v_before = d["fk"].clone(), d["fv"].clone()
        rc = decode_ref.c_decode(d["q"], d["k"], d["v"], d["kc"], d["vc"], d["pos"], d["cos"], d["sin"], d["o"])
        assert rc == 0
        torch.cuda.synchronize()
        with pytest.raises(_lib.VaaError, match="vaa_model_attention_decode met a pos outside"):
            ops.async_error_check()
        ops.async_error_check()  # reported once: the poll cleared the word
        assert bool((d["o"][0] == 0).all()) and bool((d["o"][2] == 0).all())
        may = _storage_mask((3, TMAX, H, hd), d["fk"], slots=(None, 64, None))
        assert torch.equal(d["fk"][~may], k_before[~may]) and torch.equal(d["fv"][~may], v_before[~may])
        assert bool((d["fo"][~_storage_mask((3, H, hd), d["fo"])] == SENTINEL16).all())
        one = decode_ref.device_case({k: (v[1:2] if k in ("qkv", "kc", "vc", "pos") else v) for k, v in inp.items()})
        decode_ref.run_kernel(one)
        assert torch.equal(_bits(one["o"][0]), _bits(d["o"][1])) and torch.equal(_bits(one["kc"][0]), _bits(d["kc"][1]))
        ref = decode_ref.ref_fp64(inp)
        assert float((d["o"][1].cpu().double() - ref["o"][1]).abs().max()) <= 2.0 ** -7 * float(ref["o"][1].abs().max()) + 1e-3


# ---------------------------------------------------------------- model level ----------------------------------------------------------------
# Seed chosen on a CPU run of the stock routes in bf16 (decode_ref.tiny_model + prompt_batch): the no-cache logits' smallest top-2 margin over
# the 3 x 7 steps is 1.09e-1 there and the cached stock route differs from the no-cache one by 1.56e-2 (one bf16 ulp of a logit of magnitude
# ~4), so 2 x tolerance = 6.25e-2 excludes no step.
MODEL_SEED = 13


def _decode(model, batch, no_cache):
    from roboticattack_amd import predict

    t, l = predict.greedy_decode(model, *batch, 7, no_cache=no_cache)
    torch.cuda.synchronize()
    return t.cpu(), l.cpu()


@pytest.fixture(scope="module")
def tiny():
    model = decode_ref.tiny_model(MODEL_SEED, torch.bfloat16, DEV)
    batch = decode_ref.prompt_batch(MODEL_SEED, (5, 9, 12), torch.bfloat16, DEV)
    return model, batch


def _agree(name, ta, la, tn, ln, tol):
    """Logits within tol wherever the two decodings answered the same question; tokens equal at every step whose no-cache margin exceeds
    2 x tol; at most one of the 21 steps excluded."""
    same = decode_ref.same_prefix(ta, tn)
    diff = float((la - ln).abs().amax(-1)[same].max())
    decided = decode_ref.top2_margin(ln) > 2 * tol
    print("%s: max |logit difference| %.4e (tolerance %.4e), %d of %d steps excluded by the margin rule, tokens differ at %d steps"
          % (name, diff, tol, int((~decided).sum()), decided.numel(), int((ta != tn).sum())))
    assert diff <= tol
    assert int((~decided).sum()) <= 1
    assert torch.equal(ta[decided], tn[decided])


def test_cached_kernel_route_matches_no_cache(tiny, monkeypatch):
    """B = 3, prompts of 5 / 9 / 12 tokens, bf16. The no-cache route is ONE thing here: action_dim full forward calls in the default
    environment. Tolerance = 2 x the measured difference between the cached STOCK route (VAA_NO_FUSED_ATTENTION=1: the stock formulation of
    attention_decode in place of the kernel) and that no-cache route on the same inputs; the cached kernel route's per-step logits must be
    within it of the same no-cache logits, tokens equal wherever the no-cache margin exceeds 2 x tolerance, at most 1 of 21 steps excluded.
    Also printed, not asserted on: the same difference with both routes under VAA_NO_FUSED_MODEL_OPS=1 (stock ops throughout) — on an
    MI355X that one is exactly 0 for this model (the stock bf16 ops give the two routes the same bits), which is why it cannot serve as a
    tolerance for a route that keeps the softmax in fp32.
    Measured on an MI355X: cached stock route vs no-cache 1.5625e-2 (one bf16 ulp of a logit in [2, 4)) -> tolerance 3.125e-2; cached kernel
    route vs no-cache 3.125e-2 (one ulp of a logit in [4, 8)); smallest no-cache top-2 margin 1.094e-1; no step excluded, all 21 tokens equal."""
    model, batch = tiny
    for k in ("VAA_NO_FUSED_MODEL_OPS", "VAA_NO_FUSED_ATTENTION", "VAA_PREDICT_NO_CACHE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VAA_NO_FUSED_MODEL_OPS", "1")
    ts, ls = _decode(model, batch, False)
    tns, lns = _decode(model, batch, True)
    monkeypatch.delenv("VAA_NO_FUSED_MODEL_OPS")
    print("stock ops throughout, cached vs no-cache: max |logit difference| %.4e (information only)"
          % float((ls - lns).abs().amax(-1)[decode_ref.same_prefix(ts, tns)].max()))
    tn, ln = _decode(model, batch, True)       # the no-cache route: action_dim full forward calls (the training kernels)
    monkeypatch.setenv("VAA_NO_FUSED_ATTENTION", "1")
    ta, la = _decode(model, batch, False)      # the cached stock route: stock attention_decode (and SDPA prefill)
    monkeypatch.delenv("VAA_NO_FUSED_ATTENTION")
    stock_diff = float((la - ln).abs().amax(-1)[decode_ref.same_prefix(ta, tn)].max())
    tol = 2 * stock_diff
    print("cached stock route vs no-cache route: max |logit difference| %.4e -> tolerance %.4e; smallest no-cache top-2 margin %.4e"
          % (stock_diff, tol, float(decode_ref.top2_margin(ln).min())))
    tk, lk = _decode(model, batch, False)      # the cached kernel route
    _agree("cached kernel route", tk, lk, tn, ln, tol)
    _agree("cached stock route (VAA_NO_FUSED_ATTENTION=1)", ta, la, tn, ln, tol)
    decided = decode_ref.top2_margin(ln) > 2 * tol
    assert torch.equal(ta[decided], tk[decided])
    # the public method returns the cached kernel route's tokens and their bin centres
    from roboticattack_amd import predict

    tokens, actions = model.predict_action(*batch)
    assert torch.equal(tokens.cpu(), tk) and torch.equal(actions, predict.tokens_to_actions(tk))
