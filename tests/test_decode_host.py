"""CPU-only: the decode entry point's argument rules, predict_action's host logic (29871 insertion, un-normalisation) and, on tiny_cfg() in
fp32, the KV-cached greedy decoding against the no-cache one (the stock formulations: the host layer runs them wherever the kernel does not apply)."""
import ctypes

import numpy as np
import pytest
import torch

import decode_ref
from roboticattack_amd import _lib, model_ops, predict
from roboticattack_amd.constants import N_IMG_TOKENS, PAD_ID


def test_library_exports_the_decode_symbol():
    assert "vaa_model_attention_decode" in _lib.MODEL_OP_EXPORTS
    assert hasattr(_lib.lib(), "vaa_model_attention_decode")


def _call(hd=128, B=1, H=2, Tmax=8, scale=0.1, null=None):
    """The entry point on host buffers: every case below returns before a launch."""
    L = _lib.lib()
    bufs = [ctypes.create_string_buffer(64) for _ in range(9)]
    s2, s3 = (ctypes.c_int64 * 2)(H * hd, hd), (ctypes.c_int64 * 3)(Tmax * H * hd, H * hd, hd)
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    args = dict(q=p[0], q_str=s2, k_new=p[1], k_str=s2, v_new=p[2], v_str=s2, kcache=p[3], kc_str=s3, vcache=p[4], vc_str=s3, pos=p[5], cos=p[6],
                sin=p[7], o=p[8], o_str=s2)
    if null:
        args[null] = None
    return L.vaa_model_attention_decode(*args.values(), B, H, Tmax, hd, scale, None)


def test_argument_rules_without_gpu():
    L = _lib.lib()
    assert _call(B=0) == 0
    for name in ("q", "k_new", "v_new", "kcache", "vcache", "pos", "cos", "sin", "o", "q_str", "kc_str", "o_str"):
        assert _call(null=name) == -1
        msg = L.vaa_last_error()
        assert b"null pointer" in msg and ("(%s)" % name).encode() in msg, msg
    for hd in (8, 32, 64, 96, 256):
        assert _call(hd=hd) == -2 and b"head width" in L.vaa_last_error()
    assert _call(B=-1) == -1 and _call(H=0) == -1 and _call(Tmax=0) == -1
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert _call(scale=scale) == -1 and b"scale" in L.vaa_last_error()


def test_empty_token_is_inserted_at_each_rows_length():
    ids = torch.tensor([[1, 50, 60, 29871, PAD_ID, PAD_ID],   # already ends in 29871: unchanged, len stays 4
                        [1, 51, 61, 71, 81, 91],              # full row: 29871 goes into the new column
                        [1, PAD_ID, PAD_ID, PAD_ID, PAD_ID, PAD_ID],  # length 1: 29871 at column 1
                        [1, 52, 29871, 62, PAD_ID, PAD_ID]])  # 29871 inside, not at the end: inserted at column 4
    mask = (ids != PAD_ID).long()
    out, lens = predict.insert_empty_token(ids, mask)
    assert lens.tolist() == [4, 7, 2, 5]
    assert out.tolist() == [[1, 50, 60, 29871, PAD_ID, PAD_ID, PAD_ID],
                            [1, 51, 61, 71, 81, 91, 29871],
                            [1, 29871, PAD_ID, PAD_ID, PAD_ID, PAD_ID, PAD_ID],
                            [1, 52, 29871, 62, 29871, PAD_ID, PAD_ID]]
    # a batch of one that ends in 29871 (the reference's un-padded case)
    out1, lens1 = predict.insert_empty_token(torch.tensor([[1, 7, 29871]]), torch.ones(1, 3, dtype=torch.long))
    assert lens1.tolist() == [3] and out1[0, :3].tolist() == [1, 7, 29871]


def test_unnormalisation_is_the_references_formula():
    rs = np.random.RandomState(3)
    tokens = torch.from_numpy(rs.randint(31744, 32000, size=(4, 7)))
    tokens[0, 0], tokens[0, 1], tokens[1, 0] = 31744, 31999, 5  # both ends of the action range and a non-action token (clipped like the reference)
    stats = dict(q01=rs.uniform(-2, 0, 7).tolist(), q99=rs.uniform(0.5, 3, 7).tolist(), mask=[True, True, False, True, True, True, False])
    got = predict.tokens_to_actions(tokens, stats).numpy()
    # modeling_prismatic.py:521-534 restated literally
    bins = np.linspace(-1, 1, 256)
    bin_centers = (bins[:-1] + bins[1:]) / 2.0
    discretized_actions = 32000 - tokens.numpy()
    discretized_actions = np.clip(discretized_actions - 1, a_min=0, a_max=bin_centers.shape[0] - 1)
    normalized_actions = bin_centers[discretized_actions]
    mask = np.array(stats["mask"])
    action_high, action_low = np.array(stats["q99"]), np.array(stats["q01"])
    want = np.where(mask, 0.5 * (normalized_actions + 1) * (action_high - action_low) + action_low, normalized_actions)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, ~mask], normalized_actions[:, ~mask]) and not np.array_equal(got[:, mask], normalized_actions[:, mask])
    assert np.array_equal(predict.tokens_to_actions(tokens).numpy(), normalized_actions)  # no statistics: the bin centres
    no_mask = predict.tokens_to_actions(tokens, dict(q01=stats["q01"], q99=stats["q99"])).numpy()
    assert np.array_equal(no_mask, 0.5 * (normalized_actions + 1) * (action_high - action_low) + action_low)


def test_greedy_argmax_takes_the_lowest_index_of_a_tie():
    x = torch.tensor([[0.0, 3.0, 1.0, 3.0], [2.0, 2.0, 2.0, 2.0], [-1.0, -5.0, -1.0, -0.5]])
    assert predict.greedy_argmax(x).tolist() == [1, 0, 3]


def test_stock_decode_step_matches_the_fp64_restatement():
    """model_ops.attention_decode on CPU tensors is the stock formulation: fp32 against decode_ref's fp64 graph, out-of-range rows included."""
    inp = decode_ref.make_inputs((3, 16, (5, -1, decode_ref.TMAX, 0, 319)))
    ref = decode_ref.ref_fp64(inp)
    qkv, kc, vc = inp["qkv"].float(), inp["kc"].float(), inp["vc"].float()
    o = model_ops.attention_decode(qkv[:, 0], qkv[:, 1], qkv[:, 2], kc, vc, inp["pos"], inp["cos"], inp["sin"])
    assert float((o.double() - ref["o"]).abs().max()) < 1e-5
    assert float((kc.double() - ref["kc"]).abs().max()) < 1e-6 and torch.equal(vc.double(), ref["vc"])
    assert bool((o[1] == 0).all()) and bool((o[2] == 0).all())
    assert torch.equal(kc[1], inp["kc"][1].float()) and torch.equal(kc[2], inp["kc"][2].float())


# seed -> smallest top-2 margin of the no-cache logits over the 3 x 7 steps (fp32, this model and these prompts; measured when the seeds
# were chosen): 13 -> 4.6e-3, 22 -> 6.6e-2, 7 -> 1.9e-2. The two routes' logits differ by <= 1.9e-6 there (logits of magnitude ~5).
@pytest.mark.parametrize("seed", [13, 22, 7])
def test_cached_tokens_equal_no_cache_tokens_fp32(seed, monkeypatch):
    monkeypatch.delenv("VAA_PREDICT_NO_CACHE", raising=False)
    model = decode_ref.tiny_model(seed, torch.float32)
    ids, mask, pix = decode_ref.prompt_batch(seed)
    tc, lc = predict.greedy_decode(model, ids, mask, pix, 7, no_cache=False)
    tn, ln = predict.greedy_decode(model, ids, mask, pix, 7, no_cache=True)
    margin = decode_ref.top2_margin(ln)
    print("seed %d: min top-2 margin %.3e, max |cached - no-cache| logit %.3e" % (seed, float(margin.min()), float((lc - ln).abs().max())))
    assert float(margin.min()) > 1e-3
    assert torch.equal(tc, tn)
    assert float((lc - ln).abs().max()) < 1e-4
    # the public method: the same tokens by either route, actions = the tokens' bin centres
    tokens, actions = model.predict_action(ids, mask, pix)
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (3, 7) and torch.equal(tokens, tc)
    assert torch.equal(actions, predict.tokens_to_actions(tc)) and tuple(actions.shape) == (3, 7)
    monkeypatch.setenv("VAA_PREDICT_NO_CACHE", "1")
    assert torch.equal(model.predict_action(ids, mask, pix)[0], tn)


def test_decode_positions_follow_each_rows_length(monkeypatch):
    """Decode step s runs row b at position 256 + len[b] + s (len after the 29871 insertion), and nothing is written behind a row's last
    step: the cache slots past both the prefill and 256 + len[b] + action_dim - 2 are still zero."""
    model = decode_ref.tiny_model(13, torch.float32)
    ids, mask, pix = decode_ref.prompt_batch(13)
    seen = []
    orig = model_ops.attention_decode

    def spy(q, k_new, v_new, kcache, vcache, pos, *a, **k):
        seen.append((pos.tolist(), kcache))
        return orig(q, k_new, v_new, kcache, vcache, pos, *a, **k)

    monkeypatch.setattr(model_ops, "attention_decode", spy)
    predict.greedy_decode(model, ids, mask, pix, 7, no_cache=False)
    lens = [6, 10, 13]  # 5, 9, 12 + the inserted 29871
    layers = len(model.layers)
    assert [p for p, _ in seen[::layers]] == [[N_IMG_TOKENS + n + s for n in lens] for s in range(6)]
    kc = seen[-1][1]
    T = N_IMG_TOKENS + 13  # the prefill's (padded) length
    assert kc.shape[1] == T + 7
    for b, n in enumerate(lens):
        assert bool((kc[b, max(T, N_IMG_TOKENS + n + 6):] == 0).all()) and bool((kc[b, N_IMG_TOKENS + n + 5] != 0).any())
