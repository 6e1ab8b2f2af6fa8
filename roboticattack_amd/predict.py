"""Greedy action decoding (inference only): what the reference's evaluation calls `vla.predict_action(..., do_sample=False)`
(prismatic/extern/hf/modeling_prismatic.py:506-536) — insert the empty token 29871 behind the prompt, decode `action_dim` tokens greedily,
each conditioned on the model's own earlier choices, map them to bins in [-1, 1] and un-normalise with the dataset statistics.

Two routes compute the same tokens:
  cached    towers + projector once, one prefill of the Llama stack that fills a KV cache [layers][B,Tmax,H,hd], then action_dim - 1 decode
            steps of one token per row (LlamaLayer.decode_step -> model_ops.attention_decode: one launch per layer and step);
  no cache  VAA_PREDICT_NO_CACHE=1: action_dim full `forward` calls on the growing sequence — the yardstick and the escape hatch.
Rows are right-padded and may have different lengths; row b's multimodal sequence is [BOS, 256 image tokens, text 1 .. len_b-1], so its last
prompt position is 256 + len_b - 1 and decode step s (s = 0 .. action_dim-2) runs at position 256 + len_b + s.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from .action_tokenizer import ActionTokenizer
from .constants import N_IMG_TOKENS, PAD_ID

EMPTY_TOKEN_ID = 29871  # the '' token the prompts of the training data carry behind "OUT:" (modeling_prismatic.py:512)


def insert_empty_token(input_ids: torch.Tensor, attention_mask: torch.Tensor):
    """Per row: if the last REAL token is not 29871, put 29871 behind it (at column len[b], not at the padded end). Returns (ids [B,L+1],
    lens [B]); the added column holds PAD_ID where a row needs nothing. No host synchronisation."""
    B, L = input_ids.shape
    lens = attention_mask.to(torch.int64).sum(1)
    last = input_ids.gather(1, (lens - 1).clamp_min(0)[:, None])[:, 0]
    need = last != EMPTY_TOKEN_ID
    ids = torch.cat([input_ids, torch.full((B, 1), PAD_ID, dtype=input_ids.dtype, device=input_ids.device)], dim=1)
    at = lens[:, None]
    ids.scatter_(1, at, torch.where(need[:, None], torch.full_like(at, EMPTY_TOKEN_ID).to(ids.dtype), ids.gather(1, at)))
    return ids, lens + need.to(torch.int64)


def greedy_argmax(logits: torch.Tensor) -> torch.Tensor:
    """argmax over the last axis with the LOWEST index winning a tie (torch.argmax leaves the choice among equal maxima open)."""
    V = logits.shape[-1]
    idx = torch.arange(V, device=logits.device)
    best = torch.where(logits == logits.max(-1, keepdim=True).values, idx, V).min(-1).values
    return best.clamp_max(V - 1)  # a row of NaNs matches nothing: stay inside the vocabulary


def unnormalize_actions(normalized: np.ndarray, unnorm_stats=None) -> np.ndarray:
    """0.5 * (a + 1) * (q99 - q01) + q01 where `mask` is set, a unchanged elsewhere (modeling_prismatic.py:527-534); no mask = all set."""
    if unnorm_stats is None:
        return normalized
    low, high = np.asarray(unnorm_stats["q01"], dtype=np.float64), np.asarray(unnorm_stats["q99"], dtype=np.float64)
    mask = np.asarray(unnorm_stats.get("mask", np.ones_like(low, dtype=bool)), dtype=bool)
    return np.where(mask, 0.5 * (normalized + 1) * (high - low) + low, normalized)


def tokens_to_actions(tokens: torch.Tensor, unnorm_stats=None) -> torch.Tensor:
    """Token ids [B,action_dim] -> bin centres in [-1, 1] (action_tokenizer) -> un-normalised actions, float64 [B,action_dim] on the CPU."""
    normalized = ActionTokenizer().decode_token_ids_to_actions(tokens.cpu().numpy())
    return torch.from_numpy(np.asarray(unnormalize_actions(normalized, unnorm_stats), dtype=np.float64))


def _multimodal_embeds(model, input_ids, pixel_values):
    """[B, 256 + L, D]: [BOS, projected patch tokens of the two towers, text 1 .. L-1] (the front end of OpenVLAShaped.hidden_states)."""
    in0, in1 = torch.split(pixel_values, [3, 3], dim=1)
    f0, f1 = model._towers(in0, in1, False)
    proj = model.fc3(F.gelu(model.fc2(F.gelu(model.fc1(torch.cat([f0, f1], dim=2))))))
    emb = model.embed_tokens(input_ids)
    return torch.cat([emb[:, :1], proj.to(emb.dtype), emb[:, 1:]], dim=1)


def _head(model, x):
    return model.lm_head(model.norm(x)).float()


@torch.no_grad()
def greedy_cached(model, ids, lens, pixel_values, action_dim: int):
    """(tokens int64 [B,action_dim], logits float32 [B,action_dim,V]) through the KV cache. ids/lens: insert_empty_token's."""
    cfg = model.cfg
    B, L = ids.shape
    H, hd = cfg.llm_heads, cfg.llm_dim // cfg.llm_heads
    x = _multimodal_embeds(model, ids, pixel_values)
    T = x.shape[1]
    Tmax = N_IMG_TOKENS + L + action_dim  # >= 256 + max len + action_dim: every decode position 256 + len + s is a slot
    rope_tab = model._rope_tables(Tmax, x.device, x.dtype)[2]
    # zeros, not empty: the stock decode formulation multiplies the masked slots' values by a zero weight
    caches = [(torch.zeros((B, Tmax, H, hd), dtype=x.dtype, device=x.device), torch.zeros((B, Tmax, H, hd), dtype=x.dtype, device=x.device))
              for _ in model.layers]
    for layer, cache in zip(model.layers, caches):
        x = layer.prefill(x, rope_tab, cache)
    last = (N_IMG_TOKENS + lens - 1)[:, None, None].expand(B, 1, x.shape[-1])
    logits = [_head(model, x.gather(1, last)[:, 0])]
    tokens = [greedy_argmax(logits[0])]
    pos0 = (N_IMG_TOKENS + lens).to(torch.int32)
    for s in range(action_dim - 1):
        pos = pos0 + s
        x = model.embed_tokens(tokens[-1])[:, None]
        for layer, cache in zip(model.layers, caches):
            x = layer.decode_step(x, pos, rope_tab, cache)
        logits.append(_head(model, x[:, 0]))
        tokens.append(greedy_argmax(logits[-1]))
    return torch.stack(tokens, 1), torch.stack(logits, 1)


@torch.no_grad()
def greedy_no_cache(model, ids, lens, pixel_values, action_dim: int):
    """The same decoding as action_dim full `forward` calls on the growing right-padded sequence (no state kept between the steps)."""
    B, L = ids.shape
    seq = torch.cat([ids, torch.full((B, action_dim - 1), PAD_ID, dtype=ids.dtype, device=ids.device)], dim=1)
    tokens, logits = [], []
    for s in range(action_dim):
        full = model.forward(seq, pixel_values=pixel_values).logits  # [B, 256 + L + action_dim - 1, V]
        at = (N_IMG_TOKENS + lens - 1 + s)[:, None, None].expand(B, 1, full.shape[-1])
        logits.append(full.gather(1, at)[:, 0])
        tokens.append(greedy_argmax(logits[-1]))
        if s + 1 < action_dim:
            seq.scatter_(1, (lens + s)[:, None], tokens[-1][:, None].to(seq.dtype))
    return torch.stack(tokens, 1), torch.stack(logits, 1)


def greedy_decode(model, input_ids, attention_mask, pixel_values, action_dim: int = 7, no_cache: bool | None = None):
    """insert_empty_token, then the cached or (no_cache / VAA_PREDICT_NO_CACHE=1) the no-cache route: (tokens, per-step logits)."""
    if no_cache is None:
        no_cache = os.environ.get("VAA_PREDICT_NO_CACHE", "0") not in ("", "0")
    ids, lens = insert_empty_token(input_ids, attention_mask)
    return (greedy_no_cache if no_cache else greedy_cached)(model, ids, lens, pixel_values, int(action_dim))
