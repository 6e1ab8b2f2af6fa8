"""What the decode tests share (a plain module, not a conftest): an fp64 restatement of vaa_model_attention_decode (RoPE at pos, cache
append, masked softmax attention), the eager bf16 formulation of the same graph (the error yardstick, in the style of attention_ref.py), the
kernel cases, the raw C call on caller-owned views, and the tiny model + prompts of the model-level checks.

Bound on o (the convention of attention_ref.py, constants taken from there and not tuned against the kernel):
    rms(kernel - fp64) <= RMS_FACTOR * rms(eager bf16 - fp64) + RMS_FLOOR        and        max error <= 2^-7 max|ref| + 1e-3
Both sides see q and k_new rotated AND rounded to bf16 and round o once; the eager side also rounds q.k and P, the kernel keeps them in fp32.
"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from attention_ref import BF, DEV, RMS_FACTOR, RMS_FLOOR, SENTINEL16, _rope, _round_bf16  # noqa: E402,F401

TMAX = 320
POS_EDGES = (0, 1, 63, 64, 65, 255, 256, 319)  # first slot, one key in the cache, around the 64-key round of the hd = 128 groups, last slot
HEADS = ((1, 128), (5, 128), (3, 16))          # (H, hd): one head, more heads than waves, the tiny model's width
POS_ROWS = ((0, 64, 319), (1, 65, 255), (63, 256, 0))  # B = 3: different per row


def cases():
    """(H, hd, pos tuple): B = 3 with mixed rows and B = 1 at every edge, for every head shape."""
    return [(H, hd, p) for H, hd in HEADS for p in POS_ROWS + tuple((e,) for e in POS_EDGES)]


def case_id(c):
    return "H%d_hd%d_pos%s" % (c[0], c[1], "-".join(str(p) for p in c[2]))


def rope_tables(T, hd):
    ang = torch.outer(torch.arange(T, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd)))
    return ang.cos().contiguous(), ang.sin().contiguous()


def make_inputs(c, seed=0):
    """CPU tensors: qkv bf16 [B,3,H,hd] (q, k_new, v_new are its slices), kc / vc bf16 [B,TMAX,H,hd] random in the slots below pos[b] (what
    earlier steps left) and zero elsewhere, pos int32 [B], cos / sin float32 [TMAX, hd/2]."""
    H, hd, pos = c
    B = len(pos)
    g = torch.Generator().manual_seed(seed * 1000003 + H * 131 + hd * 7 + sum((i + 1) * (p + 2) for i, p in enumerate(pos)))
    qkv = torch.randn((B, 3, H, hd), generator=g).to(BF)
    kc, vc = torch.randn((B, TMAX, H, hd), generator=g).to(BF), torch.randn((B, TMAX, H, hd), generator=g).to(BF)
    live = torch.arange(TMAX)[None, :] < torch.tensor(pos)[:, None].clamp(0, TMAX)
    kc, vc = kc * live[:, :, None, None], vc * live[:, :, None, None]
    cos, sin = rope_tables(TMAX, hd)
    return dict(qkv=qkv, kc=kc, vc=vc, pos=torch.tensor(pos, dtype=torch.int32), cos=cos, sin=sin)


def _graph(inp, dtype, rnd):
    """o [B,H,hd] and the appended caches; rnd = identity (fp64) or one bf16 rounding where the eager bf16 formulation has one. A row whose
    pos is outside [0, TMAX) gets o = 0 and keeps its caches."""
    qkv, pos = inp["qkv"].to(dtype), inp["pos"].tolist()
    B, _, H, hd = qkv.shape
    kc, vc = inp["kc"].to(dtype).clone(), inp["vc"].to(dtype).clone()
    o = torch.zeros((B, H, hd), dtype=dtype)
    scale = float(hd) ** -0.5
    for b, p in enumerate(pos):
        if not 0 <= p < TMAX:
            continue
        cs, sn = inp["cos"][p:p + 1], inp["sin"][p:p + 1]
        q = rnd(_rope(qkv[b:b + 1, 0][:, None], cs, sn))[0, 0]   # [H,hd]
        k = rnd(_rope(qkv[b:b + 1, 1][:, None], cs, sn))[0, 0]
        kc[b, p], vc[b, p] = k, qkv[b, 2]
        keys, vals = kc[b, :p + 1].permute(1, 0, 2), vc[b, :p + 1].permute(1, 0, 2)  # [H,p+1,hd]
        s = rnd(torch.einsum("hd,htd->ht", q, keys)) * scale
        o[b] = rnd(torch.einsum("ht,htd->hd", rnd(torch.softmax(s, -1)), vals))
    return dict(o=o.double(), kc=kc.double(), vc=vc.double())


def ref_fp64(inp):
    return _graph(inp, torch.float64, lambda x: x)


def eager_bf16(inp):
    """bf16 q.k, fp32 softmax, P cast to bf16, bf16 P.V: each bf16 product as the fp32 product of the bf16 values rounded once."""
    return _graph(inp, torch.float32, _round_bf16)


_REFS = {}


def references(c):
    """(inputs, fp64 reference, (max, rms) error of the eager bf16 o against it), computed once per case and process and left unchanged."""
    k = case_id(c)
    if k not in _REFS:
        inp = make_inputs(c)
        ref = ref_fp64(inp)
        d = eager_bf16(inp)["o"] - ref["o"]
        _REFS[k] = (inp, ref, (float(d.abs().max()), float(d.square().mean().sqrt())))
    return _REFS[k]


# ---------------------------------------------------------------- the kernel ----------------------------------------------------------------
def _strs(x, n):
    assert x.stride(-1) == 1
    return (ctypes.c_int64 * n)(*x.stride()[:n])


def c_decode(q, k_new, v_new, kcache, vcache, pos, cos, sin, o, scale=None):
    """vaa_model_attention_decode on caller-owned views; returns the entry point's code."""
    from roboticattack_amd import _lib

    B, H, hd = q.shape
    scale = float(hd) ** -0.5 if scale is None else scale
    return _lib.lib().vaa_model_attention_decode(q.data_ptr(), _strs(q, 2), k_new.data_ptr(), _strs(k_new, 2), v_new.data_ptr(), _strs(v_new, 2),
                                                 kcache.data_ptr(), _strs(kcache, 3), vcache.data_ptr(), _strs(vcache, 3), pos.data_ptr(),
                                                 cos.data_ptr(), sin.data_ptr(), o.data_ptr(), _strs(o, 2), B, H, kcache.shape[1], hd, float(scale),
                                                 torch.cuda.current_stream().cuda_stream)


def sentinel_view(shape, slack_rows=130):
    """A view of `shape` (last dim hd) inside a sentinel-filled buffer whose rows are hd + 8 wide and whose second axis has 3 spare entries,
    followed by slack_rows more sentinel rows; and the flat int16 storage (attention_ref._sentinel_view for any rank >= 3)."""
    full = list(shape)
    full[1] += 3
    full[-1] += 8
    n = 1
    for s in full:
        n *= s
    flat = torch.full((n + slack_rows * full[-1],), SENTINEL16, dtype=torch.int16, device=DEV)
    view = flat[:n].view(BF).view(*full)
    return view[(slice(None), slice(0, shape[1])) + (slice(None),) * (len(shape) - 3) + (slice(0, shape[-1]),)], flat


def device_case(inp):
    """The case on the device: q / k_new / v_new as slices of one packed buffer, the caches and o as views of sentinel-filled storage (slots
    below pos[b] hold the case's keys and values, everything else the sentinel)."""
    B, _, H, hd = inp["qkv"].shape
    qkv = inp["qkv"].to(DEV)
    (kc, fk), (vc, fv) = sentinel_view((B, TMAX, H, hd)), sentinel_view((B, TMAX, H, hd))
    for b, p in enumerate(inp["pos"].tolist()):
        n = min(max(p, 0), TMAX)
        kc[b, :n] = inp["kc"][b, :n].to(DEV)
        vc[b, :n] = inp["vc"][b, :n].to(DEV)
    o, fo = sentinel_view((B, H + 0, hd))  # [B,H,hd] view of [B,H+3,hd+8]
    return dict(q=qkv[:, 0], k=qkv[:, 1], v=qkv[:, 2], kc=kc, vc=vc, fk=fk, fv=fv, o=o, fo=fo, pos=inp["pos"].to(DEV), cos=inp["cos"].to(DEV),
                sin=inp["sin"].to(DEV))


def run_kernel(d):
    from roboticattack_amd import _lib

    _lib.check(c_decode(d["q"], d["k"], d["v"], d["kc"], d["vc"], d["pos"], d["cos"], d["sin"], d["o"]), "vaa_model_attention_decode")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- model level ----------------------------------------------------------------
ACTION_BOOST = 8.0


def tiny_model(seed, dtype, device="cpu"):
    """tiny_cfg() with random weights drawn on the CPU (the same on every machine), the LM head's 256 action rows scaled by ACTION_BOOST: like
    the trained policy the model then answers with action tokens, and the top-2 margins are of the size of the logits instead of the gaps of
    32,064 nearly equal ones."""
    from roboticattack_amd.constants import ACTION_HI, ACTION_LO
    from roboticattack_amd.openvla_model import build_openvla, tiny_cfg

    m = build_openvla(tiny_cfg(), device="cpu", dtype=dtype, seed=seed)
    with torch.no_grad():
        m.lm_head.weight[ACTION_LO:ACTION_HI] *= ACTION_BOOST
    return m.to(device)


def prompt_batch(seed, lens=(5, 9, 12), dtype=torch.float32, device="cpu"):
    """(input_ids, attention_mask, pixel_values): right-padded random prompts of the given lengths and random frames."""
    from roboticattack_amd.constants import BOS_ID, PAD_ID

    g = torch.Generator().manual_seed(seed)
    B, L = len(lens), max(lens)
    ids = torch.randint(3, 31000, (B, L), generator=g)
    ids[:, 0] = BOS_ID
    mask = torch.arange(L)[None, :] < torch.tensor(lens)[:, None]
    ids = torch.where(mask, ids, torch.full_like(ids, PAD_ID))
    pix = torch.randn((B, 6, 224, 224), generator=g).to(dtype)
    return ids.to(device), mask.long().to(device), pix.to(device)


def top2_margin(logits):
    top = logits.float().topk(2, -1).values
    return top[..., 0] - top[..., 1]


def same_prefix(ta, tb):
    """[B,S] bool: the two decodings chose the same tokens at every EARLIER step of the row (their step-s logits answer the same question)."""
    eq = (ta == tb).long()
    return torch.cat([torch.ones_like(eq[:, :1]), eq.cumprod(1)[:, :-1]], 1).bool()


# ---------------------------------------------------------------- one layer's inference graph, written out ----------------------------------------------------------------
# LlamaLayer.prefill / decode_step restated in a straight line from the public pieces, without the layer's projection kinds: a projection is
# `linear(name, x2, res)` with name in "qkv" -> [M,3D], "o_proj" -> [M,D], "gate_up" -> (g, u), "down_proj" -> [M,D], supplied by
# layer_linear below. Both sides run the same operations on the same inputs, so the tests compare with torch.equal.
LAYER_KINDS = (("bf16", None), ("nf4", None), ("fp4", None), ("int8", 6.0), ("int8", 0.0))
LAYER_T, LAYER_TMAX = 12, 20
LAYER_POS = {3: (5, 9, 12), 1: (12,)}  # different per row; 12 is the first slot behind the prompt
LAYER_BIG_COLUMN = 5  # x carries 64 times the other columns' scale here: RMSNorm maps it to about sqrt(64) = 8 >= the int8 threshold 6


def layer_kind_id(k):
    return k[0] if k[1] is None else "%s_thr%g" % k


def layer_fused(layer, x):
    from roboticattack_amd import model_ops

    D = x.shape[-1]
    return model_ops.enabled(x) and (D // layer.heads) % 16 == 0 and D % 8 == 0 and D <= 8192


def layer_linear(layer, kind, fused, gemv):
    """The projections of `layer` (layer 0 of a tiny model, converted to `kind`) for one phase of the written-out graph."""
    import torch.nn.functional as F

    from roboticattack_amd import quant

    def bf16(name, x2, res):
        if name == "qkv":
            if fused:
                return F.linear(x2, torch.cat([layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight], 0))
            return torch.stack([layer.q_proj(x2), layer.k_proj(x2), layer.v_proj(x2)], dim=1).view(x2.shape[0], -1)
        if name == "gate_up":
            return layer.gate_proj(x2), layer.up_proj(x2)
        w = getattr(layer, name).weight
        if name == "o_proj" or fused:
            return torch.addmm(res, x2, w.t())
        return res + F.linear(x2, w)  # down_proj on the stock route: two roundings

    def quantised(name, x2, res):
        lin = getattr(layer, name + ("_q8" if kind == "int8" else "_q4") if name in ("qkv", "gate_up") else name)
        if name == "down_proj":
            x2 = x2.contiguous()
        if kind == "int8":
            y = quant.q8_linear(x2, lin, res, None, layer._quant_scratch)
        else:
            y = quant.q4_linear(x2, lin, res, layer._quant_scratch, gemv)
        return (y[:, :y.shape[1] // 2], y[:, y.shape[1] // 2:]) if name == "gate_up" else y

    return bf16 if kind == "bf16" else quantised


@torch.no_grad()
def ref_layer_prefill(layer, linear, x, rope_tab, cache):
    import torch.nn.functional as F

    from roboticattack_amd import model_ops
    from roboticattack_amd.openvla_model import _rope as rope_qk

    B, T, D = x.shape
    H = layer.heads
    fused = layer_fused(layer, x)
    n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
    h = (model_ops.ResidualRMSNormFn.apply(x, n1.weight, n1.eps)[1] if fused else n1(x)).reshape(-1, D)
    qkv = linear("qkv", h, None).view(B, T, 3, H, D // H)
    cos, sin = rope_tab[0][:T], rope_tab[1][:T]
    if fused:
        q, k = model_ops.RopeFn.apply(qkv[:, :, 0], cos, sin), model_ops.RopeFn.apply(qkv[:, :, 1], cos, sin)
    else:
        c, s = (torch.cat([t, t], -1).to(x.dtype)[None, :, None, :] for t in (cos, sin))
        q, k = rope_qk(qkv[:, :, 0], qkv[:, :, 1], c, s)
    v = qkv[:, :, 2]
    if fused and model_ops.attention_enabled(q):
        a = model_ops.attention_fwd(q, k, v, True)[0]
    else:
        a = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), is_causal=True).transpose(1, 2)
    cache[0][:, :T] = k
    cache[1][:, :T] = v
    x2 = linear("o_proj", a.reshape(-1, D), x.reshape(-1, D))
    h = (model_ops.ResidualRMSNormFn.apply(x2.view(B, T, D), n2.weight, n2.eps)[1] if fused else n2(x2.view(B, T, D))).reshape(-1, D)
    g, u = linear("gate_up", h, None)
    y = model_ops.SwiGLUFn.apply(g, u) if fused and (B * T * g.shape[1]) % 8 == 0 else F.silu(g) * u
    return linear("down_proj", y, x2).view(B, T, D)


@torch.no_grad()
def ref_layer_decode_step(layer, linear, x, pos, rope_tab, cache):
    import torch.nn.functional as F

    from roboticattack_amd import model_ops

    B, _, D = x.shape
    H = layer.heads
    fused = layer_fused(layer, x)
    n1, n2 = layer.input_layernorm, layer.post_attention_layernorm
    h = (model_ops.ResidualRMSNormFn.apply(x, n1.weight, n1.eps)[1] if fused else n1(x)).reshape(-1, D)
    qkv = linear("qkv", h, None).view(B, 3, H, D // H)
    a = model_ops.attention_decode(qkv[:, 0], qkv[:, 1], qkv[:, 2], cache[0], cache[1], pos, rope_tab[0], rope_tab[1])
    x2 = linear("o_proj", a.reshape(-1, D), x.reshape(-1, D))
    h = (model_ops.ResidualRMSNormFn.apply(x2.view(B, 1, D), n2.weight, n2.eps)[1] if fused else n2(x2.view(B, 1, D))).reshape(-1, D)
    g, u = linear("gate_up", h, None)
    y = model_ops.SwiGLUFn.apply(g, u) if fused and (B * g.shape[1]) % 8 == 0 else F.silu(g) * u
    return linear("down_proj", y, x2).view(B, 1, D)


_LAYERS = {}


def layer_of_kind(kind, threshold, device="cpu", seed=3):
    """Layer 0 of tiny_model(seed, bf16), converted to `kind`; built once per process and device and left unchanged."""
    from roboticattack_amd import quant

    key = (kind, threshold, str(device))
    if key not in _LAYERS:
        m = tiny_model(seed, BF, device)
        if kind == "int8":
            quant.quantize_llm(m, kind, threshold=threshold)
        elif kind != "bf16":
            quant.quantize_llm(m, kind)
        _LAYERS[key] = m.layers[0]
    return _LAYERS[key]


def layer_inputs(B, device="cpu", seed=3):
    """(x bf16 [B,12,64], x1 bf16 [B,1,64], pos int32 [B], rope_tab): rows of one seeded draw with LAYER_BIG_COLUMN scaled up."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.ones(64)
    scale[LAYER_BIG_COLUMN] = 64.0
    x = (torch.randn((3, LAYER_T, 64), generator=g) * scale).to(BF)[:B]
    x1 = (torch.randn((3, 1, 64), generator=g) * scale).to(BF)[:B]
    cos, sin = rope_tables(LAYER_TMAX, 16)
    return x.to(device), x1.to(device), torch.tensor(LAYER_POS[B], dtype=torch.int32, device=device), (cos.to(device), sin.to(device))


def layer_outlier_columns(layer, x, threshold=6.0):
    """How many columns of the q/k/v projection's input quant.q8_linear carries in bf16 at `threshold`."""
    from roboticattack_amd import quant

    return int(quant.q8_act_quant_torch(layer.input_layernorm(x).reshape(-1, x.shape[-1]), threshold)[2].sum())


def layer_graph_pairs(layer, kind, x, x1, pos, rope_tab):
    """[(what, the layer's result, the written-out statement's)] for one prefill and one decode step behind it: hidden states and caches."""
    B, _, D = x.shape
    H = layer.heads
    caches = [tuple(torch.zeros((B, LAYER_TMAX, H, D // H), dtype=x.dtype, device=x.device) for _ in range(2)) for _ in range(2)]
    fused = layer_fused(layer, x)
    y = layer.prefill(x, rope_tab, caches[0])
    yr = ref_layer_prefill(layer, layer_linear(layer, kind, fused, False), x, rope_tab, caches[1])
    z = layer.decode_step(x1, pos, rope_tab, caches[0])
    zr = ref_layer_decode_step(layer, layer_linear(layer, kind, fused, True), x1, pos, rope_tab, caches[1])
    return [("prefill", y, yr), ("decode step", z, zr), ("k cache", caches[0][0], caches[1][0]), ("v cache", caches[0][1], caches[1][1])]
