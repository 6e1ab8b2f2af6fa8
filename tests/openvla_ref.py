"""What the OpenVLA model-path tests share (a plain module, not a conftest): an fp64 CPU reference of `OpenVLAShaped` assembled from
INDEPENDENT code, the weights that make the comparison sensitive, the cases, and the measures.

The reference is made of Hugging Face `transformers` model classes built from config objects alone (random weights, no hub access, no
checkpoint), loaded with the weights of the model under test:

    Llama stack   LlamaForCausalLM, eager attention, driven with `inputs_embeds`, a right-padded `attention_mask` and HF's default position ids
    DINOv2 tower  Dinov2WithRegistersModel: cls_token, register_tokens [1,4,D], position_embeddings [1,257,D], layer_scale{1,2}.lambda1,
                  separate query / key / value (the project's fused qkv is split in three)
    SigLIP tower  SiglipVisionModel (no pooling head)

Each tower returns `hidden_states[depth-1]` — the output after depth-1 blocks (hidden_states[0] is the embedding output), before the final
norm — with the prefix tokens dropped: what timm's `get_intermediate_layers(n={depth-2})` returns. For a `cls_pos=False` tower the class
token's slot of HF's position_embeddings is zero (timm `no_embed_class`: position embedding on the patch tokens only); for `cls_pos=True`
it carries pos_embed[:, 0]. Both HF classes express their tower exactly, so no tower is restated by hand. The projector
(fc1 -> GELU -> fc2 -> GELU -> fc3, erf GELU) and the multimodal assembly [BOS, 256 projected tokens, text 1..] are restated here in a few
lines of plain torch double; none of the model's own modules is called. `lm_head` is applied to the rows that are read only.

Every reference parameter must have been assigned: `load_state_dict`'s missing keys may only be parts that are never evaluated (the final
norms, DINOv2's mask token, the last block of each tower).

Observables (measured against the fp64 reference): the labelled-row logits [R,V] of `forward_rows`, the full `forward()` logits on real
tokens, and the gradient of the LINEAR functional sum(rows * C), C a fixed random cotangent — so the measured quantity is the model's adjoint
and not a loss's curvature — with respect to `pixel_values`, or to the two patch-embed inputs of the `patch_embeds=` path.
Measures: relative rms error, relative max error (max|x - ref| / max|ref|) and, for gradients, the cosine.

`init_sensitive` draws weights at which such a comparison can see a wrong rotary table, mask or position: pre-softmax attention logits with
a standard deviation of 1-2 in the ViT blocks and the Llama layers (`attention_logit_std` measures it), random norm gains, biases,
LayerScale, pos_embed and prefix tokens. With `init_random(std=0.02)` at toy widths attention is near-uniform and the blocks near-linear.
"""
import os
import re
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from roboticattack_amd.constants import IGNORE_INDEX, N_IMG_TOKENS, PAD_ID  # noqa: E402
from roboticattack_amd.openvla_model import OpenVLACfg, OpenVLAShaped, VitCfg  # noqa: E402

F64 = torch.float64
BOS_ID = 1


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def _cfg(dino, siglip, dim, layers, heads, mlp):
    return OpenVLACfg(dino=dino, siglip=siglip, llm_dim=dim, llm_layers=layers, llm_heads=heads, llm_mlp=mlp, seq_floor=44, seq_multiple=4)


# name -> (cfg, prompt lengths, which of the last 8 tokens of a prompt are labelled). Images are 224 x 224 and the sequence is 256 + L, so the
# knobs are widths, depth, B and the prompt lengths. L = max length; the bucket of seq_floor=44 / seq_multiple=4 is given per case.
CASES = {
    # Llama head dim 128 (RopePackedAttentionFn / RopeAttentionFn); tower head dims 64 and 72 as in the 7B towers (1024/16, 1152/16).
    # L = 40 -> bucket 44: every prompt is below the floor
    "hd128": (_cfg(VitCfg(128, 3, 2, 256, 5, False, True), VitCfg(144, 3, 2, 288, 0, False, False), 256, 2, 2, 512), (30, 40, 37), (0, 2, 3, 5, 6, 7)),
    # Llama head dim 64, three layers (a middle layer with neither the embedding below nor the row selection above), a cls_pos=True DINO
    # tower (head dim 32), SigLIP head dim 48. L = 33 -> bucket 44
    "hd64_clspos": (_cfg(VitCfg(64, 3, 2, 128, 5, True, True), VitCfg(96, 3, 2, 192, 0, False, False), 192, 3, 3, 384), (21, 33), (0, 1, 4, 7)),
    # Llama head dim 80: hd % 16 == 0 but not 64 / 128 -> RopeFn + AttentionFn. L = 50 -> bucket 52 (the multiple, above the floor)
    "hd80": (_cfg(VitCfg(64, 3, 2, 128, 5, False, True), VitCfg(80, 3, 2, 160, 0, False, False), 160, 2, 2, 320), (46, 50), (1, 2, 6, 7)),
}
FULL_CASE = "hd128"   # the case whose full forward() logits and patch-embed gradients are measured on the GPU


def make_batch(name):
    """The batch of a case, on the CPU: input_ids / attention_mask / labels [B,L] right-padded like the collator's, pixel_values [B,6,224,224]
    (values exactly representable in bf16, so every precision sees the same input), the cotangent C [R,V] and the two patch-embed inputs
    [B,256,D] of the `patch_embeds=` path (random, bf16-representable: an input like any other)."""
    cfg, lens, keep = CASES[name]
    g = torch.Generator().manual_seed(1000 + sum(lens) + cfg.llm_dim)
    B, L = len(lens), max(lens)
    ids = torch.full((B, L), PAD_ID, dtype=torch.int64)
    labels = torch.full((B, L), IGNORE_INDEX, dtype=torch.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(3, 31000, (n,), generator=g)
        ids[b, 0] = BOS_ID
        for j in keep:
            labels[b, n - 8 + j] = ids[b, n - 8 + j]
    pix = torch.randn(B, 6, 224, 224, generator=g).to(torch.bfloat16).to(F64)
    R = int((labels[:, 1:] != IGNORE_INDEX).sum())
    cot = torch.randn(R, cfg.vocab, generator=g).to(torch.bfloat16).to(F64)
    emb = tuple(torch.randn(B, N_IMG_TOKENS, d, generator=g).to(torch.bfloat16).to(F64) for d in (cfg.dino.dim, cfg.siglip.dim))
    return dict(name=name, input_ids=ids, attention_mask=ids.ne(PAD_ID), labels=labels, pixel_values=pix, cot=cot, patch_embeds=emb, lens=lens)


def build_model(name, seed=0):
    """`OpenVLAShaped` of the case on the CPU in fp32 with init_sensitive's weights ROUNDED TO bf16 (then a .double(), a .bfloat16() and the
    reference all hold the same values)."""
    m = OpenVLAShaped(CASES[name][0])
    init_sensitive(m, seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16))
    return m.eval()


# ---------------------------------------------------------------- weights ----------------------------------------------------------------
QK_LOGIT_STD = 1.5  # target standard deviation of the pre-softmax attention logits


@torch.no_grad()
def init_sensitive(model, seed):
    """Weights at which a reference comparison is sensitive (module docstring). For unit-variance normed activations h (gain about 1) and
    q, k weights of standard deviation s, scale * q.k has standard deviation s^2 * D: s = sqrt(QK_LOGIT_STD / D). Every other matrix has
    unit gain (1 / sqrt(fan_in)), so the residual streams neither vanish nor blow up over 2-3 blocks."""
    g = torch.Generator().manual_seed(seed)

    def rnd(p, std, mean=0.0):
        p.copy_((torch.randn(p.shape, generator=g, dtype=F64) * std + mean).to(p.dtype))

    def linear(lin, std=None):
        rnd(lin.weight, std if std is not None else lin.in_features ** -0.5)
        if lin.bias is not None:
            rnd(lin.bias, 0.1)

    for vit in (model.featurizer, model.fused_featurizer):
        D = vit.c.dim
        rnd(vit.patch_embed.weight, 588 ** -0.5)
        rnd(vit.patch_embed.bias, 0.1)
        rnd(vit.pos_embed, 0.5)
        if vit.prefix is not None:
            rnd(vit.prefix, 0.5)
        for blk in vit.blocks:
            for n in (blk.norm1, blk.norm2):
                rnd(n.weight, 0.2, 1.0)
                rnd(n.bias, 0.1)
            linear(blk.qkv)
            rnd(blk.qkv.weight[: 2 * D], (QK_LOGIT_STD / D) ** 0.5)
            linear(blk.proj)
            linear(blk.fc1)
            linear(blk.fc2)
            if blk.ls1 is not None:
                rnd(blk.ls1, 0.25, 0.6)
                rnd(blk.ls2, 0.25, 0.6)
    for lin in (model.fc1, model.fc2, model.fc3):
        linear(lin)
    rnd(model.embed_tokens.weight, 1.0)
    D = model.cfg.llm_dim
    for lyr in model.layers:
        rnd(lyr.input_layernorm.weight, 0.2, 1.0)
        rnd(lyr.post_attention_layernorm.weight, 0.2, 1.0)
        linear(lyr.q_proj, (QK_LOGIT_STD / D) ** 0.5)
        linear(lyr.k_proj, (QK_LOGIT_STD / D) ** 0.5)
        for n in ("v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"):
            linear(getattr(lyr, n))
    rnd(model.norm.weight, 0.2, 1.0)
    linear(model.lm_head)
    return model


@torch.no_grad()
def attention_logit_std(model, batch):
    """Standard deviation of the pre-softmax attention logits of every block, measured on the fp64 model's own projections (forward hooks on
    `qkv` / `q_proj` / `k_proj`; the Llama logits with the rotation applied, over the causally visible real keys): {block name: std}."""
    m = OpenVLAShaped(model.cfg).double()
    m.load_state_dict({k: v.double().cpu() for k, v in model.state_dict().items()})
    got, hooks = {}, []
    for tn, vit in (("dino", m.featurizer), ("siglip", m.fused_featurizer)):
        for i, blk in enumerate(vit.blocks):
            hooks.append(blk.qkv.register_forward_hook(lambda mod, a, out, key="%s.%d" % (tn, i), H=blk.heads: got.__setitem__(key, (out, H))))
    for i, lyr in enumerate(m.layers):
        hooks.append(lyr.q_proj.register_forward_hook(lambda mod, a, out, key="llm.%d.q" % i: got.__setitem__(key, out)))
        hooks.append(lyr.k_proj.register_forward_hook(lambda mod, a, out, key="llm.%d.k" % i: got.__setitem__(key, out)))
    m.hidden_states(batch["input_ids"], batch["pixel_values"])
    for h in hooks:
        h.remove()
    out = {}
    for key, val in got.items():
        if key.startswith("llm"):
            continue
        qkv, H = val
        B, T, D3 = qkv.shape
        q, k, _ = qkv.view(B, T, 3, H, D3 // 3 // H).permute(2, 0, 3, 1, 4)
        out[key] = float((q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5).std())
    H = model.cfg.llm_heads
    real = multimodal_mask(batch["attention_mask"])
    for i in range(len(m.layers)):
        q, k = got["llm.%d.q" % i], got["llm.%d.k" % i]
        B, T, D = q.shape
        hd = D // H
        ang = torch.outer(torch.arange(T, dtype=F64), model.cfg.rope_theta ** (-torch.arange(0, hd, 2, dtype=F64) / hd))
        cos, sin = torch.cat([ang.cos()] * 2, -1), torch.cat([ang.sin()] * 2, -1)
        rot = lambda x: x * cos + torch.cat([-x[..., hd // 2:], x[..., : hd // 2]], -1) * sin
        q, k = rot(q.view(B, T, H, hd).transpose(1, 2)), rot(k.view(B, T, H, hd).transpose(1, 2))
        s = q @ k.transpose(-1, -2) * hd ** -0.5
        vis = torch.ones(T, T, dtype=torch.bool).tril()[None, None] & real[:, None, :, None] & real[:, None, None, :]
        out["llm.%d" % i] = float(s[vis.expand_as(s)].std())
    return out


# ---------------------------------------------------------------- the reference ----------------------------------------------------------------
def multimodal_mask(attention_mask):
    """[B,L] -> [B,256+L]: BOS, the 256 image tokens, text 1.."""
    B = attention_mask.shape[0]
    return torch.cat([attention_mask[:, :1].bool(), torch.ones(B, N_IMG_TOKENS, dtype=torch.bool), attention_mask[:, 1:].bool()], 1)


def label_rows(labels):
    """(b, t) of the labelled rows in row-major order: multimodal position t predicts the label at t + 1 (HF's causal shift); the multimodal
    labels are [labels[0], 256 x IGNORE, labels[1:]]."""
    B = labels.shape[0]
    mm = torch.cat([labels[:, :1], torch.full((B, N_IMG_TOKENS), IGNORE_INDEX, dtype=labels.dtype), labels[:, 1:]], 1)
    bt = (mm[:, 1:] != IGNORE_INDEX).nonzero(as_tuple=False)
    return bt[:, 0], bt[:, 1]


def _load(module, sd, unused):
    """Assign `sd`; nothing unexpected, and nothing missing except keys matching `unused` (parts that are never evaluated)."""
    res = module.load_state_dict({k: v.detach().double().cpu().clone() for k, v in sd.items()}, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    left = [k for k in res.missing_keys if not re.match(unused, k)]
    assert not left, "reference parameters never assigned: %s" % left
    assert len(sd) > 0 and len(res.missing_keys) < len(module.state_dict())
    return module


def _dino_tower(vit):
    """A tower with prefix tokens [cls, registers] -> Dinov2WithRegistersModel."""
    from transformers import Dinov2WithRegistersConfig, Dinov2WithRegistersModel

    c = vit.c
    assert c.n_prefix >= 1 and c.mlp % c.dim == 0
    conf = Dinov2WithRegistersConfig(hidden_size=c.dim, num_hidden_layers=c.depth, num_attention_heads=c.heads, mlp_ratio=c.mlp // c.dim,
                                     hidden_act="gelu", layer_norm_eps=1e-6, image_size=224, patch_size=14, num_register_tokens=c.n_prefix - 1,
                                     qkv_bias=True, use_swiglu_ffn=False, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                     drop_path_rate=0.0, attn_implementation="eager")
    m = Dinov2WithRegistersModel(conf).double().eval()
    p = dict(vit.named_parameters())
    D = c.dim
    pos = p["pos_embed"] if c.cls_pos else torch.cat([torch.zeros(1, 1, D, dtype=p["pos_embed"].dtype, device=p["pos_embed"].device), p["pos_embed"]], 1)
    sd = {"embeddings.cls_token": p["prefix"][:, :1], "embeddings.register_tokens": p["prefix"][:, 1:], "embeddings.position_embeddings": pos,
          "embeddings.patch_embeddings.projection.weight": p["patch_embed.weight"], "embeddings.patch_embeddings.projection.bias": p["patch_embed.bias"]}
    for i in range(c.depth - 1):
        a, b = "blocks.%d." % i, "encoder.layer.%d." % i
        for j, n in enumerate(("query", "key", "value")):
            sd[b + "attention.attention.%s.weight" % n] = p[a + "qkv.weight"][j * D:(j + 1) * D]
            sd[b + "attention.attention.%s.bias" % n] = p[a + "qkv.bias"][j * D:(j + 1) * D]
        for src, dst in (("norm1", "norm1"), ("norm2", "norm2"), ("proj", "attention.output.dense"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + dst + ".weight"], sd[b + dst + ".bias"] = p[a + src + ".weight"], p[a + src + ".bias"]
        for n in ("1", "2"):
            sd[b + "layer_scale%s.lambda1" % n] = p[a + "ls" + n] if c.layerscale else torch.ones(D)
    return _load(m, sd, r"layernorm\.|embeddings\.mask_token$|encoder\.layer\.%d\." % (c.depth - 1))


def _siglip_tower(vit):
    """A tower without prefix tokens and without LayerScale -> SiglipVisionModel (no pooling head)."""
    from transformers import SiglipVisionConfig, SiglipVisionModel

    c = vit.c
    assert c.n_prefix == 0 and not c.layerscale and not c.cls_pos
    conf = SiglipVisionConfig(hidden_size=c.dim, num_hidden_layers=c.depth, num_attention_heads=c.heads, intermediate_size=c.mlp, hidden_act="gelu",
                              layer_norm_eps=1e-6, image_size=224, patch_size=14, attention_dropout=0.0, vision_use_head=False,
                              attn_implementation="eager")
    m = SiglipVisionModel(conf).double().eval()
    p = dict(vit.named_parameters())
    D = c.dim
    sd = {"embeddings.patch_embedding.weight": p["patch_embed.weight"], "embeddings.patch_embedding.bias": p["patch_embed.bias"],
          "embeddings.position_embedding.weight": p["pos_embed"][0]}
    for i in range(c.depth - 1):
        a, b = "blocks.%d." % i, "encoder.layers.%d." % i
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            sd[b + "self_attn.%s.weight" % n] = p[a + "qkv.weight"][j * D:(j + 1) * D]
            sd[b + "self_attn.%s.bias" % n] = p[a + "qkv.bias"][j * D:(j + 1) * D]
        for src, dst in (("norm1", "layer_norm1"), ("norm2", "layer_norm2"), ("proj", "self_attn.out_proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            sd[b + dst + ".weight"], sd[b + dst + ".bias"] = p[a + src + ".weight"], p[a + src + ".bias"]
    return _load(m, sd, r"post_layernorm\.|encoder\.layers\.%d\." % (c.depth - 1))


def _llama(model):
    from transformers import LlamaConfig, LlamaForCausalLM

    c = model.cfg
    conf = LlamaConfig(vocab_size=c.vocab, hidden_size=c.llm_dim, intermediate_size=c.llm_mlp, num_hidden_layers=c.llm_layers,
                       num_attention_heads=c.llm_heads, num_key_value_heads=c.llm_heads, hidden_act="silu", rms_norm_eps=c.rms_eps,
                       rope_theta=c.rope_theta, attention_bias=False, mlp_bias=False, attention_dropout=0.0, tie_word_embeddings=False,
                       max_position_embeddings=2048, attn_implementation="eager")
    theta = conf.rope_parameters["rope_theta"] if getattr(conf, "rope_parameters", None) else conf.rope_theta
    assert float(theta) == float(c.rope_theta) and conf.rms_norm_eps == c.rms_eps and conf.head_dim == c.llm_dim // c.llm_heads
    m = LlamaForCausalLM(conf).double().eval()
    p = dict(model.named_parameters())
    sd = {"model.embed_tokens.weight": p["embed_tokens.weight"], "model.norm.weight": p["norm.weight"], "lm_head.weight": p["lm_head.weight"]}
    for i in range(c.llm_layers):
        a, b = "layers.%d." % i, "model.layers.%d." % i
        for n in ("q_proj", "k_proj", "v_proj", "o_proj"):
            sd[b + "self_attn.%s.weight" % n] = p[a + n + ".weight"]
        for n in ("gate_proj", "up_proj", "down_proj"):
            sd[b + "mlp.%s.weight" % n] = p[a + n + ".weight"]
        for n in ("input_layernorm", "post_attention_layernorm"):
            sd[b + n + ".weight"] = p[a + n + ".weight"]
    return _load(m, sd, r"$^")  # every Llama parameter is evaluated


class Reference:
    """fp64 CPU reference of an OpenVLAShaped (build_reference)."""

    def __init__(self, model):
        self.cfg = model.cfg
        self.towers = (_dino_tower(model.featurizer), _siglip_tower(model.fused_featurizer))
        self.llm = _llama(model)
        self.proj = [(getattr(model, n).weight.detach().double().cpu().clone(), getattr(model, n).bias.detach().double().cpu().clone())
                     for n in ("fc1", "fc2", "fc3")]
        for t in (*self.towers, self.llm):
            for q in t.parameters():
                q.requires_grad_(False)

    def _tower(self, i, pixels, embedded):
        """Patch tokens after depth-1 blocks. `embedded` [B,256,D] replaces the patch-embedding module's output (a forward hook: the HF model's
        own forward still does everything else)."""
        tower = self.towers[i]
        depth = (self.cfg.dino, self.cfg.siglip)[i].depth
        n_prefix = (self.cfg.dino, self.cfg.siglip)[i].n_prefix
        hook = None
        if embedded is not None:
            B, N, D = embedded.shape
            if i == 0:  # Dinov2WithRegistersPatchEmbeddings returns [B,256,D]
                hook = tower.embeddings.patch_embeddings.register_forward_hook(lambda mod, a, out: embedded)
            else:       # SigLIP's Conv2d returns [B,D,16,16]; its embedding module flattens it
                hook = tower.embeddings.patch_embedding.register_forward_hook(lambda mod, a, out: embedded.transpose(1, 2).reshape(B, D, 16, 16))
            pixels = torch.zeros(B, 3, 224, 224, dtype=F64)
        try:
            hs = tower(pixel_values=pixels, output_hidden_states=True).hidden_states
        finally:
            if hook is not None:
                hook.remove()
        assert len(hs) == depth + 1
        return hs[depth - 1][:, n_prefix:]

    def hidden(self, input_ids, attention_mask, pixel_values=None, patch_embeds=None):
        """Final-norm hidden states [B,256+L,D] (rows of padding positions are meaningless)."""
        if patch_embeds is not None:
            f = [self._tower(i, None, patch_embeds[i]) for i in (0, 1)]
        else:
            f = [self._tower(i, pixel_values[:, 3 * i:3 * i + 3], None) for i in (0, 1)]
        x = torch.cat(f, dim=2)
        (w1, b1), (w2, b2), (w3, b3) = self.proj
        x = F.gelu(x @ w1.t() + b1)       # erf GELU
        x = F.gelu(x @ w2.t() + b2)
        x = x @ w3.t() + b3
        emb = self.llm.model.embed_tokens(input_ids)
        x = torch.cat([emb[:, :1], x, emb[:, 1:]], dim=1)  # [BOS, 256 projected tokens, text 1..]
        return self.llm.model(inputs_embeds=x, attention_mask=multimodal_mask(attention_mask).long()).last_hidden_state

    def observables(self, batch, embeds=False, full=False):
        """dict(rows [R,V], grad: the gradient(s) of sum(rows * cot) w.r.t. pixel_values (or the tuple of patch-embed inputs), full [N,V]: the
        logits of all real tokens in (b,t) row-major order, or None)."""
        leaves = [t.clone().requires_grad_(True) for t in (batch["patch_embeds"] if embeds else (batch["pixel_values"],))]
        h = self.hidden(batch["input_ids"], batch["attention_mask"], None if embeds else leaves[0], tuple(leaves) if embeds else None)
        b, t = label_rows(batch["labels"])
        rows = self.llm.lm_head(h[b, t])
        grads = torch.autograd.grad((rows * batch["cot"]).sum(), leaves)
        out = dict(rows=rows.detach(), grad=grads if embeds else grads[0], full=None)
        if full:
            with torch.no_grad():
                out["full"] = self.llm.lm_head(h.detach()[multimodal_mask(batch["attention_mask"])])
        return out


def build_reference(model):
    return Reference(model)


# ---------------------------------------------------------------- the model under test ----------------------------------------------------------------
def model_observables(model, batch, embeds=False, full=False, pack=None, rows_from_full=False):
    """The same observables from `model` (any dtype / device), as tensors on the model's device. rows / grad come from `forward_rows`
    (rows_from_full: from the labelled rows of the full `forward()` instead); full from `forward()` on the real tokens."""
    dev, dt = model.device, model.embed_tokens.weight.dtype
    ids, labels = batch["input_ids"].to(dev), batch["labels"].to(dev)
    leaves = [t.to(dev, dt).requires_grad_(True) for t in (batch["patch_embeds"] if embeds else (batch["pixel_values"],))]
    cot = batch["cot"].to(dev, torch.float32 if dt == torch.bfloat16 else dt)
    if rows_from_full:
        b, t = label_rows(batch["labels"])
        rows = model(ids, pixel_values=leaves[0]).logits[b.to(dev), t.to(dev)]
    else:
        rows = model.forward_rows(ids, None if embeds else leaves[0], labels, patch_embeds=tuple(leaves) if embeds else None, pack=pack)
    grads = torch.autograd.grad((rows.to(cot.dtype) * cot).sum(), leaves)
    out = dict(rows=rows.detach(), grad=tuple(grads) if embeds else grads[0], full=None)
    if full:
        with torch.no_grad():
            out["full"] = model(ids, pixel_values=batch["pixel_values"].to(dev, dt)).logits[multimodal_mask(batch["attention_mask"]).to(dev)]
    return out


# ---------------------------------------------------------------- measures ----------------------------------------------------------------
def errors(x, ref):
    """dict(rms = rms(x - ref) / rms(ref), max = max|x - ref| / max|ref|, cos) of x against the fp64 reference (computed where x lives)."""
    ref = ref.to(x.device)
    d = x.double() - ref
    return dict(rms=float(d.square().mean().sqrt() / ref.square().mean().sqrt()), max=float(d.abs().max() / ref.abs().max()),
                cos=float(F.cosine_similarity(x.double().flatten(), ref.flatten(), dim=0)))


def measure(got, ref):
    """{observable: errors} of model_observables' result against Reference.observables'."""
    out = dict(rows=errors(got["rows"], ref["rows"]))
    if isinstance(ref["grad"], tuple):
        for i, (a, b) in enumerate(zip(got["grad"], ref["grad"])):
            out["embed_grad%d" % i] = errors(a, b)
    else:
        out["pixel_grad"] = errors(got["grad"], ref["grad"])
    if got.get("full") is not None and ref.get("full") is not None:
        out["full"] = errors(got["full"], ref["full"])
    return out
