"""openvla_model._route: every reachable combination of the facts a LlamaLayer.forward call decides from, against the route it takes — the
table was written by reading the forward this function replaced — and hidden_states' decision to pack against the layers' decision to take
a pack. No GPU: the route is computed from facts, not from a tensor."""
import dataclasses
import types

import pytest
import torch

from roboticattack_amd import model_ops, openvla_model
from roboticattack_amd.openvla_model import Route, _route

PACK = types.SimpleNamespace(cu="cu", max_len=17)
BASE = dict(ops_on=True, attn_on=True, tn_on=True, qkv_mode="auto", hd=128, D=4096, rows=2400, has_tab=True, pack=None)
STOCK = Route(False, False, False, "stock_sdpa", None, 0)
OFF = dict(ops_on=False, attn_on=False)  # attention_kernel_enabled(False, hd) is False
TABLE = [  # (facts that differ from BASE, route)
    (OFF, STOCK),
    (dict(OFF, pack=PACK), STOCK),
    (dict(OFF, tn_on=False, qkv_mode="1"), STOCK),
    (dict(has_tab=False), STOCK),  # no rotary table: the [1,1,T,hd] cos/sin form of _rope
    (dict(has_tab=False, pack=PACK), STOCK),
    (dict(hd=72, D=1152), STOCK),  # hd % 16
    (dict(D=16384), STOCK),
    ({}, Route(True, True, True, "rope_packed", None, 0)),
    (dict(rows=8191), Route(True, True, True, "rope_packed", None, 0)),
    (dict(rows=8192), Route(True, True, False, "rope", None, 0)),
    (dict(rows=19200), Route(True, True, False, "rope", None, 0)),
    (dict(rows=19200, qkv_mode="1"), Route(True, True, True, "rope_packed", None, 0)),
    (dict(qkv_mode="0"), Route(True, True, False, "rope", None, 0)),
    (dict(tn_on=False), Route(True, False, False, "rope", None, 0)),
    (dict(tn_on=False, qkv_mode="1"), Route(True, False, False, "rope", None, 0)),  # the one GEMM is a FrozenLinearsFn call: TN only
    (dict(hd=64, D=1024), Route(True, True, True, "rope_packed", None, 0)),
    (dict(hd=80, D=2560), Route(True, True, False, "rope_fn_attention", None, 0)),
    (dict(hd=80, D=2560, qkv_mode="1"), Route(True, True, False, "rope_fn_attention", None, 0)),  # never the cat / packed route
    (dict(hd=80, D=2560, tn_on=False), Route(True, False, False, "rope_fn_attention", None, 0)),
    (dict(hd=80, D=2560, pack=PACK), Route(True, True, False, "rope_fn_attention", None, 0)),  # and no pack
    (dict(attn_on=False), Route(True, True, True, "rope_fn_sdpa", None, 0)),  # still ONE GEMM, split by views
    (dict(attn_on=False, qkv_mode="0"), Route(True, True, False, "rope_fn_sdpa", None, 0)),
    (dict(attn_on=False, rows=19200), Route(True, True, False, "rope_fn_sdpa", None, 0)),
    (dict(attn_on=False, tn_on=False), Route(True, False, False, "rope_fn_sdpa", None, 0)),
    (dict(attn_on=False, hd=80, D=2560), Route(True, True, False, "rope_fn_sdpa", None, 0)),
    (dict(attn_on=False, pack=PACK), Route(True, True, True, "rope_fn_sdpa", None, 0)),
    (dict(pack=PACK), Route(True, True, True, "rope_packed", "cu", 17)),
    (dict(pack=PACK, qkv_mode="0"), Route(True, True, False, "rope", "cu", 17)),
    (dict(pack=PACK, tn_on=False), Route(True, False, False, "rope", "cu", 17)),
    (dict(pack=PACK, hd=64, D=1024, rows=18688), Route(True, True, False, "rope", "cu", 17)),
]


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_route_table(i):
    facts, want = TABLE[i]
    assert _route(**dict(BASE, **facts)) == want


def test_rope_in_attention_head_widths():
    assert [hd for hd in range(8, 257, 8) if model_ops.rope_in_attention(hd)] == [64, 128]


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_hidden_states_packs_iff_the_layers_take_the_pack(hd, monkeypatch):
    """hidden_states gathers the packed token axis exactly when the route its layers run on takes cu_seqlens: the layers then get the pack
    and that route; otherwise no layer sees the pack and the padded axis goes through."""
    cfg = dataclasses.replace(openvla_model.tiny_cfg(), llm_dim=2 * hd, llm_heads=2, llm_layers=2, llm_mlp=64)
    model = openvla_model.OpenVLAShaped(cfg).eval()
    seen = []

    def facts(x, heads, rope_tab, _orig=openvla_model._facts):  # the layer input's own facts, as if it were bf16 on the GPU
        return dict(_orig(x, heads, rope_tab), ops_on=True, attn_on=True)

    def layer_forward(self, x, cos, sin, rope_tab=None, rows=None, pack=None, route=None):
        seen.append((x.shape, rope_tab[0].shape[0], pack, route))
        return x

    monkeypatch.setattr(openvla_model, "_facts", facts)
    monkeypatch.setattr(openvla_model.LlamaLayer, "forward", layer_forward)
    mask = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1]])
    pack = openvla_model.SeqPack(mask)
    tokens = pack.total + (-pack.total) % 256
    assert pack.total == 2 * pack.T_pad - 1  # packing drops the one pad position (and adds the fill sequence)
    with torch.no_grad():
        model.hidden_states(torch.ones(2, 4, dtype=torch.int64), torch.zeros(2, 6, 224, 224), pack=pack)
    takes = _route(**dict(BASE, hd=hd, D=2 * hd, pack=pack)).cu is not None
    assert takes == model_ops.rope_in_attention(hd) and len(seen) == cfg.llm_layers
    for shape, tab_rows, got_pack, route in seen:
        if takes:
            assert got_pack is pack and route.cu is pack.cu and route.max_len == pack.max_len
            assert shape == (1, tokens, 2 * hd) and tab_rows == tokens and route.attention in ("rope_packed", "rope")
        else:
            assert got_pack is None and route.cu is None and route.max_len == 0
            assert shape == (2, pack.T_pad, 2 * hd) and tab_rows == pack.T_pad and route.attention == "rope_fn_attention"
