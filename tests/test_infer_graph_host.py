"""LlamaLayer.prefill / decode_step against the written-out statement of the same graph in decode_ref, bit for bit, for the bf16, 4-bit and
int8 kinds of projection on the CPU; and what quantize_llm leaves on a layer: row views that alias the fused parent, the bytes it holds."""
import pytest
import torch

import decode_ref
from roboticattack_amd import quant


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("kind", decode_ref.LAYER_KINDS, ids=decode_ref.layer_kind_id)
def test_layer_graph_equals_the_written_out_statement(kind, B):
    """x bf16 [B,12,64], Tmax = 20, one prefill and one decode step at pos (5, 9, 12) (B = 1: 12): hidden states and both caches are equal.
    The int8 inputs carry one scaled-up column, so at threshold 6 some and not all columns of the q/k/v input take the bf16 outlier path."""
    layer = decode_ref.layer_of_kind(*kind)
    x, x1, pos, rope_tab = decode_ref.layer_inputs(B)
    if kind[0] == "int8":
        for rows in (x, x1):
            assert 0 < decode_ref.layer_outlier_columns(layer, rows) < rows.shape[-1]
    assert type(layer.projections).__name__ == ("Bf16Projections" if kind[0] == "bf16" else "QuantProjections")
    for what, got, ref in decode_ref.layer_graph_pairs(layer, kind[0], x, x1, pos, rope_tab):
        assert got.shape == ref.shape and torch.equal(got, ref), what


@pytest.mark.parametrize("kind", ["nf4", "int8"])
def test_row_views_alias_the_fused_parent(kind):
    layer = decode_ref.layer_of_kind(kind, 6.0 if kind == "int8" else None)
    qkv, gate_up = (layer.qkv_q8, layer.gate_up_q8) if kind == "int8" else (layer.qkv_q4, layer.gate_up_q4)
    d, mlp = layer.o_proj.out_features, layer.down_proj.in_features
    for parent, names, rows in ((qkv, ("q_proj", "k_proj", "v_proj"), d), (gate_up, ("gate_proj", "up_proj"), mlp)):
        for i, n in enumerate(names):
            view = getattr(layer, n)
            assert isinstance(view, quant.Q8LinearRows if kind == "int8" else quant.Q4LinearRows) and view.out_features == rows
            for buf in ("codes", "wscale" if kind == "int8" else "absmax"):
                assert getattr(view, buf).data_ptr() == getattr(parent, buf)[i * rows:].data_ptr()
            assert not list(view.buffers()) and view.quant_type == parent.quant_type  # held once, on the parent
    assert layer.q_proj.codes.data_ptr() == qkv.codes.data_ptr()
    assert (layer.q_proj.threshold == qkv.threshold) if kind == "int8" else (layer.q_proj.table == qkv.table)


@pytest.mark.parametrize("kind,nbytes", [("nf4", 46592), ("fp4", 46592), ("int8", 87040)])
def test_llm_weight_bytes_of_a_converted_tiny_model(kind, nbytes):
    """The literals are quant.llm_weight_bytes of the same converted model computed on the CPU at the commit before the projection kinds
    (164352 before conversion)."""
    m = decode_ref.tiny_model(3, torch.bfloat16)
    assert quant.llm_weight_bytes(m) == 164352
    assert quant.llm_weight_bytes(quant.quantize_llm(m, kind)) == nbytes
