"""LlamaLayer.prefill / decode_step on the GPU against the written-out statement of the same graph in decode_ref, bit for bit: the bf16, 4-bit
and int8 kinds of projection, with the fused model ops and on the stock route, and the 4-bit decode step through dequant + GEMM as well.
Both sides issue the same launches on the same inputs in one process."""
import pytest
import torch

import decode_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUTES = {"fused": {}, "stock": {"VAA_NO_FUSED_MODEL_OPS": "1", "VAA_NO_FUSED_ATTENTION": "1"}}


def _check(kind, route, monkeypatch):
    for k in ROUTES["stock"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    layer = decode_ref.layer_of_kind(*kind, device=DEV)
    for B in (3, 1):
        x, x1, pos, rope_tab = decode_ref.layer_inputs(B, DEV)
        assert decode_ref.layer_fused(layer, x) == (route == "fused")
        if kind[0] == "int8":
            for rows in (x, x1):
                assert 0 < decode_ref.layer_outlier_columns(layer, rows) < rows.shape[-1]
        pairs = decode_ref.layer_graph_pairs(layer, kind[0], x, x1, pos, rope_tab)
        torch.cuda.synchronize()
        for what, got, ref in pairs:
            assert got.shape == ref.shape and torch.equal(got, ref), "%s, B = %d" % (what, B)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", decode_ref.LAYER_KINDS, ids=decode_ref.layer_kind_id)
def test_layer_graph_equals_the_written_out_statement(kind, route, monkeypatch):
    """The cases of test_infer_graph_host.py (B = 3 at pos (5, 9, 12) and B = 1 at 12) with the fused model ops and without them."""
    _check(kind, route, monkeypatch)


@pytest.mark.parametrize("name", ["nf4", "fp4"])
def test_layer_graph_with_the_decode_step_through_dequant_and_gemm(name, monkeypatch):
    """quant.GEMV_MAX_ROWS = 0: the decode step's projections take vaa_model_q4_dequant + the stock GEMM on both sides."""
    from roboticattack_amd import quant

    monkeypatch.setattr(quant, "GEMV_MAX_ROWS", 0)
    _check((name, None), "fused", monkeypatch)
