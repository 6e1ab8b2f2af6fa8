"""vaa_model_attention_{fwd,bwd}: every kernel form (4 head-width families x causal x G in {1,2} x {fwd, dq, dk/dv}) against the fp64
reference of attention_ref.py, with the eager bf16 formulation as the error yardstick; layouts, batch independence and write ownership bit
for bit. Bounds and their derivation: attention_ref's docstring."""
import functools

import pytest

import attention_ref as A

pytestmark = pytest.mark.gpu


def _assert_cases(results, n_expected):
    assert len(results) == n_expected
    for (fam, n), w in sorted(A.worst_ratios(results).items()):
        print("family <%s> %-2s worst rms(kernel)/rms(eager bf16) = %.3f" % (fam, n, w))
    bad = [m for r in results for m in A.failures(r)]
    assert not bad, "\n".join(bad[:40])


@functools.lru_cache(maxsize=None)
def _child(attn_g):
    """One fresh process per forced grouping, shared by the tests that need it."""
    return A.run_child(("dense", "packed", "writes") if attn_g == "222" else ("dense",), attn_g)


@pytest.mark.parametrize("fam", ["2,4", "3,5", "3,6", "4,8"])
def test_dense_every_instantiation_default_grouping(fam):
    """hd (padded and exact width of the family) x causal x T on the wave / tile / G=2-block edges x B*H around the 8-pair XCD grouping,
    forward (o, lse) and backward (dq, dk, dv) against fp64, with the default G."""
    cases = [c for c in A.group("dense") if A.family(c["hd"]) == fam]
    _assert_cases(A.run_cases(cases), len(cases))


@pytest.mark.parametrize("attn_g", ["111", "222"])
def test_dense_every_instantiation_forced_grouping(attn_g):
    """The same cases with VAA_ATTN_G forcing one / two row groups per wave for every head width (a fresh process: read once)."""
    _assert_cases(_child(attn_g)["dense"], len(A.group("dense")))


def test_layouts_bitwise():
    for r in A.run_group("layouts"):
        assert r["packed_qkv_equal"] and r["bhtd_view_equal"], r


def test_batch_independence_bitwise():
    for r in A.run_group("independence"):
        assert r["slice_equal"], r


def test_packed_sequences_vs_fp64():
    """cu_seqlens form against a per-sample fp64 loop: causal and not, forward and backward, plain and with the fused RoPE adjoint."""
    _assert_cases(A.run_group("packed"), len(A.group("packed")))


def test_packed_sequences_vs_fp64_two_groups():
    _assert_cases(_child("222")["packed"], len(A.group("packed")))


def test_fused_rope_adjoint_vs_fp64():
    _assert_cases(A.run_group("rope"), len(A.group("rope")))


def test_softmax_range_large_logits():
    """scale q.k spanning about +-60: running-max rescale and exp2 underflow; outputs finite (failures() checks it) and within the bounds."""
    _assert_cases(A.run_group("range"), len(A.group("range")))


def test_causal_row_zero_sees_one_key():
    for r in A.run_group("single_key"):
        assert r["o0_is_v0"] and r["lse0_err"] <= 1e-4, r


def test_writes_stay_inside():
    for r in A.run_group("writes"):
        assert r["sentinels_intact"] and r["view_equals_plain"], r


def test_writes_stay_inside_two_groups():
    res = _child("222")["writes"]
    assert len(res) == 12
    for r in res:
        assert r["sentinels_intact"] and r["view_equals_plain"], r
