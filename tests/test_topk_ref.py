"""CPU checks of tests/topk_ref.py: the reference selection, the ``ties`` family, the clear-row share
the GPU test's exact-id assertion rests on, and that each checker rejects what it is there to reject.
"""
import pytest
import torch

import tail_ref as R
import topk_ref as T

# the six decoder shapes of tests/test_gpu_gemm_epi.py, and two with slabs of fewer than k columns
SHAPES = [(1000, 256), (1153, 3 * 256), (21128, 3 * 768), (1025, 256), (1100, 256), (30522, 768), (130, 256), (100, 256)]
CLEAR_SHARE_MIN = 0.85
_refs = {}


def _ref(family, V, K, M=512):
    key = (family, V, K, M)
    if key not in _refs:
        if len(_refs) >= 4:
            _refs.pop(next(iter(_refs)))
        W = R.decoder_weight(V, K, seed=V + K)
        A, b, _ = T.operands(family, M, V, K, W, seed=V + K + len(family))
        _refs[key] = T.Ref(A, W, b, V)
    return _refs[key]


def test_topk_ref_order_is_logit_then_column():
    z = torch.tensor([[0.0, 2.0, 2.0, -1.0, 2.0, 5.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=torch.float64)
    assert T.topk_ref(z, 4).tolist() == [[5, 1, 2, 4], [0, 1, 2, 3]]
    assert T.topk_ref(z, 6)[0].tolist() == [5, 1, 2, 4, 0, 3]


@pytest.mark.parametrize("V", [100, 130, 1000, 1100])
def test_ties_family_expected_ids(V):
    """The logits are exactly the bias, so the float64 order is the tie rule's: the columns c % 97 == 3
    in ascending order (they cross slab and tile borders), then the lowest remaining columns."""
    ref = _ref("ties", V, 256, M=8)
    assert ref.e32.max().item() == 0.0
    ones = [c for c in range(V) if c % 97 == 3]
    for k in (1, 5, 16):
        want = T.ties_expected(V, k)
        assert want[:min(k, len(ones))] == ones[:k] and len(set(want)) == k
        if k > len(ones):
            assert want[len(ones):] == [c for c in range(V) if c % 97 != 3][:k - len(ones)]
        assert T.topk_ref(ref.z, k).tolist() == [want] * 8
    assert not ref.clear_rows(16).any()             # all ties: float64 decides nothing here


@pytest.mark.parametrize("V,K", SHAPES, ids=lambda x: str(x))
@pytest.mark.parametrize("family", R.DECODER_FAMILIES)
def test_clear_share(family, V, K):
    """At k = 16 at least 0.85 of the 512 reference rows are clear (the reference alone decides)."""
    share = float(_ref(family, V, K).clear_rows(16).double().mean())
    print(f"CLEAR {family} V{V} K{K}: {share:.3f}")
    assert share >= CLEAR_SHARE_MIN, (family, V, K, share)


def _good(ref, k, m=64):
    ids = T.topk_ref(ref.z[:m], k).to(torch.int32)
    lp = ref.lp[:m].gather(1, ids.long()).float()
    return ids, lp


@pytest.mark.parametrize("family", R.DECODER_FAMILIES)
def test_checkers_accept_the_reference(family):
    ref = _ref(family, 1100, 256)
    for k in (1, 5, 16):
        ids, lp = _good(ref, k)
        T.check_values(ids, lp, ref)
        T.check_complete(ids, ref)
        assert T.check_exact(ids, ref) == float(ref.clear_rows(k)[:64].double().mean())


def test_checkers_reject():
    ref = _ref("plain", 1100, 256)
    k = 5
    ids, lp = _good(ref, k)
    row = int(torch.nonzero(ref.clear_rows(k)[:64])[0])
    # a swapped pair on a clear row: the values no longer match their ids' order, and the ids differ
    sw = ids.clone()
    sw[row, 1], sw[row, 2] = ids[row, 2], ids[row, 1]
    with pytest.raises(AssertionError, match="float64 order"):
        T.check_exact(sw, ref)
    lp_sw = ref.lp[:64].gather(1, sw.long()).float()
    with pytest.raises(AssertionError, match="increase"):
        T.check_values(sw, lp_sw, ref)
    # a pad column (id >= V), and a negative id
    for bad_id in (1100, 1151, -1):
        pad = ids.clone()
        pad[row, k - 1] = bad_id
        with pytest.raises(AssertionError, match="outside"):
            T.check_values(pad, lp, ref)
    # a duplicate id
    dup = ids.clone()
    dup[row, 3] = ids[row, 2]
    with pytest.raises(AssertionError, match="duplicate"):
        T.check_values(dup, lp, ref)
    # a missing column: the list shifted by one (the best column left out)
    shifted = T.topk_ref(ref.z[:64], k + 1)[:, 1:].to(torch.int32)
    with pytest.raises(AssertionError, match="missing"):
        T.check_complete(shifted, ref)
    # a log-prob off by more than the bound
    off = lp.clone()
    off[row, 0] += 1e-3
    with pytest.raises(AssertionError, match="log-prob off"):
        T.check_values(ids, off, ref)
