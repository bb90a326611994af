"""Masked-LM scores for candidate sets (rs_masked_logprob_cands; include/rescore.h).

1. The kernels through rs_debug_decoder_cands — launch_mlm_decoder_cands, the function head_mlm runs for
   a candidate call: the -inf preset, EPI_LSE_CAND on the 256 x 256 / 256 x 128 tile, cand_finalize —
   against the float64 reference of tests/topk_ref.py and, bit for bit, against the label form
   (rs_debug_decoder).
2. The product (PLLScorer.score_cands / masked_logprob_cands) against rs_masked_logprob_multi bitwise and
   against the fp32 oracle (oracle.bert_ref.TorchBert), tiny BERT in both precisions and BERT-base.
3. Errors.
"""
import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
from asr_rescoring_amd.weights import BERT_BASE, BERT_TINY, make_weights
import slotlm_ref as S
import tail_ref as R
import topk_ref as T

pytestmark = pytest.mark.gpu

REL = 1e-3                                                                   # the project's tolerance on log-probs
SENT32 = 0x7FC12345                                                          # NaN sentinel (bit pattern)
SLACK = 64                                                                   # sentinel elements behind n_c
# (family, V, K, M_pad, m_valid).  (130, 256) vpad 256, slabs of 64 / 64 / 2 / 0 valid columns and
# (1000, 256) vpad 1024: the 256 x 256 tile; (1100, 256) vpad 1152: the 256 x 128 tile.  peaked / slab_spread:
# the |bias| 80 / 200 families, whose candidates' probabilities are tiny (log-probs near -80 / -200 .. -400).
ROWS = [(256, 1), (256, 37), (512, 300)]
CASES = [("plain", V, K) + r for V, K in [(130, 256), (1000, 256), (1100, 256)] for r in ROWS] + \
        [("peaked", 1000, 256, 256, 37), ("slab_spread", 1100, 256, 512, 300)]
LENS = (200, 0, 1, 2, 64, 5, 2, 200)                                         # list length of row i: LENS[i % 8]
_dec = {}


def _case_id(c):
    return f"{c[0]}-V{c[1]}-K{c[2]}-M{c[3]}-v{c[4]}"


def _decoder_case(family, V, K, rows=512):
    """Operands for ``rows`` rows and their float64 reference, once per (family, V, K).  Never modified."""
    key = (family, V, K)
    if key not in _dec:
        _dec.clear()
        W = R.decoder_weight(V, K, seed=V + K, device="cuda")
        A, b, _ = T.operands(family, rows, V, K, W, seed=V + K + len(family), device="cuda")
        _dec[key] = (W, A, b, T.Ref(A, W, b, V))
    return _dec[key]


def _lists(m_valid, V, seed, lens=LENS):
    """(c_off, cand) in the caller's order.  Row i's list has lens[i % len(lens)] entries: random ids with
    columns 0, 63, 64 and V - 1 planted in the long lists, a list of 5 that lies inside the slab
    [64, 128) (V permitting), and a duplicated id in every list of at least two entries (the entry at
    index 1 repeats the one at index 0; the long lists repeat more by chance or, for V = 130, by count)."""
    rng = np.random.default_rng(seed)
    c_off, cand = [0], []
    for i in range(m_valid):
        n = lens[i % len(lens)]
        if n == 5:
            ids = rng.integers(64, min(128, V), size=n)
        else:
            ids = rng.integers(0, V, size=n)
        if n >= 64:
            ids[[3, 17, 40, n - 1]] = [0, 63, 64, V - 1]
            ids[n // 2] = V - 1
        if n >= 2:
            ids[1] = ids[0]
        cand += ids.tolist()
        c_off.append(len(cand))
    return np.asarray(c_off, np.int32), np.asarray(cand, np.int32)


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _launch_cands(A, W, b, M_pad, m_valid, V, c_off, cand):
    """One rs_debug_decoder_cands launch on sentinel-filled buffers; the lists sorted as the C entry does."""
    vpad, K = W.shape
    A = A[:M_pad].contiguous()
    n_c = int(c_off[-1])
    ids, perm = S.sort_candidates(c_off.tolist(), cand.tolist())
    d_off, d_id, d_perm = _dev(c_off), _dev(ids + [0]), _dev(perm + [0])
    part = _sentinel((M_pad, vpad // 64, 2))
    clog = _sentinel((n_c + SLACK,))
    out = _sentinel((n_c + SLACK,))
    rc = _lib.load().rs_debug_decoder_cands(A.data_ptr(), W.data_ptr(), b.data_ptr(), M_pad, m_valid, vpad, V, K,
                                            part.data_ptr(), d_off.data_ptr(), d_id.data_ptr(), d_perm.data_ptr(),
                                            clog.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {"out": out, "part": part, "clog": clog}


def _launch_decoder(A, W, b, lab, M_pad, m_valid, V):
    """rs_debug_decoder (the label form) -> out [m_valid], part."""
    vpad, K = W.shape
    A = A[:M_pad].contiguous()
    part = _sentinel((M_pad, vpad // 64, 2))
    llog = _sentinel((M_pad,))
    out = _sentinel((m_valid,))
    labw = torch.empty((m_valid,), dtype=torch.int32, device="cuda")
    lab = lab[:m_valid].contiguous()
    rc = _lib.load().rs_debug_decoder(A.data_ptr(), W.data_ptr(), b.data_ptr(), lab.data_ptr(), M_pad, m_valid, vpad, V,
                                      K, labw.data_ptr(), part.data_ptr(), llog.data_ptr(), out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, part


def _check_cands(A, W, b, ref, M_pad, m_valid, V, c_off, cand, what):
    n_c = int(c_off[-1])
    got = _launch_cands(A, W, b, M_pad, m_valid, V, c_off, cand)
    out = got["out"][:n_c]
    assert (_bits(got["out"][n_c:]) == SENT32).all(), "out written past n_c"
    assert (_bits(got["clog"][n_c:]) == SENT32).all(), "cand_logit written past n_c"
    assert (_bits(got["part"][m_valid:]) == SENT32).all(), "part: rows >= m_valid written"
    assert torch.isfinite(out).all(), "an entry was not written (or is not finite)"
    # every value within the bound topk_ref.check_values applies to a log-prob (Ref.lp_bound's expression)
    row = torch.from_numpy(np.repeat(np.arange(m_valid), np.diff(c_off))).cuda()
    col = _dev(cand).long()
    err = (out.double() - ref.lp[row, col]).abs()
    bound = 4 * torch.maximum(ref.e32_lp[row], T.EPS32 * torch.maximum(ref.z[row, col].abs(), ref.lse[row].abs()))
    worst = float((err / bound).max()) if n_c else 0.0
    print(f"CANDS {what} tile 256x{R.decoder_tile(W.shape[0])}: n_c {n_c} lp err/bound {worst:.3f} "
          f"min lp {float(out.min()) if n_c else 0:.1f}")
    assert not (err > bound).any(), f"log-prob off by {float(err.max()):.3e} (err/bound {worst:.2f})"
    # the first, the last and a duplicated entry of every row: the label form's log-prob of that id, bitwise
    n = np.diff(c_off)
    has = torch.from_numpy(n > 0).cuda()
    for name, idx in (("first", c_off[:-1]), ("last", c_off[1:] - 1), ("duplicated", c_off[:-1] + 1)):
        ok = torch.from_numpy(n >= 2).cuda() if name == "duplicated" else has
        at = torch.from_numpy(np.clip(idx, 0, max(n_c - 1, 0)).astype(np.int64)).cuda()
        lab = torch.where(ok, col[at] if n_c else torch.zeros_like(at), torch.zeros_like(at)).to(torch.int32)
        out0, part0 = _launch_decoder(A, W, b, lab, M_pad, m_valid, V)
        assert torch.equal(_bits(out[at[ok]]), _bits(out0[ok])), f"{name} entry != rs_debug_decoder(label = its id)"
        if name == "duplicated":            # the two copies (index 0 and 1 of the caller's list) both got it
            assert torch.equal(_bits(out[at[ok] - 1]), _bits(out0[ok])), "a duplicated id's copies differ"
    assert torch.equal(_bits(got["part"][:m_valid]), _bits(part0[:m_valid])), "slab pairs differ from the label form's"
    again = _launch_cands(A, W, b, M_pad, m_valid, V, c_off, cand)
    for name in ("out", "part", "clog"):
        assert torch.equal(_bits(got[name]), _bits(again[name])), f"run-to-run: {name}"
    return got


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_decoder_cands_vs_float64_and_label_form(case):
    family, V, K, M_pad, m_valid = case
    W, A, b, ref = _decoder_case(family, V, K)
    c_off, cand = _lists(m_valid, V, seed=V + m_valid)
    assert {0, 63, 64, V - 1} <= set(cand.tolist())
    _check_cands(A, W, b, ref, M_pad, m_valid, V, c_off, cand, _case_id(case))


def test_decoder_cands_all_lists_empty():
    W, A, b, ref = _decoder_case("plain", 130, 256)
    got = _launch_cands(A, W, b, 256, 37, 130, np.zeros(38, np.int32), np.zeros(0, np.int32))
    assert (_bits(got["out"]) == SENT32).all() and (_bits(got["clog"]) == SENT32).all()
    _, part0 = _launch_decoder(A, W, b, torch.zeros(37, dtype=torch.int32, device="cuda"), 256, 37, 130)
    assert torch.equal(_bits(got["part"][:37]), _bits(part0[:37]))


def test_decoder_cands_rejects_malformed_lists():
    W, A, b, _ = _decoder_case("plain", 130, 256)
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    part, buf = _sentinel((256, 4, 2)), _sentinel((8,))
    ids, perm = _dev([1, 2, 3, 4]), _dev([0, 1, 2, 3])

    def call(off, pm):
        return lib.rs_debug_decoder_cands(A.data_ptr(), W.data_ptr(), b.data_ptr(), 256, 2, 256, 130, 256, part.data_ptr(),
                                          _dev(off).data_ptr(), ids.data_ptr(), pm.data_ptr(), buf.data_ptr(),
                                          buf.data_ptr(), st)
    assert call([0, 3, 2], perm) == -1                     # descending offsets
    assert call([1, 2, 4], perm) == -1                     # not from 0
    assert call([0, 2, 4], _dev([0, 1, 2, 4])) == -1       # perm outside [0, n_c)
    torch.cuda.synchronize()
    assert (_bits(buf) == SENT32).all() and (_bits(part) == SENT32).all()


def test_decoder_cands_product_shape():
    """The product's decoder (bert-base-chinese vocabulary, fp16x3 operand image), 50 candidates per row."""
    V, K, M_pad, m_valid = 21128, 3 * 768, 256, 37
    W, A, b, ref = _decoder_case("plain", V, K, rows=256)
    c_off, cand = _lists(m_valid, V, seed=9, lens=(50,))
    _check_cands(A, W, b, ref, M_pad, m_valid, V, c_off, cand, f"product V{V}-K{K}-v{m_valid}")


# ---- the product -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


def _rows(shape, lens, n_queries, seed, max_list=12):
    """Padded rows [B, T] with [MASK] at 1 .. 3 query positions each, and per query a candidate list of
    1 .. max_list ids (any order, a duplicate in lists of three or more): (ids, mask, types, qpos per row,
    lists per query)."""
    rng = np.random.default_rng(seed)
    B, Tm = len(lens), max(lens)
    ids, am = torch.zeros(B, Tm, dtype=torch.int64), torch.zeros(B, Tm, dtype=torch.int64)
    types = torch.zeros(B, Tm, dtype=torch.int64)
    qpos, lists = [], []
    for r, (T_, nq) in enumerate(zip(lens, n_queries)):
        row = rng.integers(106, shape.vocab, size=T_)
        row[0], row[-1] = 101, 102
        pos = sorted(rng.choice(np.arange(1, T_ - 1), size=nq, replace=False).tolist())
        row[pos] = shape.mask_id
        ids[r, :T_], am[r, :T_] = torch.from_numpy(row), 1
        types[r, T_ // 2:T_] = 1
        qpos.append(pos)
        for _ in pos:
            c = rng.integers(0, shape.vocab, size=int(rng.integers(1, max_list + 1))).tolist()
            if len(c) >= 3:
                c[2] = c[0]
            lists.append(c)
    return ids, am, types, qpos, lists


def _ragged(ids, am):
    lens = am.sum(1).tolist()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return torch.cat([ids[r, :n] for r, n in enumerate(lens)]).to(torch.int32).cuda(), off


def _score_cands(s, ids, am, qpos, lists, types=None):
    d_ids, off = _ragged(ids, am)
    q_off = np.concatenate([[0], np.cumsum([len(p) for p in qpos])]).astype(np.int32)
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int32)
    tt = None if types is None else _ragged(types, am)[0]
    out = s.score_cands(d_ids, off, q_off, np.asarray([p for ps in qpos for p in ps], np.int32), c_off,
                        np.asarray([x for c in lists for x in c], np.int32), token_types=tt)
    torch.cuda.synchronize()
    return out, c_off


def _multi_by_index(s, ids, am, qpos, lists, types=None):
    """rs_masked_logprob_multi once per candidate index j: entry j of every list that has one."""
    n_c = sum(len(c) for c in lists)
    c_off = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
    want = torch.zeros(n_c, dtype=torch.float32, device="cuda")
    rows = [r for r, ps in enumerate(qpos) for _ in ps]
    flat_pos = [p for ps in qpos for p in ps]
    for j in range(max(len(c) for c in lists)):
        labels = torch.full_like(ids, -100)
        for q, c in enumerate(lists):
            labels[rows[q], flat_pos[q]] = c[j] if j < len(c) else 0
        full = s.masked_logprob_multi(ids, am, labels, token_type_ids=types)
        for q, c in enumerate(lists):
            if j < len(c):
                want[c_off[q] + j] = full[rows[q], flat_pos[q]]
    return want


def _oracle(w, shape, ids, am, qpos, lists):
    """float64 log_softmax of the oracle's fp32 logits at every query, gathered at the candidates."""
    from oracle.bert_ref import TorchBert, set_cpu_threads
    set_cpu_threads()
    model = TorchBert(w, shape)
    with torch.no_grad():
        hid = model.encoder(ids, am)
        rows = [r for r, ps in enumerate(qpos) for _ in ps]
        lp = model.mlm_logits(hid[rows, [p for ps in qpos for p in ps], :]).double().log_softmax(dim=-1)
    return torch.cat([lp[q, torch.tensor(c)] for q, c in enumerate(lists)])


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_score_cands_tiny(w_tiny, precision):
    from asr_rescoring_amd.scorer import PLLScorer
    ids, am, types, qpos, lists = _rows(BERT_TINY, [5, 9, 34], [1, 3, 2], seed=3)
    assert min(map(len, lists)) >= 1 and max(map(len, lists)) <= 12
    s = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048, precision=precision)
    try:
        got, c_off = _score_cands(s, ids, am, qpos, lists)
        again, _ = _score_cands(s, ids, am, qpos, lists)
        want = _multi_by_index(s, ids, am, qpos, lists)
        got_t, _ = _score_cands(s, ids, am, qpos, lists, types)
        want_t = _multi_by_index(s, ids, am, qpos, lists, types)
        # the padded form: one query per row
        one = [[p[0]] for p in qpos]
        first = [lists[int(np.cumsum([0] + [len(p) for p in qpos])[r])] for r in range(len(qpos))]
        ids1 = ids.clone()
        for r, ps in enumerate(qpos):                    # only the first query of a row stays masked
            for p in ps[1:]:
                ids1[r, p] = 200 + p
        padded = s.masked_logprob_cands(ids1, am, [p[0] for p in one], first)
        flat1, _ = _score_cands(s, ids1, am, one, first)
    finally:
        s.close()
    assert got.dtype == torch.float32 and got.shape == (int(c_off[-1]),)
    assert torch.equal(_bits(got), _bits(again)), "run-to-run"
    assert torch.equal(_bits(got), _bits(want)), "score_cands != rs_masked_logprob_multi per candidate index"
    assert torch.equal(_bits(got_t), _bits(want_t)), "with token types: != rs_masked_logprob_multi"
    assert not torch.equal(_bits(got_t), _bits(got)), "the token types did not reach the call"
    assert [len(t) for t in padded] == [len(c) for c in first]
    assert torch.equal(_bits(torch.cat(padded)), _bits(flat1)), "masked_logprob_cands != score_cands"
    ref = _oracle(w_tiny, BERT_TINY, ids, am, qpos, lists)
    rel = ((got.cpu().double() - ref).abs() / ref.abs()).max().item()
    print(f"CANDS tiny {precision}: {len(lists)} queries, {int(c_off[-1])} candidates, max rel err vs oracle {rel:.2e}")
    assert rel < REL


def test_score_cands_chunked_is_bitwise(w_tiny):
    """max_rows 512 cuts 40 rows of 34 tokens into three chunks; candidates of later chunks land behind
    those of earlier ones.  Same bits as one chunk."""
    from asr_rescoring_amd.scorer import PLLScorer
    rng = np.random.default_rng(8)
    ids, am, _, qpos, lists = _rows(BERT_TINY, [34] * 40, rng.integers(1, 4, size=40).tolist(), seed=4)
    lists[5] = []                                        # an empty list in the middle of a chunk
    big = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=4096)
    small = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=512)
    try:
        a, c_off = _score_cands(big, ids, am, qpos, lists)
        b, _ = _score_cands(small, ids, am, qpos, lists)
        b2, _ = _score_cands(small, ids, am, qpos, lists[:-1] + [lists[-1] + [7, 7, 3]])   # the workspace grows
    finally:
        big.close()
        small.close()
    assert 40 * 34 > 2 * 512 and torch.isfinite(a).all()
    assert torch.equal(_bits(a), _bits(b)), "max_rows 512 vs 4096"
    assert torch.equal(_bits(b2[:len(b)]), _bits(b)), "a candidate's value depends on the other candidates"


def test_score_cands_base():
    from asr_rescoring_amd.scorer import PLLScorer
    w = make_weights(BERT_BASE, seed=1234, with_cls_linear=False, with_pooler=False)
    ids, am, _, qpos, lists = _rows(BERT_BASE, [7, 20], [1, 2], seed=6, max_list=4)
    s = PLLScorer(w, BERT_BASE, device=0, max_rows=4096, precision="fp16x3")
    try:
        got, _ = _score_cands(s, ids, am, qpos, lists)
        want = _multi_by_index(s, ids, am, qpos, lists)
    finally:
        s.close()
    assert torch.equal(_bits(got), _bits(want))
    ref = _oracle(w, BERT_BASE, ids, am, qpos, lists)
    assert ((got.cpu().double() - ref).abs() / ref.abs()).max().item() < REL


# ---- errors ----------------------------------------------------------------------------------------

def test_score_cands_errors(w_tiny):
    from asr_rescoring_amd._lib import RS_HEAD_CLS, RescoreError
    from asr_rescoring_amd.scorer import BertEngine, PLLScorer
    ids, am, _, qpos, lists = _rows(BERT_TINY, [5, 9, 34], [1, 3, 2], seed=3)
    s = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        good, _ = _score_cands(s, ids, am, qpos, lists)
        for bad in (-1, BERT_TINY.vocab):
            broken = [list(c) for c in lists]
            broken[2][-1] = bad
            with pytest.raises(RescoreError, match=r"error -1.*query 2\b") as e:
                _score_cands(s, ids, am, qpos, broken)
            assert e.value.code == -1
        # h_c_off not ascending: straight through the C ABI
        d_ids, off = _ragged(ids, am)
        q_off = np.asarray([0, 1, 4, 6], np.int32)
        qp = np.asarray([p for ps in qpos for p in ps], np.int32)
        c_off = np.asarray([0, 2, 1, 3, 4, 5, 6], np.int32)
        cand = np.zeros(6, np.int32)
        out = torch.zeros(6, dtype=torch.float32, device="cuda")
        rc = s.lib.rs_masked_logprob_cands(s.handle, d_ids.data_ptr(), off.ctypes.data, 3, q_off.ctypes.data, qp.ctypes.data,
                                           c_off.ctypes.data, cand.ctypes.data, out.data_ptr(), _lib.stream_ptr(0))
        assert rc == -1 and b"c_off" in s.lib.rs_last_error()
        # every list empty: succeeds, scores nothing
        none, _ = _score_cands(s, ids, am, qpos, [[] for _ in lists])
        assert none.numel() == 0
        after, _ = _score_cands(s, ids, am, qpos, lists)
        assert torch.equal(_bits(after), _bits(good))
    finally:
        s.close()
    e = BertEngine(w_tiny, BERT_TINY, heads=RS_HEAD_CLS, device=0, max_rows=2048)
    try:
        d_ids, off = _ragged(ids, am)
        rc = e.lib.rs_masked_logprob_cands(e.handle, d_ids.data_ptr(), off.ctypes.data, 3, q_off.ctypes.data, qp.ctypes.data,
                                           np.arange(7, dtype=np.int32).ctypes.data, cand.ctypes.data, out.data_ptr(),
                                           _lib.stream_ptr(0))
        assert rc == -3, (rc, e.lib.rs_last_error())      # RS_ESTATE: no MLM head
    finally:
        e.close()
