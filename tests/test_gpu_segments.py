"""GPU: segment ids (``rs_model_set_token_types``) through every scoring entry point, against the
float64 CPU reference with per-token types (tests/seg_ref.py), in both precision modes.

Inputs (BERT_TINY):
  * "pairs" — ``[CLS] context [SEP] hypothesis [SEP]`` with context lengths CTX_L and hypothesis
    lengths HYP_L (``data.with_context``: types 0 / 1, only the hypothesis half scored).  Every
    T <= 64, so fp16x3 keeps its layer-0 dedup, and the type boundary (position C + 2) falls on
    both sides of the 16-key tile edges;
  * "long" — the same plus pairs of T = 65 and T = 130 (fp16x3 chunks without dedup, three key
    blocks);
  * "random" — the tokens of "pairs" with a random 0/1 type per token and every position scored: an
    index taken per row or per chunk instead of per token cannot pass.
Tolerances are those of the files that check the same quantities without types: REL / REL_BATCH of
test_gpu_spans.py, the CLS bound of test_gpu_bert.py, the embedding bounds of test_gpu_bertscore.py.
"""
import dataclasses

import numpy as np
import pytest
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights

import seg_ref

pytestmark = pytest.mark.gpu

REL = 1e-3          # against the reference (test_gpu_spans.py, test_gpu_bert.py)
REL_BATCH = 1e-5    # the same rows in another batch composition (test_gpu_spans.py)
CTX_L = [0, 1, 13, 30]
HYP_L = [1, 2, 15, 16, 17, 31]
LONG = [(30, 32), (60, 67)]          # (context, hypothesis): T = C + L + 3 = 65, 130
PRECS = ["fp16", "fp16x3"]


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def _words(rng, n):
    """uint8 [n]: seeded word lengths 1..4."""
    ws = np.zeros(n, np.uint8)
    p = 0
    while p < n:
        ws[p] = 1
        p += int(rng.integers(1, 5))
    return ws


def _make_pairs(seed, groups, vocab=BERT_TINY.vocab):
    """groups: (context length, [hypothesis lengths]) per utterance."""
    rng = np.random.default_rng(seed)
    toks, off, uoff, ws, ctx, coff, cws = [], [0], [0], [], [], [0], []
    for C, lens in groups:
        for L in lens:
            toks += [D.CLS_ID] + rng.integers(D.FIRST_WORD_ID, vocab, size=L).tolist() + [D.SEP_ID]
            ws += [1] + _words(rng, L).tolist() + [1]
            off.append(len(toks))
        uoff.append(len(off) - 1)
        ctx += rng.integers(D.FIRST_WORD_ID, vocab, size=C).tolist()
        cws += _words(rng, C).tolist()
        coff.append(len(ctx))
    tokens, hyp_off, types, score_from, word_start = D.with_context(
        np.asarray(toks, np.int32), off, uoff, np.asarray(ctx, np.int32), coff, 512, np.asarray(ws, np.uint8),
        np.asarray(cws, np.uint8))
    return dict(tokens=tokens, off=hyp_off, types=types.astype(np.int32), sf=score_from, ws=word_start)


PAIR_GROUPS = [(C, HYP_L) for C in CTX_L]
SETS = {"pairs": _make_pairs(21, PAIR_GROUPS), "long": _make_pairs(21, PAIR_GROUPS + [(C, [L]) for C, L in LONG])}
N_PAIR_HYP = len(CTX_L) * len(HYP_L)
assert np.array_equal(SETS["long"]["tokens"][:len(SETS["pairs"]["tokens"])], SETS["pairs"]["tokens"])
assert int(np.diff(SETS["pairs"]["off"]).max()) == 64 and np.diff(SETS["long"]["off"])[-2:].tolist() == [65, 130]
_rng = np.random.default_rng(22)
SETS["random"] = dict(SETS["pairs"], types=_rng.integers(0, 2, len(SETS["pairs"]["tokens"])).astype(np.int32), sf=None)


@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def scorers(w_tiny):
    """BERT_TINY PLL scorers by (precision, max_rows), made on first use."""
    from asr_rescoring_amd.scorer import PLLScorer
    made = {}

    def get(prec, max_rows=65536):
        if (prec, max_rows) not in made:
            made[(prec, max_rows)] = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=max_rows, precision=prec)
        return made[(prec, max_rows)]
    yield get
    for s in made.values():
        s.close()


_ref = {}


def _spans(name, variant):
    s = SETS[name]
    return D.pll_spans(s["off"], s["ws"], variant, score_from=s["sf"])


def _reference(w, name, variant):
    """(log-softmax rows float64 [R, vocab], label log-probs [R]) of seg_ref, computed once.  The rows
    of "pairs" are the first rows of "long"."""
    if name == "pairs":
        lsm, lp = _reference(w, "long", variant)
        n = int(_spans("pairs", variant)[0][-1])
        return lsm[:n], lp[:n]
    if (name, variant) not in _ref:
        s = SETS[name]
        spans = _spans(name, variant)
        lsm = seg_ref.span_rows(seg_ref.SegBert(w, BERT_TINY), s["tokens"], s["off"], s["types"], *spans)
        _ref[(name, variant)] = (lsm, seg_ref.row_logprobs(lsm, s["tokens"], s["off"], spans[0], spans[3]))
    return _ref[(name, variant)]


def _score(s, name, variant="original", types="set", **kw):
    st = SETS[name]
    tt = st["types"] if isinstance(types, str) else types
    pll, rows = s.score_nbest(st["tokens"], st["off"], return_rows=True, variant=variant, word_start=st["ws"],
                              token_types=tt, score_from=st["sf"], **kw)
    return pll.cpu().numpy(), rows.cpu().numpy()


# ---- 1. against the reference ---------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("variant", D.PLL_VARIANTS)
@pytest.mark.parametrize("name", ["pairs", "long"])
def test_context_pairs_match_reference(scorers, w_tiny, name, variant, prec):
    pll, rows = _score(scorers(prec), name, variant)
    _, ref = _reference(w_tiny, name, variant)
    spans = _spans(name, variant)
    assert len(rows) == len(ref) == int(np.sum(np.diff(SETS[name]["off"]) - SETS[name]["sf"] - 1))
    e_row, e_hyp = rel_err(rows, ref).max(), rel_err(pll, seg_ref.sum_rows(ref, spans[0])).max()
    print(f"{name} {variant} {prec}: vs seg_ref max rel rows {e_row:.3e}, PLL {e_hyp:.3e}")
    assert e_row < REL and e_hyp < REL
    if variant != "original":
        assert (spans[2] - spans[1] > 1).any()


@pytest.mark.parametrize("prec", PRECS)
def test_random_types_match_reference(scorers, w_tiny, prec):
    pll, rows = _score(scorers(prec), "random")
    _, ref = _reference(w_tiny, "random", "original")
    row_off = _spans("random", "original")[0]
    e_row, e_hyp = rel_err(rows, ref).max(), rel_err(pll, seg_ref.sum_rows(ref, row_off)).max()
    print(f"random types {prec}: vs seg_ref max rel rows {e_row:.3e}, PLL {e_hyp:.3e}")
    assert e_row < REL and e_hyp < REL


# ---- 2. the types move the scores -----------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_types_move_the_rows(scorers, prec):
    s = scorers(prec)
    _, typed = _score(s, "pairs")
    _, zero = _score(s, "pairs", types=None)
    shift = rel_err(typed, zero)
    frac = float((shift > 10 * REL).mean())
    print(f"pairs {prec}: typed vs zero-type rows: min shift {shift.min():.3e}, median {np.median(shift):.3e}, "
          f"rows moved by more than {10 * REL:g}: {frac:.3f}")
    assert frac >= 0.5


# ---- 3. no-op and state ---------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_setter_is_one_shot_and_zero_types_are_a_no_op(scorers, w_tiny, prec):
    from asr_rescoring_amd import _lib
    from asr_rescoring_amd.scorer import PLLScorer
    st = SETS["random"]
    fresh = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=65536, precision=prec)
    try:
        plain = fresh.score_nbest(st["tokens"], st["off"], return_rows=True)[1].cpu().numpy()
    finally:
        fresh.close()
    s = scorers(prec)

    def rows(types=None):
        return s.score_nbest(st["tokens"], st["off"], return_rows=True, token_types=types)[1].cpu().numpy()
    typed = rows(st["types"])
    assert np.array_equal(rows(), plain)                                   # right after a typed call
    assert (typed != plain).any()
    assert np.array_equal(rows(np.zeros_like(st["types"])), plain)         # explicit zeros
    with pytest.raises(_lib.RescoreError, match=r"error -1: rs_model_set_token_types gave \d+ token types, this call "
                                                r"addresses \d+ tokens"):
        rows(st["types"][:-1])
    assert np.array_equal(rows(), plain)                                   # the failed call consumed the setting
    d_type = s._set_types(st["types"])
    s.clear_token_types()                                                  # d_type == NULL
    assert np.array_equal(rows(), plain)
    d_type = s._set_types(st["types"])                                     # noqa: F841
    assert s.score_nbest(np.zeros(0, np.int32), [0]).shape == (0,)         # n_hyp == 0 consumes it too
    assert np.array_equal(rows(), plain)
    assert np.array_equal(rows(st["types"]), typed)


# ---- 4. dedup on / off ----------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,variant", [(n, v) for n in ("pairs", "long") for v in D.PLL_VARIANTS]
                         + [("random", "original")])       # "random": every position, through rs_pll_score
def test_dedup_is_exact_with_types(scorers, name, variant, prec, monkeypatch):
    s = scorers(prec)
    out, flops = {}, {}
    for dd in ("1", "0"):
        monkeypatch.setenv("RS_DEDUP", dd)
        s.profile(True)
        out[dd] = _score(s, name, variant)
        flops[dd] = s.profile_read()["qkv"][2]
        s.profile(False)
    assert np.array_equal(out["1"][1], out["0"][1]) and np.array_equal(out["1"][0], out["0"][0])
    if name != "long":
        print(f"{name} {variant} {prec}: QKV flops dedup {flops['1']:.4g}, plain {flops['0']:.4g}")
        assert 0 < flops["1"] < flops["0"]                # the plan was used


# ---- 5. copies of one pair cut across chunks -------------------------------------------------

# Sets whose sequences all have T <= 64 in both precisions, "long" in fp16x3 only: in the fp16 mode a
# chunk's longest sequence picks its attention kernel (test_gpu_spans.py _masked_rows), so a
# 512-row chunk of short pairs and the one big chunk that also holds T = 130 run different kernels
# and rows move by ~1e-4 with or without types (measured on "long", fp16: 1.631e-4 with types,
# 1.646e-4 without; every case below: 0.0).  That is chunking in fp16, not segment ids.
@pytest.mark.parametrize("name,prec", [("pairs", "fp16"), ("pairs", "fp16x3"), ("random", "fp16"),
                                       ("random", "fp16x3"), ("long", "fp16x3")])
def test_chunking_with_types(scorers, name, prec):
    small, big = _score(scorers(prec, 512), name), _score(scorers(prec, 65536), name)
    e_row, e_hyp = rel_err(small[1], big[1]).max(), rel_err(small[0], big[0]).max()
    print(f"{name} {prec}: max_rows 512 vs 65536 max rel rows {e_row:.3e}, PLL {e_hyp:.3e}")
    # the same comparison without types (a figure, not a check): what chunking alone moves
    small0, big0 = _score(scorers(prec, 512), name, types=None), _score(scorers(prec, 65536), name, types=None)
    print(f"{name} {prec}: the same without types: rows {rel_err(small0[1], big0[1]).max():.3e}, "
          f"PLL {rel_err(small0[0], big0[0]).max():.3e}")
    assert e_row < REL_BATCH and e_hyp < REL_BATCH


# ---- 6. top-k with types --------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_pll_topk_with_types(scorers, w_tiny, prec):
    st = SETS["random"]
    s = scorers(prec)
    pll, rows = s.score_nbest(st["tokens"], st["off"], return_rows=True, token_types=st["types"])
    top_id, top_lp, pll_k, rows_k = s.topk_nbest(st["tokens"], st["off"], k=3, return_pll=True, token_types=st["types"])
    assert np.array_equal(rows_k.cpu().numpy(), rows.cpu().numpy())
    assert np.array_equal(pll_k.cpu().numpy(), pll.cpu().numpy())
    lsm, _ = _reference(w_tiny, "random", "original")
    best = np.sort(lsm, axis=1)[:, -2:]
    clear = best[:, 1] - best[:, 0] > 1e-3
    assert clear.mean() > 0.5
    assert np.array_equal(top_id.cpu().numpy()[clear, 0], lsm.argmax(axis=1)[clear])
    assert rel_err(top_lp.cpu().numpy()[clear, 0], best[clear, 1]).max() < REL


# ---- 7. padded token_type_ids ---------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_padded_token_type_ids_equal_the_ragged_path(scorers, prec):
    from asr_rescoring_amd import _lib
    st = SETS["random"]
    s = scorers(prec)
    hyps = [3, 9, 14, 20]                                  # T = 18, 20, 31, 48
    off = np.zeros(len(hyps) + 1, np.int32)
    off[1:] = np.cumsum([st["off"][h + 1] - st["off"][h] for h in hyps])
    ids = np.concatenate([st["tokens"][st["off"][h]:st["off"][h + 1]] for h in hyps]).astype(np.int32)
    types = np.concatenate([st["types"][st["off"][h]:st["off"][h + 1]] for h in hyps]).astype(np.int32)
    assert np.diff(off).tolist() == [18, 20, 31, 48]
    mp = np.asarray([1, 7, 29, 34], np.int32)
    lab = ids[off[:-1] + mp].copy()
    ids[off[:-1] + mp] = D.MASK_ID
    B, T = len(hyps), int(np.diff(off).max())
    p_ids, p_am, p_tt = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64), np.ones((B, T), np.int64)
    p_lab = np.zeros((B, T), np.int64)
    for i in range(B):
        n = off[i + 1] - off[i]
        p_ids[i, :n], p_am[i, :n], p_tt[i, :n] = ids[off[i]:off[i + 1]], 1, types[off[i]:off[i + 1]]
        p_lab[i, mp[i]] = lab[i]
    t = torch.from_numpy
    got = s.masked_logprob(t(p_ids), t(p_am), t(p_lab), mp, token_type_ids=t(p_tt))
    untyped = s.masked_logprob(t(p_ids), t(p_am), t(p_lab), mp)
    top_id, top_lp = s.masked_topk(t(p_ids), t(p_am), mp, k=4, token_type_ids=t(p_tt))
    # the ragged path: the C entry points on the unpadded arrays
    d_ids, d_lab = s._dev_tokens(ids), s._dev_tokens(lab)
    out = torch.empty(B, dtype=torch.float32, device=s.device)
    d_type = s._set_types(types)
    _lib.check(s.lib.rs_masked_logprob(s.handle, _lib.ptr(d_ids), off.ctypes.data, mp.ctypes.data, _lib.ptr(d_lab), B,
                                       _lib.ptr(out), _lib.stream_ptr(s.device)))
    r_id = torch.empty((B, 4), dtype=torch.int32, device=s.device)
    r_lp = torch.empty((B, 4), dtype=torch.float32, device=s.device)
    d_type = s._set_types(types)                           # noqa: F841
    _lib.check(s.lib.rs_masked_topk(s.handle, _lib.ptr(d_ids), off.ctypes.data, mp.ctypes.data, B, 4, _lib.ptr(r_id),
                                    _lib.ptr(r_lp), _lib.stream_ptr(s.device)))
    assert np.array_equal(got.cpu().numpy(), out.cpu().numpy())
    assert (got.cpu().numpy() != untyped.cpu().numpy()).any()
    assert np.array_equal(top_id.cpu().numpy(), r_id.cpu().numpy())
    assert np.array_equal(top_lp.cpu().numpy(), r_lp.cpu().numpy())
    with pytest.raises(ValueError):
        s.masked_logprob(t(p_ids), t(p_am), t(p_lab), mp, token_type_ids=t(p_tt[:, :-1]))


# ---- 8. RescoreBert -------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_cls_scores_with_types(w_tiny, prec):
    from asr_rescoring_amd.scorer import RescoreBertHIP
    st = SETS["long"]
    ref = seg_ref.cls_scores(seg_ref.SegBert(w_tiny, BERT_TINY), st["tokens"], st["off"], st["types"])
    zero = seg_ref.cls_scores(seg_ref.SegBert(w_tiny, BERT_TINY), st["tokens"], st["off"], np.zeros_like(st["types"]))
    assert np.abs(ref - zero).max() > 100 * 1e-4
    m = RescoreBertHIP(w_tiny, BERT_TINY, device=0, max_rows=4096, precision=prec)
    try:
        got = m.engine.score_nbest(st["tokens"], st["off"], token_types=st["types"]).cpu().numpy()
        lens = np.diff(st["off"])
        B, T = len(lens), int(lens.max())
        ids, am, tt = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64), np.ones((B, T), np.int64)
        for i in range(B):
            a, b = st["off"][i], st["off"][i + 1]
            ids[i, :b - a], am[i, :b - a], tt[i, :b - a] = st["tokens"][a:b], 1, st["types"][a:b]
        fwd = m(torch.from_numpy(ids), torch.from_numpy(am), token_type_ids=torch.from_numpy(tt)).cpu().numpy()
        plain = m(torch.from_numpy(ids), torch.from_numpy(am)).cpu().numpy()
    finally:
        m.engine.close()
    err = np.abs(got - ref)
    print(f"CLS {prec}: vs seg_ref max abs {err.max():.3e}")
    assert (err <= np.maximum(REL * np.abs(ref), 1e-4)).all(), err.max()
    assert np.array_equal(fwd, got)
    assert (np.abs(plain - zero) <= np.maximum(REL * np.abs(zero), 1e-4)).all()


# ---- 9. a third type ------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_type_vocab_3(prec):
    from asr_rescoring_amd.scorer import PLLScorer
    shape = dataclasses.replace(BERT_TINY, type_vocab=3)
    w = make_weights(shape, seed=8)
    assert w["bert.embeddings.token_type_embeddings.weight"].shape == (3, shape.hidden)
    st = SETS["pairs"]
    types = np.random.default_rng(23).integers(0, 3, len(st["tokens"])).astype(np.int32)
    assert set(types.tolist()) == {0, 1, 2}
    spans = D.pll_spans(st["off"], None, "original", score_from=st["sf"])
    lsm = seg_ref.span_rows(seg_ref.SegBert(w, shape), st["tokens"], st["off"], types, *spans)
    ref = seg_ref.row_logprobs(lsm, st["tokens"], st["off"], spans[0], spans[3])
    s = PLLScorer(w, shape, device=0, max_rows=65536, precision=prec)
    try:
        pll, rows = s.score_nbest(st["tokens"], st["off"], return_rows=True, token_types=types, score_from=st["sf"])
        two = s.score_nbest(st["tokens"], st["off"], return_rows=True, token_types=np.minimum(types, 1),
                            score_from=st["sf"])[1]
        bad = types.copy()
        bad[5] = 3
        with pytest.raises(ValueError):
            s.score_nbest(st["tokens"], st["off"], token_types=bad, score_from=st["sf"])
        with pytest.raises(ValueError):
            s.score_nbest(st["tokens"], st["off"], token_types=-bad)
        again = s.score_nbest(st["tokens"], st["off"], return_rows=True, score_from=st["sf"])[1]     # nothing pending
        zero = s.score_nbest(st["tokens"], st["off"], return_rows=True, token_types=np.zeros_like(types),
                             score_from=st["sf"])[1]
    finally:
        s.close()
    e_row = rel_err(rows.cpu().numpy(), ref).max()
    e_hyp = rel_err(pll.cpu().numpy(), seg_ref.sum_rows(ref, spans[0])).max()
    print(f"type_vocab 3 {prec}: vs seg_ref max rel rows {e_row:.3e}, PLL {e_hyp:.3e}")
    assert e_row < REL and e_hyp < REL
    assert (two.cpu().numpy() != rows.cpu().numpy()).any()                 # row 2 is not row 1
    assert np.array_equal(again.cpu().numpy(), zero.cpu().numpy())


# ---- 10. token embeddings -------------------------------------------------------------------

def test_embed_with_types(w_tiny):
    from asr_rescoring_amd.bertscore import BertScorer
    st = SETS["long"]
    hid = np.concatenate(seg_ref.hidden_states(seg_ref.SegBert(w_tiny, BERT_TINY), st["tokens"], st["off"], st["types"]))
    ref = hid / np.linalg.norm(hid, axis=1, keepdims=True)
    for prec, tol_e in (("fp16x3", 2e-6), ("fp16", 5e-3)):             # test_gpu_bertscore.py test_embed_rows_are_unit_norm
        s = BertScorer(w_tiny, BERT_TINY, num_layers=BERT_TINY.layers, device=0, precision=prec)
        try:
            e = s.embed(st["tokens"], st["off"], token_types=st["types"]).float().cpu().numpy()
            plain = s.embed(st["tokens"], st["off"]).float().cpu().numpy()
        finally:
            s.close()
        err = np.abs(e - ref).max()
        print(f"embed {prec}: vs seg_ref max abs {err:.3e}")
        assert err < tol_e, prec
        assert np.abs(plain - ref).max() > 10 * tol_e          # untyped rows are far outside the bound
