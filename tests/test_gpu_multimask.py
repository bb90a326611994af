"""GPU: multi-mask rows (``rs_pll_score_sets`` / ``PLLScorer.score_sets``, the strided PLL
approximation of ``data.pll_strided``, and ``rs_masked_logprob_multi`` /
``PLLScorer.masked_logprob_multi``): several [MASK] positions in one row, all of them scored from
that row's one forward.

Checked against the CPU oracle (every scored position as a row of its own, masked on the host),
against the product's single-query path (``masked_logprob`` on the same host-masked rows,
``score_nbest`` for the singleton rows), and for the exact properties: the float64 sum, run-to-run
bits, and a query's independence of its row's other queries.

Inputs are the seeded sets of test_gpu_spans.py: "short" (L in SHORT_L, every T <= 64) and "mixed"
(plus L = 63 and L = 130: T = 65 and three key blocks).
"""
import json

import numpy as np
import pytest
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_BASE, BERT_TINY, make_weights

from test_gpu_spans import MIXED_L, REL, REL_BATCH, SETS, _make_set, rel_err

pytestmark = pytest.mark.gpu

PRECS = ["fp16", "fp16x3"]
STRIDES = [1, 2, 3, 4, 16]


@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def scorers(w_tiny):
    """BERT_TINY scorers by (precision, max_rows), made on first use."""
    from asr_rescoring_amd.scorer import PLLScorer
    made = {}

    def get(prec, max_rows=65536):
        if (prec, max_rows) not in made:
            made[(prec, max_rows)] = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=max_rows, precision=prec)
        return made[(prec, max_rows)]
    yield get
    for s in made.values():
        s.close()


def _entry_rows(tokens, hyp_off, plan, mask_id=D.MASK_ID):
    """One host-masked row per scored position (the row that holds it, repeated): padded
    (input_ids, attention_mask, labels) int64 and the query position of every entry."""
    row_off, pos_off, pos = plan
    hyp = np.repeat(np.arange(len(hyp_off) - 1), np.diff(row_off))
    row = np.repeat(np.arange(len(pos_off) - 1), np.diff(pos_off))
    T = np.diff(hyp_off)[hyp[row]] if len(row) else np.zeros(0, np.int64)
    tmax = int(T.max()) if len(T) else 1
    ids = np.zeros((len(pos), tmax), np.int64)
    am = np.zeros((len(pos), tmax), np.int64)
    lab = np.zeros((len(pos), tmax), np.int64)
    for i, r in enumerate(row):
        seg = tokens[hyp_off[hyp[r]]:hyp_off[hyp[r] + 1]]
        ids[i, :T[i]] = seg
        lab[i, :T[i]] = seg
        am[i, :T[i]] = 1
        ids[i, pos[pos_off[r]:pos_off[r + 1]]] = mask_id
    return ids, am, lab, np.asarray(pos, np.int64)


def _sum_entries(vals, plan):
    """Python float64 sum of every hypothesis' entries in list order."""
    row_off, pos_off, _ = plan
    out = np.zeros(len(row_off) - 1, np.float64)
    for h in range(len(out)):
        acc = 0.0
        for i in range(pos_off[row_off[h]], pos_off[row_off[h + 1]]):
            acc += float(vals[i])
        out[h] = acc
    return out


def _free_plan(off, seed=31):
    """The L = 130 hypothesis gets rows of 1, 15, 16, 17, 64, 65 and all 130 positions; the larger
    rows hold its first and last position and the adjacent pair 64, 65 (the key-block edge).  L = 15:
    no rows (PLL 0.0).  Every other hypothesis: its odd positions in one row, then its last alone."""
    rng = np.random.default_rng(seed)
    row_off, pos_off, pos = [0], [0], []
    for h in range(len(off) - 1):
        L = int(off[h + 1] - off[h]) - 2
        rows = []
        if L == 130:
            for n in (1, 15, 16, 17, 64, 65, 130):
                if n == 1:
                    rows.append([L])
                    continue
                forced = [1, 64, 65, L]
                rest = rng.permutation(np.setdiff1d(np.arange(1, L + 1), forced))[:n - len(forced)]
                rows.append(sorted(forced + rest.tolist()))
        elif L != 15:
            rows = [list(range(1, L + 1, 2)), [L]]
        for r in rows:
            pos += r
            pos_off.append(len(pos))
        row_off.append(len(pos_off) - 1)
    return tuple(np.asarray(x, np.int32) for x in (row_off, pos_off, pos))


def _plan(name, what):
    off = SETS[name][1]
    return _free_plan(off) if what == "free" else D.pll_strided(off, what)


_oracle = {}


def _oracle_entries(w, name, what):
    """Oracle log-prob of every entry of a plan, computed once."""
    if (name, what) not in _oracle:
        from oracle.bert_ref import TorchBert, masked_logprob_ref
        tokens, off, _ = SETS[name]
        ids, am, lab, q = _entry_rows(tokens, off, _plan(name, what))
        _oracle[(name, what)] = masked_logprob_ref(TorchBert(w, BERT_TINY), ids, am, lab, q)
    return _oracle[(name, what)]


# ---- 1. against the oracle --------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
@pytest.mark.parametrize("what", STRIDES + ["free"])
def test_sets_match_oracle(scorers, w_tiny, what, max_rows, prec):
    tokens, off, _ = SETS["mixed"]
    plan = _plan("mixed", what)
    if what == "free":
        sizes = np.diff(plan[1]).tolist()
        assert all(n in sizes for n in (1, 15, 16, 17, 64, 65, 130))
    ref = _oracle_entries(w_tiny, "mixed", what)
    pll, rows = scorers(prec, max_rows).score_sets(tokens, off, *plan, return_rows=True)
    pll, rows = pll.cpu().numpy(), rows.cpu().numpy()
    assert rows.shape == ref.shape and pll.shape == (len(off) - 1,)
    ref_pll = _sum_entries(ref, plan)
    scored = ref_pll != 0.0
    e_pos = rel_err(rows, ref).max()
    e_hyp = rel_err(pll[scored], ref_pll[scored]).max()
    print(f"sets {what} {prec} max_rows={max_rows}: vs oracle max rel positions {e_pos:.3e}, hypotheses {e_hyp:.3e}")
    assert e_pos < REL and e_hyp < REL
    assert (pll[~scored] == 0.0).all()
    if what == "free":
        assert pll[MIXED_L.index(15)] == 0.0 and not scored[MIXED_L.index(15)]


# ---- 2. against the single-query path ---------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("what", [2, 4, "free"])
def test_sets_match_single_query_rows(scorers, what, prec):
    tokens, off, _ = SETS["mixed"]
    plan = _plan("mixed", what)
    s = scorers(prec, 65536)
    rows = s.score_sets(tokens, off, *plan, return_rows=True)[1].cpu().numpy()
    ids, am, lab, q = _entry_rows(tokens, off, plan)
    ref = s.masked_logprob(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(lab), q).cpu().numpy()
    err = rel_err(rows, ref).max()
    print(f"sets {what} {prec}: positions vs masked_logprob max rel {err:.3e}")
    assert err < REL_BATCH


@pytest.mark.parametrize("prec", PRECS)
def test_large_stride_is_pll_and_small_stride_is_not(scorers, prec):
    tokens, off, _ = SETS["mixed"]
    s = scorers(prec, 65536)
    pll0, rows0 = (x.cpu().numpy() for x in s.score_nbest(tokens, off, return_rows=True))
    pll, rows = (x.cpu().numpy() for x in s.score_nbest(tokens, off, return_rows=True, variant="strided", stride=200))
    e_pos, e_hyp = rel_err(rows, rows0).max(), rel_err(pll, pll0).max()
    print(f"stride >= L {prec}: vs score_nbest max rel positions {e_pos:.3e}, PLL {e_hyp:.3e}")
    assert e_pos < REL_BATCH and e_hyp < REL_BATCH
    # stride 2: the same positions in pll_strided's order (odd, then even), scored with half of the
    # other tokens hidden as well
    plan = D.pll_strided(off, 2)
    rows2 = s.score_nbest(tokens, off, return_rows=True, variant="strided", stride=2)[1].cpu().numpy()
    order = np.concatenate([off[h] - 2 * h + plan[2][plan[1][plan[0][h]]:plan[1][plan[0][h + 1]]] - 1
                            for h in range(len(off) - 1)])
    assert sorted(order.tolist()) == list(range(len(rows0)))
    assert (rows2 != rows0[order]).any()
    with pytest.raises(ValueError):
        s.score_nbest(tokens, off, variant="strided")          # stride 0


# ---- 3. exact properties ----------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("max_rows", [512, 65536])
def test_sum_and_reproducibility(scorers, max_rows, prec):
    tokens, off, _ = SETS["mixed"]
    s = scorers(prec, max_rows)
    for what in (3, "free"):
        plan = _plan("mixed", what)
        pll, rows = (x.cpu().numpy() for x in s.score_sets(tokens, off, *plan, return_rows=True))
        assert np.array_equal(pll, _sum_entries(rows, plan))
        pll_b, rows_b = (x.cpu().numpy() for x in s.score_sets(tokens, off, *plan, return_rows=True))
        assert np.array_equal(rows, rows_b) and np.array_equal(pll, pll_b)
        assert np.array_equal(s.score_sets(tokens, off, *plan).cpu().numpy(), pll)     # without d_pos_lp


@pytest.mark.parametrize("prec", PRECS)
def test_query_does_not_depend_on_other_queries(scorers, prec):
    """One row masked at six positions: a query alone and among the others gives the same bits,
    whichever place it has in the row's query list."""
    tokens, off, _ = SETS["mixed"]
    h = MIXED_L.index(130)
    seq = tokens[off[h]:off[h + 1]].astype(np.int64)
    masked = [1, 40, 64, 65, 100, 130]
    ids = seq.copy()
    ids[masked] = D.MASK_ID
    s = scorers(prec, 65536)

    def run(qs):
        lab = np.full_like(seq, -100)
        lab[qs] = seq[qs]
        out = s.masked_logprob_multi(torch.from_numpy(ids[None]), torch.ones((1, len(ids)), dtype=torch.int64),
                                     torch.from_numpy(lab[None])).cpu().numpy()[0]
        assert np.isfinite(out[qs]).all() and np.isnan(np.delete(out, qs)).all()
        return out

    full = run(masked)
    for p in masked:
        assert run([p])[p] == full[p]
    three = run([40, 65, 130])
    assert np.array_equal(three[[40, 65, 130]], full[[40, 65, 130]])


# ---- 4. masked_logprob_multi ------------------------------------------------------------------

def _multi_batch(seed=41):
    """"short" as a padded batch: row i masks and labels n_i positions of [0, T) (n_i runs over
    1 .. T - 2 across the rows, [CLS] and [SEP] may be among them); labels are the original tokens,
    the first scored position of every third row is labelled 0, of the next vocab - 1."""
    tokens, off, _ = SETS["short"]
    rng = np.random.default_rng(seed)
    B, tmax = len(off) - 1, int(np.diff(off).max())
    ids = np.zeros((B, tmax), np.int64)
    am = np.zeros((B, tmax), np.int64)
    lab = np.full((B, tmax), -100, np.int64)
    for i in range(B):
        T = int(off[i + 1] - off[i])
        ids[i, :T] = tokens[off[i]:off[i + 1]]
        am[i, :T] = 1
        n = [1, T - 2, max(T // 2, 1)][i % 3] if T > 3 else 1
        q = np.sort(rng.permutation(T)[:n])
        lab[i, q] = ids[i, q]
        if i % 3 == 0:
            lab[i, q[0]] = 0
        if i % 3 == 1:
            lab[i, q[0]] = BERT_TINY.vocab - 1
        ids[i, q] = D.MASK_ID
    return ids, am, lab


@pytest.mark.parametrize("prec", PRECS)
def test_masked_logprob_multi(scorers, w_tiny, prec):
    from asr_rescoring_amd import _lib
    from oracle.bert_ref import TorchBert, masked_logprob_ref
    ids, am, lab = _multi_batch()
    counts = (lab != -100).sum(1)
    T = am.sum(1)
    assert counts.min() == 1 and (counts == T - 2).any() and (lab == 0).any() and (lab == BERT_TINY.vocab - 1).any()
    if "multi" not in _oracle:
        b, t = np.nonzero(lab != -100)
        _oracle["multi"] = (b, t, masked_logprob_ref(TorchBert(w_tiny, BERT_TINY), ids[b], am[b], lab[b], t))
    b, t, ref = _oracle["multi"]
    s = scorers(prec, 65536)
    out = s.masked_logprob_multi(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(lab)).cpu().numpy()
    assert out.shape == ids.shape and out.dtype == np.float32
    assert np.array_equal(np.isnan(out), lab == -100)
    err = rel_err(out[b, t], ref).max()
    print(f"masked_logprob_multi {prec}: vs oracle max rel {err:.3e}")
    assert err < REL
    bad = lab.copy()
    bad[b[-1], t[-1]] = BERT_TINY.vocab                     # one label outside the vocabulary
    with pytest.raises(_lib.RescoreError, match="librescore error -5"):           # RS_EUNSUP
        s.masked_logprob_multi(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(bad))
    with pytest.raises(ValueError):                                                # a label in the padding
        pad = lab.copy()
        pad[0, -1] = 5
        assert am[0, -1] == 0
        s.masked_logprob_multi(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(pad))


# ---- 5. layer-form switches -------------------------------------------------------------------

@pytest.mark.parametrize("switch", ["RS_LASTQ", "RS_X3S_IMGRES", "RS_X3S"])
def test_layer_forms(scorers, w_tiny, switch, monkeypatch):
    """RS_LASTQ=0: Q of the query rows read from qkv; RS_X3S_IMGRES=0 / RS_X3S=0: the residual from
    the fp32 pre-LN stream and its statistics."""
    from oracle.bert_ref import TorchBert, masked_logprob_ref
    tokens, off, _ = SETS["short"]
    plan = D.pll_strided(off, 3)
    if ("short", 3) not in _oracle:
        ids, am, lab, q = _entry_rows(tokens, off, plan)
        _oracle[("short", 3)] = masked_logprob_ref(TorchBert(w_tiny, BERT_TINY), ids, am, lab, q)
    ref = _oracle[("short", 3)]
    monkeypatch.setenv(switch, "0")
    pll, rows = (x.cpu().numpy() for x in scorers("fp16x3", 65536).score_sets(tokens, off, *plan, return_rows=True))
    e_pos, e_hyp = rel_err(rows, ref).max(), rel_err(pll, _sum_entries(ref, plan)).max()
    print(f"{switch}=0: vs oracle max rel positions {e_pos:.3e}, hypotheses {e_hyp:.3e}")
    assert e_pos < REL and e_hyp < REL


# ---- 6. segment ids ---------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_sets_with_segment_ids(scorers, w_tiny, prec):
    import seg_ref
    from test_gpu_segments import SETS as SEG_SETS
    st = SEG_SETS["long"]
    tokens, off, types, sf = st["tokens"], st["off"], st["types"], st["sf"]
    plan = D.pll_strided(off, 3, score_from=sf)
    if "seg" not in _oracle:
        model = seg_ref.SegBert(w_tiny, BERT_TINY)
        ids, am, _, q = _entry_rows(tokens, off, plan)
        first = np.concatenate([[True], np.any(ids[1:] != ids[:-1], axis=1) | (am[1:] != am[:-1]).any(axis=1)])
        hyp = np.repeat(np.arange(len(off) - 1), np.diff(plan[0]))[np.repeat(np.arange(len(plan[1]) - 1), np.diff(plan[1]))]
        ref = np.zeros(len(q))
        with torch.no_grad():
            for i in np.flatnonzero(first):                 # one forward per distinct masked row
                T = int(am[i].sum())
                same = [j for j in range(i, len(q)) if hyp[j] == hyp[i] and np.array_equal(ids[j], ids[i])]
                tt = torch.from_numpy(types[off[hyp[i]]:off[hyp[i] + 1]].astype(np.int64))[None]
                hid = model.encoder(torch.from_numpy(ids[i:i + 1, :T]), torch.ones((1, T), dtype=torch.int64), tt)
                lsm = model.mlm_logits(hid[0]).log_softmax(dim=-1).numpy()
                for j in same:
                    ref[j] = lsm[q[j], tokens[off[hyp[j]] + q[j]]]
        _oracle["seg"] = ref
    ref = _oracle["seg"]
    s = scorers(prec, 65536)
    pll, rows = (x.cpu().numpy() for x in s.score_sets(tokens, off, *plan, return_rows=True, token_types=types))
    e_pos, e_hyp = rel_err(rows, ref).max(), rel_err(pll, _sum_entries(ref, plan)).max()
    print(f"segment ids {prec}: vs seg_ref max rel positions {e_pos:.3e}, PLL {e_hyp:.3e}")
    assert e_pos < REL and e_hyp < REL
    # the setting is one-shot: the next call has no types, and its bits are those of a scorer that
    # never had any
    after = s.score_sets(tokens, off, *plan, return_rows=True)[1].cpu().numpy()
    from asr_rescoring_amd.scorer import PLLScorer
    fresh = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=65536, precision=prec)
    try:
        never = fresh.score_sets(tokens, off, *plan, return_rows=True)[1].cpu().numpy()
    finally:
        fresh.close()
    assert np.array_equal(after, never) and (after != rows).any()


# ---- 7. arguments -----------------------------------------------------------------------------

def test_set_arguments(scorers, w_tiny):
    from asr_rescoring_amd import _lib
    from asr_rescoring_amd.scorer import PLLScorer, RescoreBertScorer
    s = scorers("fp16x3", 65536)
    tokens = np.asarray([D.CLS_ID, 200, 201, 202, D.SEP_ID, D.CLS_ID, 203, D.SEP_ID], np.int32)
    off = np.asarray([0, 5, 8], np.int32)
    good = ([0, 2, 3], [0, 2, 3, 4], [1, 3, 2, 1])
    pll, rows = s.score_sets(tokens, off, *good, return_rows=True)
    assert pll.shape == (2,) and rows.shape == (4,) and bool(torch.isfinite(rows).all())
    bad = {"descending": ([0, 2, 3], [0, 2, 3, 4], [3, 1, 2, 1]), "repeated": ([0, 2, 3], [0, 2, 3, 4], [2, 2, 2, 1]),
           "position 0": ([0, 2, 3], [0, 2, 3, 4], [0, 3, 2, 1]), "position T - 1": ([0, 2, 3], [0, 2, 3, 4], [1, 4, 2, 1]),
           "empty row": ([0, 2, 3], [0, 2, 2, 3], [1, 3, 1])}
    named = {"descending": 0, "repeated": 0, "position 0": 0, "position T - 1": 0, "empty row": 1}
    for what, plan in bad.items():
        with pytest.raises(_lib.RescoreError, match=rf"error -1: row {named[what]} \(hypothesis 0"):    # RS_EARG
            s.score_sets(tokens, off, *plan)
    with pytest.raises(_lib.RescoreError, match=r"error -1: row 2 \(hypothesis 1"):
        s.score_sets(tokens, off, [0, 2, 3], [0, 2, 3, 4], [1, 3, 2, 2])           # position T - 1 of hypothesis 1
    offsets = {"row_off[0] != 0": ([1, 2, 3], [0, 2, 3, 4], [1, 3, 2, 1]),
               "row_off descending": ([0, 3, 2], [0, 2, 3], [1, 3, 2]),
               "pos_off[0] != 0": ([0, 2, 3], [1, 2, 3, 4], [1, 3, 2, 1]),
               "pos_off descending": ([0, 2, 3], [0, 3, 2, 4], [1, 3, 2, 1])}
    for what, plan in offsets.items():
        with pytest.raises(_lib.RescoreError, match="librescore error -1"):
            s.score_sets(tokens, off, *plan)
    # a row with more positions than the per-query workspace of max_rows = 512 holds (171)
    long_tok = np.asarray([D.CLS_ID] + list(range(200, 400)) + [D.SEP_ID], np.int32)
    small = scorers("fp16x3", 512)
    with pytest.raises(_lib.RescoreError, match=r"error -1: row 1 scores 172 positions.*max_rows >= 513"):
        small.score_sets(long_tok, [0, 202], [0, 2], [0, 3, 175], list(range(1, 4)) + list(range(1, 173)))
    fits = small.score_sets(long_tok, [0, 202], [0, 2], [0, 3, 174], list(range(1, 4)) + list(range(1, 172)), return_rows=True)
    assert bool(torch.isfinite(fits[1]).all())
    # masked_logprob_multi: the same position rules over [0, T)
    ids = torch.from_numpy(tokens[None, :5].astype(np.int64))
    lab = torch.full((1, 5), -100, dtype=torch.int64)
    with pytest.raises(_lib.RescoreError, match=r"error -1: row 0 \(T = 5\)"):   # no scored position
        s.masked_logprob_multi(ids, torch.ones((1, 5), dtype=torch.int64), lab)
    # empty calls
    empty = s.score_sets(np.zeros(0, np.int32), [0], [0], [0], [], return_rows=True)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    none = s.score_sets(tokens, off, [0, 0, 0], [0], [])                          # no rows at all
    assert none.cpu().tolist() == [0.0, 0.0]
    out = s.masked_logprob_multi(torch.zeros((0, 4), dtype=torch.int64), torch.zeros((0, 4), dtype=torch.int64),
                                 torch.zeros((0, 4), dtype=torch.int64))
    assert out.shape == (0, 4)
    cs = RescoreBertScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        with pytest.raises(_lib.RescoreError, match="librescore error -3"):      # RS_ESTATE
            PLLScorer.score_sets(cs, tokens, off, *good)
    finally:
        cs.close()


# ---- 8. BERT-base -----------------------------------------------------------------------------

def test_strided_bert_base_matches_oracle():
    """H = 768 and the ten middle layers: 2 hypotheses (L = 17, 33), stride 4, fp16x3."""
    from asr_rescoring_amd.scorer import PLLScorer
    from oracle.bert_ref import TorchBert, masked_logprob_ref
    w = make_weights(BERT_BASE, seed=1234)
    tokens, off, _ = _make_set([17, 33], 13, vocab=BERT_BASE.vocab)
    plan = D.pll_strided(off, 4)
    assert np.diff(plan[0]).tolist() == [4, 4] and len(plan[2]) == 50
    ids, am, lab, q = _entry_rows(tokens, off, plan)
    ref = masked_logprob_ref(TorchBert(w, BERT_BASE), ids, am, lab, q)
    s = PLLScorer(w, BERT_BASE, device=0, max_rows=4096, precision="fp16x3")
    try:
        pll, rows = (x.cpu().numpy() for x in s.score_sets(tokens, off, *plan, return_rows=True))
    finally:
        s.close()
    e_pos, e_hyp = rel_err(rows, ref).max(), rel_err(pll, _sum_entries(ref, plan)).max()
    print(f"bert-base stride 4 fp16x3: vs oracle max rel positions {e_pos:.3e}, hypotheses {e_hyp:.3e}")
    assert e_pos < REL and e_hyp < REL


# ---- 9. CLI -----------------------------------------------------------------------------------

def test_cli_pll_stride(tmp_path):
    import yaml
    from asr_rescoring_amd import cli
    from asr_rescoring_amd.frontend import NativeTokenizer
    from asr_rescoring_amd.scorer import PLLScorer
    from test_gpu_spans import HYPS, VOCAB
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf-8")
    json.dump(HYPS, open(tmp_path / "hyps.json", "w", encoding="utf-8"), ensure_ascii=False)
    base = {"task": "scoring", "device": "cuda:0", "random_init_seed": 1234, "max_rows": 4096,
            "train_hyps_text_path": str(tmp_path / "hyps.json"),
            "model": {"bert": "bert-base-chinese", "vocab": str(tmp_path / "vocab.txt")}}

    def run(name, extra):
        out = tmp_path / name
        out.mkdir()
        cfg = tmp_path / f"{name}.yaml"
        cfg.write_text(yaml.safe_dump({**base, "output_path": str(out) + "/", **extra}, allow_unicode=True), encoding="utf-8")
        assert cli.main(["mlm_pll", "--config", str(cfg)]) == 0
        raw = open(out / "train_lm.json", "rb").read()
        lm = json.loads(raw.decode("utf-8"))
        assert {u: list(v) for u, v in lm.items()} == {u: list(v) for u, v in HYPS.items()}
        return raw, np.asarray([x for u in lm for x in lm[u].values()], np.float64)

    raw4, got4 = run("s4", {"pll_stride": 4})
    raw_plain, plain = run("plain", {})
    tok = NativeTokenizer(str(tmp_path / "vocab.txt"))
    tokens, off, _, _ = tok.encode_nbest(HYPS)
    s = PLLScorer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, max_rows=4096)
    try:
        want4 = s.score_nbest(tokens, off, variant="strided", stride=4).cpu().numpy()
        exact = s.score_nbest(tokens, off).cpu().numpy()
    finally:
        s.close()
    assert np.array_equal(got4, want4) and (want4 != exact).any()
    # without the key: the file the exact path writes, byte for byte
    assert np.array_equal(plain, exact)
    keys = [(u, h) for u in HYPS for h in HYPS[u]]
    want = {}
    for (u, h), x in zip(keys, exact):
        want.setdefault(u, {})[h] = float(x)
    cli.json_saving(str(tmp_path / "want.json"), want)
    assert open(tmp_path / "want.json", "rb").read() == raw_plain and raw4 != raw_plain
    with pytest.raises(ValueError):
        run("bad", {"pll_stride": 2, "pll_variant": "whole_word"})
    with pytest.raises(ValueError):
        run("neg", {"pll_stride": -1})
