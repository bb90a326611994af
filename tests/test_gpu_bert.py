"""GPU parity: HIP BERT scorers vs the golden fixtures (reference outputs) and the oracle.

Tolerance (BASELINE.json north_star): scores within 1e-3 relative of the reference
PyTorch-CPU fp32 path, per masked row as well as per hypothesis.  The default precision
(fp16x3) splits every fp32 GEMM operand into fp16 hi/lo parts on the fp16 MFMA with fp32
accumulation (fp32-level accuracy); LayerNorm, softmax, GELU, logsumexp in fp32; PLL sums
in fp64.  The opt-in "fp16" mode (fp16 operands) is reduced precision and is tested as such.
"""
import os

import numpy as np
import pytest
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_BASE, BERT_TINY, make_weights

pytestmark = pytest.mark.gpu

REL = 1e-3


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


@pytest.fixture(scope="module")
def w_base():
    return make_weights(BERT_BASE, seed=1234, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.fixture(scope="module")
def pll_base(w_base):
    from asr_rescoring_amd.scorer import PLLScorer
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=8192)
    assert s.precision == "fp16x3"
    yield s
    s.close()


@pytest.fixture(scope="module")
def pll_base16(w_base):
    from asr_rescoring_amd.scorer import PLLScorer
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=8192, precision="fp16")
    yield s
    s.close()


@pytest.fixture(scope="module")
def pll_tiny(w_tiny):
    from asr_rescoring_amd.scorer import PLLScorer
    s = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    yield s
    s.close()


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def test_pll_base_golden(pll_base, golden_dir):
    """Default precision against the reference-run F1 fixture: every masked row's
    token_score (MLM_PLL/main.py:105) and every PLL within 1e-3 relative (measured ~1e-6)."""
    g = _load(golden_dir, "pll_base.npz")
    pll, rows = pll_base.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    rows = rows.cpu().numpy()
    pll = pll.cpu().numpy()
    assert rel_err(pll, g["pll"]).max() < REL
    assert rel_err(rows, g["row_lp"]).max() < REL
    # per-hypothesis sum of the returned rows in row order, fp64 == pll (bit-exact)
    off = np.concatenate([[0], np.cumsum(np.diff(g["hyp_off"]) - 2)])
    for h in range(len(pll)):
        acc = 0.0
        for x in rows[off[h]:off[h + 1]]:
            acc += float(x)
        assert acc == pll[h]


def test_pll_fp16_mode_golden(pll_base16, golden_dir):
    """Opt-in reduced-precision mode (fp16 operands): the per-hypothesis PLL stays within
    1e-3 relative; per-row log-probs are NOT held to 1e-3 in this mode (measured max ~1.1e-3
    on F1) — that is why fp16x3 is the default and the bench headline."""
    g = _load(golden_dir, "pll_base.npz")
    pll, rows = pll_base16.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    assert rel_err(pll.cpu().numpy(), g["pll"]).max() < REL
    assert np.percentile(rel_err(rows.cpu().numpy(), g["row_lp"]), 99) < REL


def test_pll_tiny_golden(pll_tiny, golden_dir):
    g = _load(golden_dir, "pll_tiny.npz")
    pll, rows = pll_tiny.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    assert rel_err(pll.cpu().numpy(), g["pll"]).max() < REL
    assert rel_err(rows.cpu().numpy(), g["row_lp"]).max() < REL


@pytest.mark.parametrize("x3s,lnfuse,imgres", [("1", "1", "1"), ("1", "0", "1"), ("0", "1", "1"), ("1", "1", "0")],
                         ids=["1-1", "1-0", "0-1", "1-1-imgres0"])
def test_pll_fp16x3_golden(w_base, golden_dir, monkeypatch, x3s, lnfuse, imgres):
    """Split-fp16 (x3) precision mode: fp32-level accuracy from fp16 MFMA, with the split-operand
    GEMMs (RS_X3S=1, default: two-part images, three products in registers) and with the
    K-concatenated three-part form (RS_X3S=0); split-operand layers with the residual +
    LayerNorm in the O-projection / BertOutput epilogues (RS_LNFUSE=1, default), as separate
    ln_res_img passes (RS_LNFUSE=0), and with the residual held as the fp32 pre-LN stream closed by
    ln_res32 (RS_X3S_IMGRES=0, where RS_LNFUSE has no effect: eleven ln_res32 layers)."""
    from asr_rescoring_amd.scorer import PLLScorer
    g = _load(golden_dir, "pll_base.npz")
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=4096, precision="fp16x3")
    try:
        default = s.score_nbest(g["tokens"], g["hyp_off"]).cpu().numpy() if imgres == "0" else None
        monkeypatch.setenv("RS_X3S", x3s)
        monkeypatch.setenv("RS_LNFUSE", lnfuse)
        monkeypatch.setenv("RS_X3S_IMGRES", imgres)
        pll, rows = s.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    finally:
        s.close()
    e_pll = rel_err(pll.cpu().numpy(), g["pll"]).max()
    e_rows = rel_err(rows.cpu().numpy(), g["row_lp"]).max()
    print(f"fp16x3 golden x3s={x3s} lnfuse={lnfuse} imgres={imgres}: pll {e_pll:.3e} rows {e_rows:.3e}")
    # measured 1.9e-7 (PLL) / 1.1e-6 (rows) with the lo parts scaled out of the fp16 subnormal
    # range (common.h put_split); 2e-5 / 2e-5 before, when the f16 MFMA flushed them
    # (RS_X3S_IMGRES=0: 1.2e-7 / 1.3e-6)
    assert e_pll < 1e-6
    assert e_rows < 5e-6
    if default is not None:
        assert not np.array_equal(pll.cpu().numpy(), default)     # the switch really took effect


@pytest.mark.parametrize("max_rows", [4096, 65536, 262144])
def test_lnfuse_matches_separate_pass(w_base, monkeypatch, max_rows):
    """Residual + LayerNorm in the GEMM epilogue (EPI_LNRES_IMG: each 256-column tile's row
    partials exchanged between the row panel's column tiles inside the launch) against the
    separate ln_res_img pass, on enough rows that every launch has more tiles than the chip has
    workgroups (tiles claimed as workgroups free up; up to 3072 tiles per launch at 262144 rows,
    the bench's chunk) and on many small launches: the same residual sum, statistics combined in another order —
    scores within 1e-6 relative — and bitwise reproducible from call to call."""
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(12, 50, seed=11, vocab=BERT_BASE.vocab, len_lo=4, len_hi=60)
    s = PLLScorer(w_base, BERT_BASE, device=0, max_rows=max_rows, precision="fp16x3")
    try:
        monkeypatch.setenv("RS_LNFUSE", "1")
        a = s.score(nb)
        a2 = s.score(nb)
        monkeypatch.setenv("RS_LNFUSE", "0")
        b = s.score(nb)
    finally:
        s.close()
    assert np.array_equal(a, a2)
    assert not np.array_equal(a, b)          # the two paths really differ in the statistics' order
    assert rel_err(a, b).max() < 1e-6, rel_err(a, b).max()


def test_cls_golden(w_base, w_tiny, golden_dir):
    from asr_rescoring_amd.scorer import RescoreBertScorer
    for w, shape, name, key in ((w_base, BERT_BASE, "cls_base.npz", "cls"), (w_tiny, BERT_TINY, "pll_tiny.npz", "cls")):
        g = _load(golden_dir, name)
        s = RescoreBertScorer(w, shape, device=0, max_rows=2048)
        got = s.score_nbest(g["tokens"], g["hyp_off"]).cpu().numpy()
        s.close()
        # RescoreBert outputs are O(1) scalars: 1e-3 relative or 1e-4 absolute
        err = np.abs(got - g[key])
        assert (err <= np.maximum(REL * np.abs(g[key]), 1e-4)).all(), err.max()


def test_rescorebert_module_signature(w_tiny):
    """RescoreBertHIP.forward(input_ids, attention_mask) on a padded batch == ragged scores."""
    from asr_rescoring_amd.scorer import RescoreBertHIP
    nb = D.synthetic_nbest(3, 4, seed=9, vocab=BERT_TINY.vocab, len_lo=2, len_hi=20)
    m = RescoreBertHIP(w_tiny, BERT_TINY, device=0, max_rows=2048)
    seqs = [torch.tensor(nb.tokens[nb.hyp_off[h]:nb.hyp_off[h + 1]], dtype=torch.long) for h in range(nb.n_hyp)]
    ids = torch.nn.utils.rnn.pad_sequence(seqs, batch_first=True)
    am = torch.nn.utils.rnn.pad_sequence([torch.ones_like(s) for s in seqs], batch_first=True)
    out = m(ids.cuda(), am.cuda()).cpu().numpy()
    ragged = m.engine.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
    assert np.array_equal(out, ragged)


def test_masked_logprob_batch(pll_tiny, w_tiny):
    """Row-level drop-in on a reference-style padded batch of 32 rows."""
    from oracle.bert_ref import TorchBert, masked_logprob_ref, pll_rows
    nb = D.synthetic_nbest(2, 3, seed=11, vocab=BERT_TINY.vocab, len_lo=3, len_hi=30)
    rows = list(pll_rows(nb.tokens, nb.hyp_off))[:32]
    T = max(len(r[1]) for r in rows)
    ids = np.zeros((len(rows), T), np.int64)
    am = np.zeros_like(ids)
    lab = np.zeros_like(ids)
    for i, r in enumerate(rows):
        ids[i, :len(r[1])] = r[1]
        am[i, :len(r[1])] = 1
        lab[i, :len(r[3])] = r[3]
    mp = [r[2] for r in rows]
    got = pll_tiny.masked_logprob(torch.from_numpy(ids), torch.from_numpy(am), torch.from_numpy(lab), mp)
    ref = masked_logprob_ref(TorchBert(w_tiny, BERT_TINY), ids, am, lab, np.asarray(mp))
    assert rel_err(got.cpu().numpy(), ref).max() < REL


def test_batch_invariance_and_determinism(pll_tiny):
    """Scores do not depend on chunking / batch composition; repeated runs are bitwise equal."""
    nb = D.synthetic_nbest(12, 6, seed=21, vocab=BERT_TINY.vocab, len_lo=3, len_hi=45)
    a = pll_tiny.score(nb)
    b = pll_tiny.score(nb)
    assert np.array_equal(a, b)
    sub = nb.subset([3, 7])
    c = pll_tiny.score(sub)
    idx = np.concatenate([np.arange(nb.utt_off[u], nb.utt_off[u + 1]) for u in (3, 7)])
    assert rel_err(c, a[idx]).max() < 1e-5


def test_small_chunks_match(w_tiny):
    """Forcing many launch chunks (max_rows=512) gives the same scores."""
    from asr_rescoring_amd.scorer import PLLScorer
    nb = D.synthetic_nbest(6, 5, seed=3, vocab=BERT_TINY.vocab, len_lo=3, len_hi=40)
    s1 = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=512)
    s2 = PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=65536)
    a, b = s1.score(nb), s2.score(nb)
    s1.close(), s2.close()
    assert rel_err(a, b).max() < 1e-5


def test_edge_lengths(pll_tiny, w_tiny):
    """L=1 hypotheses (T=3), long hypotheses (T > 64: multi-block attention), T = 200."""
    from oracle.bert_ref import TorchBert, pll_reference_pattern
    rng = np.random.default_rng(0)
    hyps = [[rng.integers(106, BERT_TINY.vocab, size=1).tolist(),
             rng.integers(106, BERT_TINY.vocab, size=70).tolist(),
             rng.integers(106, BERT_TINY.vocab, size=198).tolist()]]
    nb = D.from_lists(hyps, [[0.0, 0.0, 0.0]])
    got = pll_tiny.score(nb)
    _, ref = pll_reference_pattern(TorchBert(w_tiny, BERT_TINY), nb.tokens, nb.hyp_off, full_head=False)
    assert rel_err(got, ref).max() < REL


def test_max_position_length(pll_tiny, w_tiny):
    """T = max_position_embeddings (512, L = 510): every position embedding, 8 key blocks of
    online-softmax attention, the scored-row attention over 512 keys — PLL and RescoreBert vs the
    oracle; T = 513 is rejected like the reference's position-embedding lookup would fail."""
    from asr_rescoring_amd._lib import RescoreError
    from asr_rescoring_amd.scorer import RescoreBertScorer
    from oracle.bert_ref import TorchBert, cls_reference_pattern, pll_reference_pattern
    rng = np.random.default_rng(5)
    L = BERT_TINY.max_pos - 2
    nb = D.from_lists([[rng.integers(106, BERT_TINY.vocab, size=L).tolist(),
                        rng.integers(106, BERT_TINY.vocab, size=7).tolist()]], [[0.0, 0.0]])
    tb = TorchBert(w_tiny, BERT_TINY)
    got = pll_tiny.score(nb)
    _, ref = pll_reference_pattern(tb, nb.tokens, nb.hyp_off, batch_size=64, full_head=False)
    assert rel_err(got, ref).max() < REL
    cs = RescoreBertScorer(w_tiny, BERT_TINY, device=0, max_rows=2048)
    try:
        c = cs.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
        cref = cls_reference_pattern(tb, nb.tokens, nb.hyp_off)
        assert (np.abs(c - cref) <= np.maximum(REL * np.abs(cref), 1e-4)).all(), np.abs(c - cref).max()
        long_nb = D.from_lists([[rng.integers(106, BERT_TINY.vocab, size=L + 1).tolist()]], [[0.0]])
        with pytest.raises(RescoreError):
            cs.score_nbest(long_nb.tokens, long_nb.hyp_off)
    finally:
        cs.close()
    with pytest.raises(RescoreError):
        pll_tiny.score_nbest(long_nb.tokens, long_nb.hyp_off)


def test_empty_and_bad_input(pll_tiny):
    from asr_rescoring_amd._lib import RescoreError
    out = pll_tiny.score_nbest(np.zeros(0, np.int32), np.zeros(1, np.int32))
    assert out.numel() == 0
    with pytest.raises(RescoreError):
        pll_tiny.score_nbest(np.array([101, 102], np.int32), np.array([0, 2], np.int32))  # L = 0


def test_oracle_parity_base_synthetic(pll_base, w_base):
    """BERT-base, synthetic N-best at L~U{24..40}: HIP vs oracle (masked-row head)."""
    from oracle.bert_ref import TorchBert, pll_reference_pattern
    nb = D.synthetic_nbest(1, 3, seed=1)
    got = pll_base.score(nb)
    _, ref = pll_reference_pattern(TorchBert(w_base, BERT_BASE), nb.tokens, nb.hyp_off, batch_size=64,
                                   full_head=False)
    assert rel_err(got, ref).max() < REL


@pytest.mark.parametrize("prec", ["fp16", "fp16x3"])
@pytest.mark.parametrize("max_rows", [512, 65536])
def test_layer0_dedup_is_exact(w_tiny, w_base, max_rows, prec, monkeypatch):
    """Layer-0 Q/K/V over unique rows (RS_DEDUP=1, default) vs over every masked copy
    (RS_DEDUP=0): the same rows go through the same GEMM, so scores are bitwise equal.
    max_rows=512 splits hypotheses across chunks (a hypothesis' rows re-planned per chunk)."""
    from asr_rescoring_amd.scorer import PLLScorer
    for w, cfg, seed in ((w_tiny, BERT_TINY, 5), (w_base, BERT_BASE, 6)):
        nb = D.synthetic_nbest(5, 4, seed=seed, vocab=cfg.vocab, len_lo=1, len_hi=70)
        s = PLLScorer(w, cfg, device=0, max_rows=max_rows, precision=prec)
        try:
            monkeypatch.setenv("RS_DEDUP", "1")
            a = s.score(nb)
            monkeypatch.setenv("RS_DEDUP", "0")
            b = s.score(nb)
        finally:
            s.close()
        assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.parametrize("prec", ["fp16", "fp16x3"])
@pytest.mark.parametrize("max_rows", [512, 65536])
def test_lastq_full_layer_is_exact(w_tiny, w_base, max_rows, prec, monkeypatch):
    """Query-row-only last layer (default) vs the full Q/K/V GEMM at the last layer (RS_LASTQ=0):
    the scored row's Q goes through the same GEMM on the same operand row either way, so scores
    are bitwise equal.  BERT_TINY: layer 0 full, layer 1 the query layer;
    max_rows=512 gives several chunks whose sequence count is no multiple of the row alignment."""
    from asr_rescoring_amd.scorer import PLLScorer
    for w, cfg, seed in ((w_tiny, BERT_TINY, 5), (w_base, BERT_BASE, 6)):
        nb = D.synthetic_nbest(5, 4, seed=seed, vocab=cfg.vocab, len_lo=1, len_hi=70)
        s = PLLScorer(w, cfg, device=0, max_rows=max_rows, precision=prec)
        try:
            monkeypatch.delenv("RS_LASTQ", raising=False)
            a = s.score(nb)
            monkeypatch.setenv("RS_LASTQ", "0")
            b = s.score(nb)
        finally:
            s.close()
        print(f"lastq {cfg.layers} layers {prec} max_rows={max_rows}: max rel diff {rel_err(b, a).max():.3e}")
        assert np.array_equal(a, b), np.abs(a - b).max()


@pytest.mark.parametrize("env,same", [({"RS_OPROJ": "resln"}, False), ({"RS_FFN2": "f16"}, True),
                                      ({"RS_LNRES_DEFER": "0"}, False), ({"RS_LNRES_DEFER": "1"}, False)])
def test_residual_paths_golden(pll_base16, golden_dir, env, same, monkeypatch):
    """The residual-block variants against the F1 fixture: O projection with the residual +
    LayerNorm rebuilt in the GEMM accumulators (RS_OPROJ=resln; default: fp16-output GEMM +
    ln_res_rows), FFN2 split the same way as the O projection (RS_FFN2=f16), and the
    post-attention stream written back (RS_LNRES_DEFER=0) or rebuilt in the BertOutput GEMM's
    accumulators (=1) instead of the default single two-block ln_res_rows pass (=2)."""
    g = _load(golden_dir, "pll_base.npz")
    base = pll_base16.score_nbest(g["tokens"], g["hyp_off"]).cpu().numpy()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pll, rows = pll_base16.score_nbest(g["tokens"], g["hyp_off"], return_rows=True)
    pll = pll.cpu().numpy()
    assert rel_err(pll, g["pll"]).max() < REL
    e = rel_err(rows.cpu().numpy(), g["row_lp"])
    assert np.percentile(e, 99) < REL
    if same:
        # RS_FFN2=f16 stores the post-attention stream x in fp32 and forms LN(x) + o2 in a
        # second pass; the default forms the same expression from (x32, o1) in one pass:
        # bit-identical by construction
        assert np.array_equal(pll, base)
    else:
        assert not np.array_equal(pll, base)      # the variant really ran a different path


@pytest.mark.parametrize("precision", ["fp16x3", "fp16"])
def test_fp16_range_guard(w_tiny, precision):
    """The operand images hold |x| <= 65504 (fp16); the fp32 reference has no such limit.
    A weight beyond it is refused at finalize; an activation beyond it (the embedding
    LayerNorm's gamma scaled until its output, the first GEMM operand, crosses 65504) makes
    the scoring call fail with RS_EUNSUP instead of returning inf / NaN scores.  Just inside
    the range the same path scores finite."""
    from asr_rescoring_amd._lib import RescoreError
    from asr_rescoring_amd.scorer import PLLScorer, RescoreBertScorer
    nb = D.synthetic_nbest(2, 3, seed=5, vocab=BERT_TINY.vocab, len_lo=3, len_hi=12)
    w = dict(w_tiny)
    k = "bert.encoder.layer.0.intermediate.dense.weight"
    w[k] = w[k].copy()
    w[k][0, 0] = 1e5
    with pytest.raises(RescoreError, match="fp16 range"):
        PLLScorer(w, BERT_TINY, device=0, max_rows=2048, precision=precision)
    g = "bert.embeddings.LayerNorm.weight"
    for scale, ok in ((30.0, True), (1e6, False)):
        w = dict(w_tiny)
        w[g] = w_tiny[g] * scale
        for cls in (PLLScorer, RescoreBertScorer):
            s = cls(w, BERT_TINY, device=0, max_rows=2048, precision=precision)
            try:
                if ok:
                    out = s.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
                    assert np.isfinite(out).all()
                else:
                    with pytest.raises(RescoreError, match="non-finite"):
                        s.score_nbest(nb.tokens, nb.hyp_off)
            finally:
                s.close()


def test_x3s_weight_range_falls_back_to_k_concatenated(w_tiny, monkeypatch):
    """A projection weight in [1023.75, 65504] fits the fp16 images but not the split-operand K
    loop's 64 W_hi (it became inf, and the call failed with a misleading range error).
    rs_model_finalize then packs no split-operand weights and the model runs every fp16x3 layer in
    the K-concatenated form: finite scores, bitwise equal to RS_X3S=0, within the north_star
    tolerance of the fp32 oracle."""
    from asr_rescoring_amd.scorer import PLLScorer
    from oracle.bert_ref import TorchBert, pll_reference_pattern
    nb = D.synthetic_nbest(2, 3, seed=5, vocab=BERT_TINY.vocab, len_lo=3, len_hi=12)
    w = dict(w_tiny)
    k = "bert.encoder.layer.1.intermediate.dense.weight"
    w[k] = w[k].copy()
    w[k][5, 7] = 2000.0
    s = PLLScorer(w, BERT_TINY, device=0, max_rows=2048, precision="fp16x3")
    try:
        a = s.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
        monkeypatch.setenv("RS_X3S", "0")
        b = s.score_nbest(nb.tokens, nb.hyp_off).cpu().numpy()
    finally:
        s.close()
    assert np.isfinite(a).all()
    assert np.array_equal(a, b)
    _, ref = pll_reference_pattern(TorchBert(w, BERT_TINY), nb.tokens, nb.hyp_off, full_head=False)
    assert rel_err(a, ref).max() < 1e-3
