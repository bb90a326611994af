"""GPU: nothing of one call stays on the scorer handle for the next one.

The form of a call (top-k request, segment ids, embedding output) lives in a descriptor on the entry
point's stack (csrc/rs_api.hip ``Call``); the handle keeps only the segment ids pending for the next
call.  So on one handle, after any sequence of calls — failed ones included — every call returns,
bit for bit, what the same call returns as the first call of a fresh handle.

Inputs (BERT_TINY, ``max_rows`` 512, both precision modes): six hypotheses of T = 3, 5, 17, 64, 65,
130 tokens — both attention kernel families (T <= 64 and above), and several chunks per call.
"""
import numpy as np
import pytest
import torch

from asr_rescoring_amd import _lib
from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights

pytestmark = pytest.mark.gpu

PRECS = ["fp16", "fp16x3"]
LENS = [3, 5, 17, 64, 65, 130]
MAX_ROWS = 512

_rng = np.random.default_rng(31)
HYPS = [[D.CLS_ID] + _rng.integers(D.FIRST_WORD_ID, BERT_TINY.vocab, size=T - 2).tolist() + [D.SEP_ID] for T in LENS]
TOKENS = np.concatenate([np.asarray(h, np.int32) for h in HYPS])
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
TYPES = _rng.integers(0, BERT_TINY.type_vocab, len(TOKENS)).astype(np.int32)
# one hypothesis more, longer than max_position_embeddings: fails in the run (RS_EUNSUP), past the
# argument checks and the top-k set-up
TOO_LONG = BERT_TINY.max_pos + 1
TOKENS_LONG = np.concatenate([TOKENS, np.full(TOO_LONG, D.FIRST_WORD_ID, np.int32)])
OFF_LONG = np.append(OFF, OFF[-1] + TOO_LONG).astype(np.int32)
# the same hypotheses as a padded batch with one [MASK] per row (masked_logprob / masked_topk)
MASK_POS = [1, 3, 9, 62, 33, 128]
LABELS = torch.zeros(len(LENS), max(LENS), dtype=torch.int64)
for _i, _h in enumerate(HYPS):
    LABELS[_i, :len(_h)] = torch.tensor(_h)
ATT = (torch.arange(max(LENS))[None, :] < torch.tensor(LENS)[:, None]).long()
IDS = LABELS.clone()
IDS[torch.arange(len(LENS)), torch.tensor(MASK_POS)] = BERT_TINY.mask_id
TYPES_PAD = torch.zeros_like(IDS)
TYPES_PAD[ATT.bool()] = torch.from_numpy(TYPES).long()


def _np(out):
    return [t.cpu().numpy() for t in (out if isinstance(out, tuple) else (out,))]


CALLS = {
    "score": lambda s: _np(s.score_nbest(TOKENS, OFF, return_rows=True)),
    "topk": lambda s: _np(s.topk_nbest(TOKENS, OFF, k=3, return_pll=True)),
    "score_typed": lambda s: _np(s.score_nbest(TOKENS, OFF, return_rows=True, token_types=TYPES)),
    "masked_topk": lambda s: _np(s.masked_topk(IDS, ATT, MASK_POS, k=3)),
    "masked_logprob": lambda s: _np(s.masked_logprob(IDS, ATT, LABELS, MASK_POS)),
}


def _bitwise(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8))


@pytest.fixture(scope="module")
def w_tiny():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


@pytest.mark.parametrize("prec", PRECS)
def test_scorer_calls_leave_nothing_on_the_handle(w_tiny, prec):
    from asr_rescoring_amd.scorer import PLLScorer

    def scorer():
        return PLLScorer(w_tiny, BERT_TINY, device=0, max_rows=MAX_ROWS, precision=prec)

    first = {}                      # each call as the first call of a fresh handle
    for name, call in CALLS.items():
        s = scorer()
        first[name] = call(s)
        s.close()
    assert not np.array_equal(first["score"][1], first["score_typed"][1])      # the types are read
    assert np.array_equal(first["topk"][3], first["score"][1])                 # top-k rows are score_nbest's

    s = scorer()
    try:
        _bitwise(CALLS["score"](s), first["score"])                                             # 1
        _bitwise(CALLS["topk"](s), first["topk"])                                               # 2
        with pytest.raises(_lib.RescoreError, match="error -5: sequence longer than max_position_embeddings"):
            s.topk_nbest(TOKENS_LONG, OFF_LONG, k=3, return_pll=True)                           # 3
        _bitwise(CALLS["score_typed"](s), first["score_typed"])                                 # 4
        with pytest.raises(_lib.RescoreError, match=r"error -1: rs_model_set_token_types gave \d+ token types, "
                                                    r"this call addresses \d+ tokens"):
            s.score_nbest(TOKENS, OFF, token_types=TYPES[:-1])                                  # 5
        _bitwise(CALLS["score"](s), first["score"])                                             # 6
        _bitwise(CALLS["masked_topk"](s), first["masked_topk"])                                 # 7
        _bitwise(CALLS["masked_logprob"](s), first["masked_logprob"])                           # 8
        # and the padded-batch calls with segment ids, then without
        typed = _np(s.masked_logprob(IDS, ATT, LABELS, MASK_POS, token_type_ids=TYPES_PAD))
        assert not np.array_equal(typed[0], first["masked_logprob"][0])
        _bitwise(CALLS["masked_topk"](s), first["masked_topk"])
    finally:
        s.close()


@pytest.mark.parametrize("prec", PRECS)
def test_bertscorer_recall_with_types_then_plain_embed(w_tiny, prec):
    from asr_rescoring_amd.bertscore import BertScorer
    utt_off = np.array([0, 3, 6], np.int32)

    def scorer():
        return BertScorer(w_tiny, BERT_TINY, device=0, max_rows=MAX_ROWS, precision=prec)

    def recall(s, types):
        d_type = s._set_types(types)      # noqa: F841  (alive until the call has returned)
        rmat, rmat0, _ = s.recall_matrices(TOKENS, OFF, utt_off)
        return _np((rmat, rmat0))

    s = scorer()
    emb_first = _np(s.embed(TOKENS, OFF))
    s.close()
    s = scorer()
    rec_first = recall(s, TYPES)
    s.close()

    s = scorer()
    try:
        plain = recall(s, None)
        _bitwise(recall(s, TYPES), rec_first)
        assert not np.array_equal(plain[0], rec_first[0])              # the types are read
        _bitwise(_np(s.embed(TOKENS, OFF)), emb_first)                 # and gone with the call
        _bitwise(recall(s, None), plain)
    finally:
        s.close()
