"""CPU: the float64 segment-id reference (tests/seg_ref.py) against the fp32 oracle at all-zero
types, and against transformers (float64) under random 0/1 types, forward and the type-table gradient.

Bounds: 1e-6 relative on row log-probs against the fp32 oracle (its own rounding: ~1e-7 measured
between transformers float64 and the oracle); 1e-10 between the two float64 implementations (the
same expressions; different summation orders leave ~1e-13)."""
import numpy as np
import pytest
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_TINY, make_weights

import seg_ref


def _set(seed, lens=(1, 2, 7, 12)):
    rng = np.random.default_rng(seed)
    toks, off = [], [0]
    for L in lens:
        toks += [D.CLS_ID] + rng.integers(D.FIRST_WORD_ID, BERT_TINY.vocab, size=L).tolist() + [D.SEP_ID]
        off.append(len(toks))
    toks, off = np.asarray(toks, np.int32), np.asarray(off, np.int32)
    return toks, off, rng.integers(0, 2, len(toks)).astype(np.int64)


@pytest.fixture(scope="module")
def w():
    return make_weights(BERT_TINY, seed=7, with_cls_linear=True, with_pooler=True)


def test_zero_types_equal_the_fp32_oracle(w):
    from oracle.bert_ref import TorchBert, cls_reference_pattern, pll_reference_pattern
    toks, off, _ = _set(1)
    zeros = np.zeros(len(toks), np.int64)
    spans = D.pll_spans(off, None, "original")
    m = seg_ref.SegBert(w, BERT_TINY)
    rows = seg_ref.row_logprobs(seg_ref.span_rows(m, toks, off, zeros, *spans), toks, off, spans[0], spans[3])
    ref_rows, ref_pll = pll_reference_pattern(TorchBert(w, BERT_TINY), toks, off, full_head=False)
    err = np.abs(rows - ref_rows) / np.abs(ref_rows)
    print(f"rows vs fp32 oracle: max rel {err.max():.3e}")
    assert err.max() < 1e-6
    assert (np.abs(seg_ref.sum_rows(rows, spans[0]) - ref_pll) / np.abs(ref_pll)).max() < 1e-6
    cls = seg_ref.cls_scores(m, toks, off, zeros)
    ref_cls = cls_reference_pattern(TorchBert(w, BERT_TINY), toks, off)
    assert np.abs(cls - ref_cls).max() < 1e-6 * max(1.0, np.abs(ref_cls).max())


def _hf(w, cls):
    transformers = pytest.importorskip("transformers")
    S = BERT_TINY
    cfg = transformers.BertConfig(vocab_size=S.vocab, hidden_size=S.hidden, num_hidden_layers=S.layers,
                                  num_attention_heads=S.heads, intermediate_size=S.intermediate,
                                  max_position_embeddings=S.max_pos, type_vocab_size=S.type_vocab,
                                  layer_norm_eps=S.ln_eps, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                  pad_token_id=S.pad_id)
    cfg._attn_implementation = "eager"
    model = getattr(transformers, cls)(cfg)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items() if not k.startswith("linear.")}
    if cls == "BertModel":
        sd = {k[len("bert."):]: v for k, v in sd.items() if k.startswith("bert.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not [k for k in missing if "position_ids" not in k], missing
    return model.double().eval()


def test_random_types_equal_transformers(w):
    toks, off, types = _set(2)
    m = seg_ref.SegBert(w, BERT_TINY)
    seqs, tys = seg_ref._split(toks, off), seg_ref._split(types, off)
    ids, am, tt = seg_ref._batch(seqs, tys)
    mlm = _hf(w, "BertForMaskedLM")
    with torch.no_grad():
        want = mlm(input_ids=ids, attention_mask=am, token_type_ids=tt).logits.log_softmax(-1)
        got = m.mlm_logits(m.encoder(ids, am, tt)).log_softmax(-1)
        keep = am.bool()
        err = ((got - want).abs() / want.abs())[keep].max().item()
        print(f"MLM log-softmax vs transformers float64: max rel {err:.3e}")
        assert err < 1e-10
        # the types matter on both sides
        zero = m.mlm_logits(m.encoder(ids, am, torch.zeros_like(tt))).log_softmax(-1)
        assert ((zero - got).abs() / got.abs())[keep].max().item() > 1e-3
        bert = _hf(w, "BertModel")
        hid = bert(input_ids=ids, attention_mask=am, token_type_ids=tt).last_hidden_state
        mine = m.encoder(ids, am, tt)
        assert ((mine - hid).abs()[keep].max() / hid.abs().max()).item() < 1e-10
        cls = seg_ref.cls_scores(m, toks, off, types)
        want_cls = torch.nn.functional.linear(hid[:, 0], m.w["linear.weight"], m.w["linear.bias"]).squeeze(-1).numpy()
        assert np.abs(cls - want_cls).max() < 1e-10 * max(1.0, np.abs(want_cls).max())


def test_type_table_gradient_equals_transformers(w):
    toks, off, types = _set(3)
    labels = toks.astype(np.int64)
    key = "bert.embeddings.token_type_embeddings.weight"
    loss, g = seg_ref.mlm_step(w, BERT_TINY, toks, off, types, labels, [key, "bert.embeddings.LayerNorm.weight"])
    mlm = _hf(w, "BertForMaskedLM")
    ids, am, tt = seg_ref._batch(seg_ref._split(toks, off), seg_ref._split(types, off))
    logits = mlm(input_ids=ids, attention_mask=am, token_type_ids=tt).logits
    keep = am.bool()
    want = torch.nn.functional.cross_entropy(logits[keep], seg_ref.pad(seg_ref._split(labels, off))[keep])
    want.backward()
    assert abs(loss - float(want.detach())) < 1e-10 * abs(float(want.detach()))
    for k, hf_k in ((key, "bert.embeddings.token_type_embeddings.weight"),
                    ("bert.embeddings.LayerNorm.weight", "bert.embeddings.LayerNorm.weight")):
        rg = dict(mlm.named_parameters())[hf_k].grad.numpy()
        err = np.abs(g[k] - rg).max() / np.abs(rg).max()
        print(f"{k}: gradient vs transformers max rel-to-max {err:.3e}")
        assert err < 1e-10
    assert np.abs(g[key][0]).max() > 0 and np.abs(g[key][1]).max() > 0
