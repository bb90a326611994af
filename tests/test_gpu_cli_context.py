"""GPU: the CLI key ``{split}_context_text_path`` — ``mlm_pll`` and ``rescorebert`` on a 3-utterance
text fixture equal the direct ``data.with_context`` + scorer call, and differ from the run without
the key."""
import json

import numpy as np
import pytest

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BERT_BASE, make_weights

pytestmark = pytest.mark.gpu

VOCAB = (["[PAD]"] + [f"[unused{i}]" for i in range(1, 100)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]", "[unused104]", "[unused105]"]
         + list("你好嗎今天氣很") + ["hello", "##llo", "he", "##l", "world", "##s", "play", "##ing", "un", "##able"])
HYPS = {"utt_1": {"hyp_1": "你好 hello worlds", "hyp_2": "你好 hell world"},
        "utt_2": {"hyp_1": "今天 unable playing", "hyp_2": "今天 playing"},
        "utt_3": {"hyp_1": "天氣很好", "hyp_2": "天氣 hello"}}
CONTEXT = {"utt_1": "今天 playing", "utt_3": "你好嗎"}        # utt_2: no context


def _fixture(tmp_path):
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n", encoding="utf-8")
    json.dump(HYPS, open(tmp_path / "hyps.json", "w", encoding="utf-8"), ensure_ascii=False)
    json.dump(CONTEXT, open(tmp_path / "context.json", "w", encoding="utf-8"), ensure_ascii=False)
    json.dump({u: {h: 0 for h in v} for u, v in HYPS.items()}, open(tmp_path / "format.json", "w", encoding="utf-8"))


def _run(tmp_path, command, name, cfg, out_file):
    import yaml
    from asr_rescoring_amd import cli
    out = tmp_path / name
    out.mkdir()
    path = tmp_path / f"{name}.yaml"
    base = {"device": "cuda:0", "random_init_seed": 1234, "max_rows": 4096, "output_path": str(out) + "/",
            "model": {"bert": "bert-base-chinese", "vocab": str(tmp_path / "vocab.txt")}}
    path.write_text(yaml.safe_dump({**base, **cfg}, allow_unicode=True), encoding="utf-8")
    assert cli.main([command, "--config", str(path)]) == 0
    lm = json.load(open(out / out_file, encoding="utf-8"))
    assert {u: list(v) for u, v in lm.items()} == {u: list(v) for u, v in HYPS.items()}       # the JSON shape stays
    return np.asarray([x for u in lm for x in lm[u].values()], np.float64)


def _pairs(tmp_path, word_start: bool):
    from asr_rescoring_amd import cli
    from asr_rescoring_amd.frontend import NativeTokenizer
    tok = NativeTokenizer(str(tmp_path / "vocab.txt"))
    nb, _ = cli._nbest_tokens(HYPS, tok)
    seqs = [tok.encode_words(CONTEXT[u]) if u in CONTEXT else [] for u in HYPS]
    ctx = np.asarray([x for s in seqs for x in s], np.int32)
    coff = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    assert len(seqs[0]) == 4 and len(seqs[1]) == 0 and len(seqs[2]) == 3
    ws = tok.word_starts(nb.tokens) if word_start else None
    return D.with_context(nb.tokens, nb.hyp_off, nb.utt_off, ctx, coff, 512, ws, tok.word_starts(ctx) if word_start else None)


def test_cli_mlm_pll_context(tmp_path):
    from asr_rescoring_amd.scorer import PLLScorer
    _fixture(tmp_path)
    cfg = {"task": "scoring", "train_hyps_text_path": str(tmp_path / "hyps.json"), "pll_variant": "word_l2r"}
    got = _run(tmp_path, "mlm_pll", "ctx", {**cfg, "train_context_text_path": str(tmp_path / "context.json")},
               "train_lm.json")
    plain = _run(tmp_path, "mlm_pll", "plain", cfg, "train_lm.json")
    tokens, off, types, score_from, ws = _pairs(tmp_path, True)
    assert types.any() and score_from.tolist() == [6, 6, 1, 1, 5, 5] and (ws == 0).sum() >= 4
    s = PLLScorer(make_weights(BERT_BASE, seed=1234), BERT_BASE, device=0, max_rows=4096)
    try:
        want = s.score_nbest(tokens, off, variant="word_l2r", word_start=ws, token_types=types,
                             score_from=score_from).cpu().numpy()
    finally:
        s.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got[2:4], plain[2:4])                # utt_2 has no context: today's scores
    assert (got[[0, 1, 4, 5]] != plain[[0, 1, 4, 5]]).all()
    json.dump([], open(tmp_path / "rows.json", "w"))
    with pytest.raises(ValueError, match="needs train_hyps_text_path"):
        _run(tmp_path, "mlm_pll", "rows", {"task": "scoring", "train_data_path": str(tmp_path / "rows.json"),
                                           "train_context_text_path": str(tmp_path / "context.json")}, "train_lm.json")


def test_cli_rescorebert_context(tmp_path):
    from asr_rescoring_amd.scorer import RescoreBertScorer
    _fixture(tmp_path)
    cfg = {"dev_feature": ["hyps_token_ids"], "dev_feature_path": [str(tmp_path / "hyps.json")],
           "dev_output_format": str(tmp_path / "format.json"), "n_best": 10}
    got = _run(tmp_path, "rescorebert", "ctx", {**cfg, "dev_context_text_path": str(tmp_path / "context.json")},
               "dev_lm.json")
    plain = _run(tmp_path, "rescorebert", "plain", cfg, "dev_lm.json")
    tokens, off, types, _, _ = _pairs(tmp_path, False)
    s = RescoreBertScorer(make_weights(BERT_BASE, seed=1234, with_cls_linear=True, with_pooler=True), BERT_BASE,
                          device=0, max_rows=4096)
    try:
        want = s.score_nbest(tokens, off, token_types=types).cpu().numpy().astype(np.float64)
    finally:
        s.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got[2:4], plain[2:4]) and (got[[0, 1, 4, 5]] != plain[[0, 1, 4, 5]]).all()
