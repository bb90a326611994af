"""GPU: the label and masking keys of ``cli mlm_finetune`` (``mlm_labels``, ``mlm_masking``,
``mlm_probability``, ``mlm_whole_word``) on the reference's train.yaml layout: do_job rows labelled at
their [MASK] only, and dynamic whole-word masking of the sentences behind them."""
import json
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

WORDS = ["ab", "cd", "abcd", "ef", "cdef", "gh"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """A WordPiece vocab with ``##`` pieces and the do_job rows of four sentences."""
    from asr_rescoring_amd.frontend import NativeTokenizer
    from asr_rescoring_amd.train import do_job_rows
    d = tmp_path_factory.mktemp("mlm_labels")
    special = {0: "[PAD]", 100: "[UNK]", 101: "[CLS]", 102: "[SEP]", 103: "[MASK]"}
    lines = [special.get(i, f"[unused{i}]") for i in range(106)] + ["ab", "cd", "ef", "gh", "##cd", "##ef"]
    (d / "vocab.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    tok = NativeTokenizer(str(d / "vocab.txt"))
    rng = np.random.default_rng(4)
    rows = []
    for u in range(4):
        text = " ".join(rng.choice(WORDS, int(rng.integers(3, 7))))
        h = [101] + list(tok.encode(text)) + [102]
        assert 100 not in h
        ids, off, lab = do_job_rows([h])
        for i in range(len(off) - 1):
            r = ids[off[i]:off[i + 1]].tolist()
            rows.append({"utt_id": str(u), "hyp_id": None, "input_ids": r, "attention_masks": [1] * len(r),
                         "mask_pos": i + 1, "labels": lab[off[i]:off[i + 1]].tolist()})
    assert any((1 - tok.word_starts(r["labels"])).any() for r in rows)        # some ## pieces
    json.dump(rows, open(d / "rows.json", "w"))
    return d


def _run(d, name, extra):
    from asr_rescoring_amd import cli
    cfg = {"task": "training", "seed": 10, "lr": 1e-5, "epoch": 2, "device": "cuda:0", "random_init_seed": 1234,
           "train_data_path": str(d / "rows.json"), "dev_data_path": str(d / "rows.json"),
           "output_path": str(d / name), "dataloader": {"shuffle": False, "batch_size": 8},
           "model": {"bert": "bert-base-chinese", "vocab": str(d / "vocab.txt")}, **extra}
    p = d / f"{name}.yaml"
    p.write_text(yaml.safe_dump(cfg), encoding="utf-8")
    return cli.mlm_finetune(cli.ArgParser().parse(["--config", str(p)]))


@pytest.mark.parametrize("name,extra", [
    ("masked", {"mlm_labels": "masked"}),
    ("dynamic", {"mlm_masking": "dynamic", "mlm_probability": 0.3, "mlm_whole_word": True})])
def test_cli_mlm_finetune_label_modes(corpus, name, extra):
    import torch
    d = corpus
    res = _run(d, name, extra)
    assert len(res["train_loss"]) == 2 and all(np.isfinite(res["train_loss"] + res["dev_loss"]))
    assert all(5.0 < v < 20.0 for v in res["train_loss"] + res["dev_loss"])   # random model: about log(vocab) = 9.96
    assert json.load(open(d / name / "loss.json")) == {"train": res["train_loss"], "dev": res["dev_loss"]}
    assert [os.path.basename(c) for c in res["checkpoints"]] == ["checkpoint_1.pth", "checkpoint_2.pth"]
    sd = torch.load(res["checkpoints"][-1], map_location="cpu", weights_only=True)
    assert torch.equal(sd["cls.predictions.decoder.weight"], sd["bert.embeddings.word_embeddings.weight"])


def test_cli_mlm_finetune_rejects_bad_label_keys(corpus):
    for extra in ({"mlm_labels": "some"}, {"mlm_masking": "static"}, {"mlm_whole_word": True},
                  {"mlm_masking": "dynamic", "mlm_labels": "masked"}, {"mlm_masking": "dynamic", "mlm_labels": "all"},
                  {"mlm_masking": "dynamic", "mlm_whole_word": True, "model": {"bert": "bert-base-chinese"}}):
        with pytest.raises(ValueError):
            _run(corpus, "bad", extra)
    # dynamic masking reads the sentences off runs of do_job rows: rows out of order are refused
    rows = json.load(open(corpus / "rows.json"))
    n0 = len(rows[0]["labels"]) - 2
    assert rows[n0]["labels"] != rows[0]["labels"]
    json.dump([rows[n0]] + rows[1:n0] + [rows[0]] + rows[n0 + 1:], open(corpus / "swapped.json", "w"))
    with pytest.raises(ValueError, match="do_job rows in order"):
        _run(corpus, "bad", {"mlm_masking": "dynamic", "train_data_path": str(corpus / "swapped.json")})
