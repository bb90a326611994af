"""The pure-Python side of the trainer options (no GPU): the prefix rule that ``freeze`` / ``unfreeze``
and ``rs_trainer_set_trainable`` select tensors by, and the learning-rate schedule."""
import pytest

from asr_rescoring_amd.train import lr_at, param_shapes, prefix_matches
from asr_rescoring_amd.weights import BERT_BASE


def _sel(head, prefix):
    return [k for k in param_shapes(BERT_BASE, head) if prefix_matches(k, prefix)]


@pytest.mark.parametrize("head", ["cls", "mlm"])
def test_prefix_selects_whole_dotted_components(head):
    keys = list(param_shapes(BERT_BASE, head))
    one = _sel(head, "bert.encoder.layer.1")
    assert len(one) == 16 and all(k.startswith("bert.encoder.layer.1.") for k in one)
    assert not any(k.startswith(("bert.encoder.layer.10.", "bert.encoder.layer.11.")) for k in one)
    assert _sel(head, "bert.encoder.layer.1.") == one                      # a trailing dot is ignored
    assert len(_sel(head, "bert.encoder.layer.10")) == 16
    body = _sel(head, "bert")
    assert body == [k for k in keys if k.startswith("bert.")]
    rest = [k for k in keys if k not in body]
    if head == "cls":
        assert rest == ["linear.weight", "linear.bias"] == _sel(head, "linear") == _sel(head, "linear.")
        assert _sel(head, "cls") == []
    else:
        assert rest == _sel(head, "cls") == _sel(head, "cls.predictions") and len(rest) == 5
        assert _sel(head, "linear") == []
    # a whole key selects itself; partial components, unknown names and the empty prefix select nothing
    assert _sel(head, "bert.embeddings.LayerNorm.weight") == ["bert.embeddings.LayerNorm.weight"]
    for bad in ("bert.encoder.lay", "ber", "bert.embeddings.word", "encoder", "nothing.here", "", "."):
        assert _sel(head, bad) == [], bad
    # the aliases of the tied decoder follow the same rule
    assert prefix_matches("cls.predictions.decoder.weight", "cls")
    assert not prefix_matches("cls.predictions.decoder.weight", "cls.predictions.dec")


def test_linear_schedule_values():
    total, warm, lr = 100, 10, 2e-5
    at = lambda s: lr_at(s, total, warm, lr, "linear")
    assert at(0) == 0.0
    assert at(warm - 1) == lr * ((warm - 1) / warm)
    assert at(warm) == lr
    assert at(total - 1) == lr * (1 / (total - warm))
    assert at(total) == 0.0 and at(total + 5) == 0.0
    up = [at(s) for s in range(warm + 1)]
    down = [at(s) for s in range(warm, total + 1)]
    assert all(a < b for a, b in zip(up, up[1:]))
    assert all(a > b for a, b in zip(down, down[1:]))


def test_constant_schedule_and_degenerate_lengths():
    assert all(lr_at(s, 50, 7, 3e-4, "constant") == 3e-4 for s in (0, 6, 7, 49, 50, 1000))
    assert lr_at(0, 50, 7, 3e-4) == 3e-4                                   # the default schedule
    # warmup = 0: starts at the full rate; total = warmup: nothing left to decay over
    assert lr_at(0, 10, 0, 1.0, "linear") == 1.0 and lr_at(5, 10, 0, 1.0, "linear") == 0.5
    assert lr_at(3, 4, 4, 1.0, "linear") == 0.75 and lr_at(4, 4, 4, 1.0, "linear") == 0.0
    assert lr_at(0, 0, 0, 1.0, "linear") == 0.0
    with pytest.raises(ValueError):
        lr_at(0, 10, 1, 1.0, "cosine")
