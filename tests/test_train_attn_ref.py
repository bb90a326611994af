"""CPU: tests/train_attn_ref.py — the explicit forward / backward expressions of the trainer's
attention in float64 against torch float64 autograd of softmax(Q K^T / 8 + mask) V, with key
lengths and a fed dropout mask, on the input families tests/test_gpu_train_attn.py uses; and the
properties those families promise (score ranges, where the planted maxima fall)."""
import numpy as np
import pytest
import torch

import train_attn_ref as R

HEADS = 4
CASES = [  # (T, klen)
    (1, None), (2, 1), (3, None), (64, 63), (65, None), (130, 129), (200, 65), (300, 129), (257, None),
]


def _mult(T, seed, p=0.1):
    g = torch.Generator().manual_seed(seed)
    keep = (torch.rand(HEADS, T, T, generator=g) >= p).float()
    return keep * np.float32(1.0 / (1.0 - p))


@pytest.mark.parametrize("family", ["normal", "peaked"])
@pytest.mark.parametrize("drop", [False, True])
def test_reference_matches_float64_autograd(family, drop):
    lens = [t for t, _ in CASES]
    klens = [t if k is None else k for t, k in CASES]
    qkv, dctx = R.make_inputs(lens, HEADS, family, 3, klens)
    r0 = 0
    for i, (t, k) in enumerate(CASES):
        m = _mult(t, 10 + i) if drop else None
        ctx, dqkv = R.attn_seq(qkv[r0:r0 + t], dctx[r0:r0 + t], HEADS, k, m)
        actx, adqkv = R.autograd_seq(qkv[r0:r0 + t], dctx[r0:r0 + t], HEADS, k, m)
        assert (ctx - actx).abs().max().item() <= 1e-12 * max(1.0, actx.abs().max().item()), (t, k)
        assert (dqkv - adqkv).abs().max().item() <= 1e-12 * max(1.0, adqkv.abs().max().item()), (t, k)
        if k is not None:           # a padding key takes no gradient
            H = HEADS * 64
            assert (dqkv[k:, H:] == 0).all()
        r0 += t


def test_batch_is_the_sequences_back_to_back():
    lens, klens = [3, 70, 1], [2, 70, 1]
    qkv, dctx = R.make_inputs(lens, HEADS, "normal", 4)
    ctx, dqkv = R.attn_batch(qkv, dctx, lens, HEADS, klens)
    c1, d1 = R.attn_seq(qkv[3:73], dctx[3:73], HEADS, 70)
    assert torch.equal(ctx[3:73], c1) and torch.equal(dqkv[3:73], d1)
    assert ctx.shape == (74, HEADS * 64) and dqkv.shape == (74, 3 * HEADS * 64)


def test_input_families():
    """normal: score spread 1-3; peaked: |score| up to about 30 and each planted row's maximum at
    its planted key (first key tile, last key tile, last unmasked key)."""
    H = HEADS * 64
    for T, k in [(300, None), (300, 129), (512, None)]:
        tk = T if k is None else k
        for family in ("normal", "peaked"):
            qkv, _ = R.make_inputs([T], HEADS, family, 5, [tk])
            q, kk = R.split_heads(qkv[:, :H].double(), HEADS), R.split_heads(qkv[:, H:2 * H].double(), HEADS)
            s = (q @ kk.transpose(1, 2) * 0.125)[:, :, :tk]
            if family == "normal":
                assert 1.0 <= s.std().item() <= 3.0
            else:
                assert 20.0 <= s.abs().max().item() <= 45.0
                pl = R.planted(T, k)
                assert pl[0][1] < R.TILE and pl[1][1] // R.TILE == (tk - 1) // R.TILE and pl[2][1] == tk - 1
                for row, key in pl:
                    assert (s[:, row].argmax(dim=-1) == key).all(), (T, k, row, key)


def test_keep_to_mults_layout():
    lens = [2, 3]
    n = HEADS * (4 + 9)
    keep = (np.arange(n) % 3 != 0).astype(np.uint8)
    m = R.keep_to_mults(keep, lens, HEADS, 0.1)
    assert m[0].shape == (HEADS, 2, 2) and m[1].shape == (HEADS, 3, 3)
    e = HEADS * 4 + 2 * 9 + 1 * 3 + 2          # sequence 1, head 2, query 1, key 2
    assert m[1][2, 1, 2].item() == pytest.approx(float(keep[e]) / 0.9, rel=1e-6)
