"""GPU: the trainer's attention kernels (k_train.hip) through rs_debug_train_attn — form 0 the
whole-head kernels (T <= 128), form 1 the tiled kernels (64-query x 64-key tiles on the f32-input
MFMA, any T) — forward then backward, against the float64 reference of tests/train_attn_ref.py.

Bound (the rule of tests/test_gpu_attention.py): for each of ctx, dQ, dK, dV,
max |out - ref64| <= 4 e32, e32 = the error of the same expressions in torch fp32 on the same
inputs, both maxima over the batch.

Lengths: 129, 160, 191, 192, 193, 255, 256, 257, 384, 511, 512 and, around the multiples of the
64-token query / key tile that list misses, 63, 64, 65, 127, 128, 319, 320, 321, 383, 385, 447,
448, 449 — one ragged launch with T = 1, 2, 3 mixed in.  Key lengths: null, 1, T - 1, 129 at
T = 300, and 63 / 64 / 65, 128 / 129, 256 either side of a key-tile edge.

Measured err / e32 on MI355X (ctx, dQ, dK, dV):
  form 1 ragged      normal 0.78 1.70 0.67 1.17   peaked 0.87 1.35 1.57 1.10
  form 1 klen        normal 0.87 1.14 1.27 1.51   peaked 1.15 0.72 0.70 1.51
  form 0 small       normal 1.21 1.09 1.28 0.95   peaked 1.00 1.28 1.63 0.95
  form 1 small       normal 1.44 0.91 1.01 1.05   peaked 0.99 1.50 1.15 1.48
  form 0 small-klen  normal 1.11 1.10 1.00 1.00   peaked 0.99 0.99 0.97 1.00
  form 1 small-klen  normal 1.21 0.92 0.85 0.87   peaked 0.88 1.04 1.03 0.87
  form 1 dropout     normal 1.08 0.81 0.78 1.32   peaked 1.42 0.65 1.05 1.18
(err 1.2e-6 .. 4.0e-5; e32 1.3e-6 .. 2.9e-5.)
"""
import functools

import numpy as np
import pytest
import torch

import train_attn_ref as R
from asr_rescoring_amd import _lib

pytestmark = pytest.mark.gpu

HEADS, H = 4, 256
RS_EUNSUP = -5

LONG = [129, 160, 191, 192, 193, 255, 256, 257, 384, 511, 512, 319, 320, 321, 383, 385, 447, 448, 449]
SHORT = [1, 2, 3, 63, 64, 65, 127, 128]
# (T, klen): 1, T - 1, 129 at T = 300, either side of the key-tile edges 64, 128, 256
KLEN = [(300, 129), (300, 1), (300, 299), (200, 63), (200, 64), (200, 65), (130, 128), (130, 129), (257, 256),
        (257, 1), (100, 1), (64, 63), (3, 1), (3, 2), (128, 127), (1, 1), (385, 384), (385, 129)]
SMALL = [1, 2, 3, 17, 63, 64, 65, 100, 127, 128]
SMALL_K = [(128, 127), (128, 1), (65, 64), (100, 63), (3, 2), (64, 64), (2, 1), (127, 65)]


def _layout(name):
    """-> (lens, klens or None)"""
    if name == "ragged":
        lens = LONG + SHORT
        np.random.default_rng(1).shuffle(lens)
        return list(lens), None
    if name == "klen":
        return [t for t, _ in KLEN], [k for _, k in KLEN]
    if name == "small":
        return list(SMALL), None
    if name == "small-klen":
        return [t for t, _ in SMALL_K], [k for _, k in SMALL_K]
    if name == "drop":
        return [300, 150, 129, 64, 3, 1, 257], [300, 150, 100, 64, 2, 1, 257]
    raise KeyError(name)


def _keep(lens, seed, step, site, p):
    from asr_rescoring_amd.train import dropout_keep
    return dropout_keep(seed, step, site, p, HEADS * sum(t * t for t in lens))


DROP = dict(seed=77, step=5, site=4, p=0.1)


@functools.lru_cache(maxsize=None)
def _case(name, family):
    """Inputs and the float64 / float32 references of a (layout, family), computed once."""
    lens, klens = _layout(name)
    qkv, dctx = R.make_inputs(lens, HEADS, family, 11 + len(name), klens)
    mults = R.keep_to_mults(_keep(lens, **DROP), lens, HEADS, DROP["p"]) if name == "drop" else None
    ref = R.attn_batch(qkv, dctx, lens, HEADS, klens, mults, torch.float64)
    r32 = R.attn_batch(qkv, dctx, lens, HEADS, klens, mults, torch.float32)
    return lens, klens, qkv, dctx, ref, r32


def _run(form, qkv, dctx, lens, klens, drop=None):
    dev = torch.device("cuda", 0)
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
    kl = None if klens is None else torch.tensor(klens, dtype=torch.int32, device=dev)
    q, g = qkv.to(dev), dctx.to(dev)
    ctx = torch.full((q.shape[0], H), float("nan"), device=dev)
    dqkv = torch.full((q.shape[0], 3 * H), float("nan"), device=dev)
    d = drop or dict(seed=0, step=0, site=0, p=0.0)
    rc = _lib.load().rs_debug_train_attn(form, q.data_ptr(), off.data_ptr(), None if kl is None else kl.data_ptr(),
                                         len(lens), H, HEADS, g.data_ptr(), d["seed"], d["step"], d["site"], d["p"],
                                         ctx.data_ptr(), dqkv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, ctx.cpu(), dqkv.cpu()


def _check(tag, ctx, dqkv, ref, r32):
    assert torch.isfinite(ctx).all() and torch.isfinite(dqkv).all(), tag
    parts = [("ctx", ctx, ref[0], r32[0])] + [
        (n, dqkv[:, i * H:(i + 1) * H], ref[1][:, i * H:(i + 1) * H], r32[1][:, i * H:(i + 1) * H])
        for i, n in enumerate(("dQ", "dK", "dV"))]
    fig = []
    for n, got, want, w32 in parts:
        err = (got.double() - want).abs().max().item()
        e32 = (w32.double() - want).abs().max().item()
        fig.append((n, err, e32))
    print(f"TRAIN-ATTN {tag}: " + "  ".join(f"{n} err {e:.2e} e32 {b:.2e} ratio {e / b:.2f}" for n, e, b in fig))
    for n, err, e32 in fig:
        assert err <= 4 * e32, (tag, n, err, e32)


def _padding_zero(dqkv, lens, klens):
    """dK and dV rows of the keys j >= klen: bitwise 0.0f"""
    r0 = 0
    for t, k in zip(lens, klens):
        pad = dqkv[r0 + k:r0 + t, H:].contiguous()
        assert (pad.view(torch.int32) == 0).all(), (t, k)
        r0 += t


@pytest.mark.parametrize("family", ["normal", "peaked"])
@pytest.mark.parametrize("name", ["ragged", "klen"])
def test_tiled_kernels_vs_float64(name, family):
    lens, klens, qkv, dctx, ref, r32 = _case(name, family)
    rc, ctx, dqkv = _run(1, qkv, dctx, lens, klens)
    assert rc == 0
    _check(f"form1-{name}-{family}", ctx, dqkv, ref, r32)
    if klens is not None:
        _padding_zero(dqkv, lens, klens)


@pytest.mark.parametrize("family", ["normal", "peaked"])
@pytest.mark.parametrize("name", ["small", "small-klen"])
def test_both_forms_up_to_128_tokens(name, family):
    """T <= 128: the whole-head kernels and the tiled kernels on the same inputs, each within the
    bound (they sum in different orders and need not be equal)."""
    lens, klens, qkv, dctx, ref, r32 = _case(name, family)
    for form in (0, 1):
        rc, ctx, dqkv = _run(form, qkv, dctx, lens, klens)
        assert rc == 0
        _check(f"form{form}-{name}-{family}", ctx, dqkv, ref, r32)
        if klens is not None:
            _padding_zero(dqkv, lens, klens)


def test_form0_refuses_more_than_128_tokens():
    lens = [129, 5]
    qkv, dctx = R.make_inputs(lens, HEADS, "normal", 2)
    rc, _, _ = _run(0, qkv, dctx, lens, None)
    assert rc == RS_EUNSUP
    assert b"128" in _lib.load().rs_last_error()


@pytest.mark.parametrize("family", ["normal", "peaked"])
def test_tiled_kernels_with_dropout_fed_to_the_reference(family):
    """p = 0.1: the keep bits of rs_dropout_keep in the saved-P layout, fed to the float64
    reference; the same bound.  The masks matter: the dropout-free reference is far off."""
    lens, klens, qkv, dctx, ref, r32 = _case("drop", family)
    rc, ctx, dqkv = _run(1, qkv, dctx, lens, klens, DROP)
    assert rc == 0
    _check(f"form1-drop-{family}", ctx, dqkv, ref, r32)
    _padding_zero(dqkv, lens, klens)
    plain = R.attn_batch(qkv, dctx, lens, HEADS, klens, None, torch.float64)
    assert (ctx.double() - plain[0]).abs().max().item() > 1e-2


def test_tiled_kernels_are_bitwise_reproducible():
    lens, klens, qkv, dctx, _, _ = _case("drop", "peaked")
    a = _run(1, qkv, dctx, lens, klens, DROP)
    b = _run(1, qkv, dctx, lens, klens, DROP)
    assert a[0] == 0 and b[0] == 0
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_keep_rate_over_one_512_token_sequence():
    n = HEADS * 512 * 512
    keep = _keep([512], **DROP).astype(np.float64)
    assert keep.size == n
    assert abs(keep.mean() - 0.9) <= 4 * np.sqrt(0.09 / n), keep.mean()
