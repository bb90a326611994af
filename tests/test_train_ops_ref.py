"""CPU: tests/train_ops_ref.py in float64 — the explicit forward / backward expressions the trainer's
non-attention kernels are compared with — against torch float64 autograd (LayerNorm, GELU,
cross-entropy, the three losses of oracle/train_ref.py, nn.Embedding(padding_idx=0)) and
torch.optim.AdamW, each to 1e-12 relative."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R

REL = 1e-12


def _close(got, want, what=""):
    want = want.double()
    assert (got.double() - want).abs().max().item() <= REL * max(1.0, want.abs().max().item()), what


def _randn(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


@pytest.mark.parametrize("H", [256, 768])
def test_layer_norm_forward_and_backward(H):
    M, eps = 9, 1e-12
    x, g, b, dy = _randn(M, H, seed=1), _randn(H, seed=2), _randn(H, seed=3), _randn(M, H, seed=4)
    x[3] = 100.0 + 1e-2 * x[3]                       # mean >> spread
    xa = x.double().requires_grad_(True)
    ga, ba = g.double().requires_grad_(True), b.double().requires_grad_(True)
    ya = F.layer_norm(xa, (H,), ga, ba, eps=R.f32(eps))
    ya.backward(dy.double())
    _, st, h = R.bias_res_ln(x, None, None, g, b, eps)
    _close(h, ya.detach(), "y")
    _close(R.ln_bwd(dy, x, st, g), xa.grad, "dx")       # st in float64: the exact statistics
    _close(R.colsum(dy, x, st, 1), ga.grad, "dgamma")
    _close(R.colsum(dy, None, None, 0), ba.grad, "dbeta")


def test_bias_residual_dropout_and_embedding_forward():
    M, H = 5, 256
    y, bias, res = _randn(M, H, seed=1), _randn(H, seed=2), _randn(M, H, seed=3)
    g, b = _randn(H, seed=4), _randn(H, seed=5)
    keep = (np.arange(M * H) % 7 != 0).astype(np.uint8)
    mult = R.keep_to_mult(keep, M, H, 0.1)
    assert mult[0, 0].item() == 0.0 and mult[0, 1].item() == pytest.approx(1 / 0.9, rel=1e-6)
    y1, _, h = R.bias_res_ln(y, bias, res, g, b, 1e-12, mult)
    want = F.dropout(y.double() + bias.double(), 0.0) * mult.double() + res.double()
    _close(y1, want)
    _close(h, F.layer_norm(want, (H,), g.double(), b.double(), eps=R.f32(1e-12)))
    # embeddings: ids clamped into their tables, no row_type = type row 0
    word, pos, typ = _randn(11, H, seed=6), _randn(8, H, seed=7), _randn(2, H, seed=8)
    tok, pidx = torch.tensor([0, 10, 99, -3, 5]), torch.tensor([0, 1, 2, 7, 3])
    x0, _, h0 = R.embed_ln(tok, pidx, torch.tensor([0, 1, 5, -1, 1]), word, pos, typ, g, b, 1e-12, mult)
    want = word.double()[[0, 10, 10, 0, 5]] + typ.double()[[0, 1, 1, 0, 1]] + pos.double()[pidx]
    _close(x0, want)
    _close(h0, F.layer_norm(want, (H,), g.double(), b.double(), eps=R.f32(1e-12)) * mult.double())
    x0n, _, _ = R.embed_ln(tok, pidx, None, word, pos, typ, g, b, 1e-12)
    _close(x0n, word.double()[[0, 10, 10, 0, 5]] + typ.double()[0] + pos.double()[pidx])


def test_gelu_and_its_derivative():
    x = torch.cat([torch.linspace(-12, 12, 4001), torch.tensor([0.0, -0.0, 1e-30, -1e-30])]).float()
    xa = x.double().requires_grad_(True)
    ya = F.gelu(xa)
    ya.backward(torch.ones_like(ya))
    bias = torch.zeros(1)
    pre, act = R.bias_gelu(x[None], bias)
    _close(act[0], ya.detach())
    d = _randn(x.numel(), seed=1)
    _close(R.gelu_bwd(d[None], x[None])[0], d.double() * xa.grad)


@pytest.mark.parametrize("V", [8, 257, 1000])
def test_cross_entropy_and_d_logits(V):
    M = 5
    x = _randn(M, V, seed=V, scale=8.0)
    lab = torch.tensor([0, V - 1, 3, -100, 1])
    x[2, 3] += 40.0
    xa = x.double().requires_grad_(True)
    la = F.cross_entropy(xa, lab.clamp(0, V - 1), reduction="mean")
    la.backward()
    rl, mean, d = R.ce(x, lab)
    _close(mean, la.detach())
    _close(rl, F.cross_entropy(x.double(), lab.clamp(0, V - 1), reduction="none"))
    _close(d, xa.grad)


@pytest.mark.parametrize("kind", ["MD", "MD_MWER", "MD_MWED"])
def test_losses_and_score_gradients(kind):
    sizes = [3, 1, 0, 16, 7, 2]
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    sc, tgt = _randn(n, seed=1, scale=3.0), _randn(n, seed=2, scale=3.0)
    am = -200.0 + 30.0 * _randn(n, seed=3)
    cer = torch.rand(n, generator=torch.Generator().manual_seed(4)).float() + 0.05
    dsc, ul, total = R.losses(sc, tgt, am, cer, off, kind, 0.5)
    ga, ta = R.loss_autograd(sc, tgt, am, cer, off, kind, 0.5)
    _close(total, ta, "loss")
    _close(dsc, ga, "dsc")
    assert ul[2].item() == 0.0


def test_embedding_gradients():
    H, lens = 256, [4, 1, 6]
    M = sum(lens)
    tok = torch.tensor([2, 0, 5, 2, 7, 2, 0, 9, 5, 5, 1])
    dx0 = _randn(M, H, seed=1)
    emb = torch.nn.Embedding(12, H, padding_idx=0).double()
    pe = torch.nn.Embedding(6, H).double()
    pidx = torch.cat([torch.arange(t) for t in lens])
    (emb(tok) + pe(pidx)).backward(dx0.double())
    dw0, dp0 = _randn(12, H, seed=2), _randn(6, H, seed=3)
    dw = R.word_grad(dx0, tok, dw0)
    _close(dw, dw0.double() + emb.weight.grad)
    assert torch.equal(dw[0], dw0[0].double())
    _close(R.pos_grad(dx0, lens, dp0), dp0.double() + pe.weight.grad)


def test_cls_head():
    H, lens = 256, [3, 1, 5]
    rows = torch.tensor([0, 3, 4])
    h, w, b, dsc = _randn(9, H, seed=1), _randn(H, seed=2), _randn(1, seed=3), _randn(3, seed=4)
    ha, wa, ba = (t.double().requires_grad_(True) for t in (h, w, b))
    out = ha[rows] @ wa + ba
    out.backward(dsc.double())
    _close(R.cls_fwd(h, rows, w, b), out.detach())
    dw0, db0 = _randn(H, seed=5), _randn(1, seed=6)
    dh, dw, db = R.cls_bwd(dsc, h, rows, w, dw0, db0)
    _close(dh, ha.grad)
    _close(dw, dw0.double() + wa.grad)
    _close(db, db0.double() + ba.grad)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("lr", [1e-3, 2e-5])
def test_adamw_steps(lr, wd):
    n, steps = 1025, 4
    hp = dict(lr=R.f32(lr), beta1=R.f32(0.9), beta2=R.f32(0.999), eps=R.f32(1e-8), wd=R.f32(wd))
    p0 = _randn(n, seed=1)
    grads = [_randn(n, seed=10 + k) * 10.0 ** torch.randint(-12, 4, (n,), generator=torch.Generator().manual_seed(k))
             for k in range(steps)]
    want = R.adamw_torch(p0, grads, dt=torch.float64, **hp)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for k, g in enumerate(grads):
        p, m, v = R.adamw_step(p, g.double(), m, v, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], k + 1)
        for got, ref, what in zip((p, m, v), want[k], "pmv"):
            _close(got, ref, (k, what))


def test_row_moves():
    x = _randn(7, 8, seed=1)
    rows = torch.tensor([6, 0, 3])
    inv = torch.full((7,), -1)
    inv[rows] = torch.arange(3)
    back = R.expand_rows(R.gather_rows(x, rows), inv, 7)
    assert torch.equal(back[rows], x[rows]) and (back[[1, 2, 4, 5]] == 0).all()
