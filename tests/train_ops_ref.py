"""Reference of the trainer's non-attention kernels (k_train.hip): plain torch expressions of each
op in any dtype — float64 is the reference, float32 gives e32, the error of the same expressions at
the kernels' precision — written from the formulas in the kernel comments, csrc/train.h and
oracle/train_ref.py.  CPU only: tests/test_train_ops_ref.py pins them against torch float64
autograd / torch.optim.AdamW; tests/test_gpu_train_ops.py compares the kernels with them.

Inputs are float32 tensors (what the kernels are given), converted to ``dt`` first.  Dropout is fed
as float32 multipliers keep / (1 - p) of element row * H + c (``keep_to_mult``).

The ops whose kernels use the fast intrinsics (tr_ce, tr_gelu_bwd: ``__expf`` = exp2(x log2 e),
``__logf`` = log2(x) ln 2) are written in those function forms, so the float32 evaluation carries
the argument rounding the form has by construction; the losses (expf / logf) use exp / log.
"""
import math

import numpy as np
import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
INV_SQRT2 = 0.7071067811865476
INV_SQRT_2PI = 0.3989422804014327
LOSS_KINDS = {"MD": 0, "MD_MWER": 1, "MD_MWED": 2}


def f32(x):
    """A python float rounded to float32: the value a kernel receives for a float argument."""
    return float(np.float32(x))


def exp_fast(x):
    return torch.exp2(x * LOG2E)


def log_fast(x):
    return torch.log2(x) * LN2


def keep_to_mult(keep, M, H, p):
    """Keep bits of elements row * H + c -> float32 [M, H] multipliers keep / (1 - p)."""
    scale = np.float32(1.0 / (1.0 - p))
    return torch.from_numpy(keep[:M * H].astype(np.float32) * scale).view(M, H)


# ---- row ops -------------------------------------------------------------------------------------

def ln_fwd(x, g, b, eps):
    """x [M, H] in its dtype -> (st [M, 2] = (mean, rstd), y); biased variance about the mean."""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(eps))
    return torch.cat([mean, rstd], dim=1), (x - mean) * rstd * g + b


def embed_ln(tok, pos_idx, typ, word, pos, typetab, g, b, eps, mult=None, dt=torch.float64):
    """x0 = (word[tok] + type[typ, 0 without]) + pos[t]; st; h0 = drop(LN(x0)).  Ids are clamped
    into their tables."""
    word, pos, typetab, g, b = (t.to(dt) for t in (word, pos, typetab, g, b))
    tok = tok.long().clamp(0, word.shape[0] - 1)
    ty = torch.zeros_like(tok) if typ is None else typ.long().clamp(0, typetab.shape[0] - 1)
    x0 = (word[tok] + typetab[ty]) + pos[pos_idx.long()]
    st, h = ln_fwd(x0, g, b, eps)
    if mult is not None:
        h = h * mult.to(dt)
    return x0, st, h


def bias_res_ln(y, bias, res, g, b, eps, mult=None, dt=torch.float64):
    """y <- drop(y + bias) + res; st; h = LN(y).  bias None: plain LN of y."""
    y, g, b = y.to(dt), g.to(dt), b.to(dt)
    if bias is not None:
        y = y + bias.to(dt)
        if mult is not None:
            y = y * mult.to(dt)
        y = y + res.to(dt)
    st, h = ln_fwd(y, g, b, eps)
    return y, st, h


def xhat_of(x, st):
    return (x - st[:, 0:1]) * st[:, 1:2]


def ln_bwd(dy, x, st, g, dt=torch.float64):
    """dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), from the saved (mean, rstd)."""
    dy, x, st, g = dy.to(dt), x.to(dt), st.to(dt), g.to(dt)
    gd = g * dy
    xh = xhat_of(x, st)
    c1 = gd.mean(dim=-1, keepdim=True)
    c2 = (gd * xh).mean(dim=-1, keepdim=True)
    return st[:, 1:2] * (gd - c1 - xh * c2)


# ---- pointwise ops -------------------------------------------------------------------------------

def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * INV_SQRT2))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * INV_SQRT2)) + x * INV_SQRT_2PI * exp_fast(-0.5 * x * x)


def bias_add(y, bias, dt=torch.float64):
    return y.to(dt) + bias.to(dt)


def bias_gelu(pre, bias, dt=torch.float64):
    """-> (pre + bias, gelu(pre + bias))"""
    v = bias_add(pre, bias, dt)
    return v, gelu(v)


def gelu_bwd(d, pre, dt=torch.float64):
    return d.to(dt) * gelu_grad(pre.to(dt))


# ---- column sums ---------------------------------------------------------------------------------

def colsum(dy, x, st, mode, rows=None, out0=None, dt=torch.float64):
    """mode 0: sum_r dy; 1: sum_r dy * xhat, over the rows of the boolean mask ``rows`` (None: all),
    added to ``out0`` when given."""
    v = dy.to(dt)
    if mode == 1:
        v = v * xhat_of(x.to(dt), st.to(dt))
    if rows is not None:
        v = v[rows]
    s = v.sum(dim=0)
    return s if out0 is None else out0.to(dt) + s


# ---- embedding gradients -------------------------------------------------------------------------

def word_grad(dx0, tok, dword0, dt=torch.float64):
    """dword0 + per token the sum of its rows of dx0; the pad id 0 takes no gradient."""
    acc = torch.zeros(dword0.shape, dtype=dt).index_add_(0, tok.long(), dx0.to(dt))
    acc[0] = 0
    return dword0.to(dt) + acc


def pos_grad(dx0, lens, dpos0, dt=torch.float64):
    """dpos0 [tmax, H] + per position the sum over the sequences that reach it."""
    acc = torch.zeros(dpos0.shape, dtype=dt)
    r0 = 0
    for t in lens:
        acc[:t] += dx0[r0:r0 + t].to(dt)
        r0 += t
    return dpos0.to(dt) + acc


# ---- CLS head ------------------------------------------------------------------------------------

def cls_fwd(h, cls_rows, w, b, dt=torch.float64):
    return h.to(dt)[cls_rows] @ w.to(dt) + b.to(dt)


def cls_bwd(dsc, h, cls_rows, w, dw0, db0, dt=torch.float64):
    """-> (dh [M, H], zero off the CLS rows; dw0 + sum_s dsc_s h[CLS_s]; db0 + sum_s dsc_s)"""
    dsc, h, w = dsc.to(dt), h.to(dt), w.to(dt)
    dh = torch.zeros(h.shape, dtype=dt)
    dh[cls_rows] = dsc[:, None] * w[None, :]
    return dh, dw0.to(dt) + (dsc[:, None] * h[cls_rows]).sum(dim=0), db0.to(dt) + dsc.sum()


# ---- distillation losses (csrc/train.h) ----------------------------------------------------------

def _softmax(x):
    e = torch.exp(x - x.max())
    return e / e.sum()


def losses(sc, tgt, am, cer, utt_off, kind, md_w, dt=torch.float64):
    """-> (dsc [n_hyp], uloss [n_utt], loss) of MD / MD_MWER / MD_MWED with the explicit gradients:
      MD      dsc = w 2 (s - t)                       (w = 1 for MD alone, else md_w)
      MWER    P = softmax(c), d = e - sum e / n; l = sum P d; dc = P (d - l)
      MWED    E = softmax(e), T = sum c / sum e, Q = softmax(c / T); l = sum E (log E - log Q);
              dz = Q sum E - E; dT = sum dz (-c / T^2); dc = dz / T + dT / sum e
    An empty group contributes nothing."""
    sc, tgt, am, cer = (t.to(dt) for t in (sc, tgt, am, cer))
    md = ((sc - tgt) ** 2).sum()
    wmd = 1.0 if kind == "MD" else f32(md_w)
    dsc = wmd * (2.0 * (sc - tgt))
    n_utt = len(utt_off) - 1
    ul = torch.zeros(n_utt, dtype=dt)
    if kind == "MD":
        return dsc, ul, md
    for u in range(n_utt):
        a, b = int(utt_off[u]), int(utt_off[u + 1])
        if b <= a:
            continue
        c, e = sc[a:b] + am[a:b], cer[a:b]
        if kind == "MD_MWER":
            p = _softmax(c)
            d = e - e.sum() / (b - a)
            l = (p * d).sum()
            dsc[a:b] += p * (d - l)
        else:
            E = _softmax(e)
            T = c.sum() / e.sum()
            Q = _softmax(c / T)
            l = torch.where(E > 0, E * (torch.log(E) - torch.log(Q)), torch.zeros_like(E)).sum()
            dz = Q * E.sum() - E
            dT = (dz * (-c / (T * T))).sum()
            dsc[a:b] += dz / T                              # two adds into dsc, as tr_loss_kernel does:
            dsc[a:b] += dT / e.sum()                        # each rounds at the magnitude of 2 w (s - t)
        ul[u] = l
    return dsc, ul, ul.sum() + wmd * md


def loss_autograd(sc, tgt, am, cer, utt_off, kind, md_w):
    """The loss expressions of oracle/train_ref.py per (ragged) group through float64 autograd."""
    s = sc.double().clone().requires_grad_(True)
    tgt, am, cer = tgt.double(), am.double(), cer.double()
    md = torch.nn.functional.mse_loss(s, tgt, reduction="sum")
    total = md if kind == "MD" else f32(md_w) * md
    for u in range(len(utt_off) - 1):
        a, b = int(utt_off[u]), int(utt_off[u + 1])
        if b <= a or kind == "MD":
            continue
        mix, c = (s[a:b] + am[a:b]).view(1, -1), cer[a:b].view(1, -1)
        if kind == "MD_MWER":
            p = torch.softmax(mix, dim=-1)
            avg = (torch.sum(c, dim=-1) / (b - a)).unsqueeze(dim=-1)
            total = total + torch.sum(torch.mul(p, c - avg))
        else:
            err = torch.softmax(c, dim=-1)
            temp = (torch.sum(mix, dim=-1) / torch.sum(c, dim=-1)).unsqueeze(dim=-1)
            q = torch.softmax(mix / temp, dim=-1)
            total = total + torch.nn.functional.kl_div(torch.log(q), err, reduction="sum")
    total.backward()
    return s.grad, total.detach()


# ---- MLM cross-entropy ---------------------------------------------------------------------------

def ce(logits, labels, dt=torch.float64):
    """-> (row losses lse - logit[label], their mean, d mean / d logits = (softmax - onehot) / M);
    labels clamped into [0, V)."""
    x = logits.to(dt)
    M, V = x.shape
    lab = labels.long().clamp(0, V - 1)
    m = x.max(dim=-1, keepdim=True).values
    lse = m + log_fast(exp_fast(x - m).sum(dim=-1, keepdim=True))
    rl = (lse - x.gather(1, lab[:, None]))[:, 0]
    onehot = torch.zeros_like(x).scatter_(1, lab[:, None], 1.0)
    return rl, rl.sum() / M, (exp_fast(x - lse) - onehot) * (1.0 / M)


# ---- AdamW ---------------------------------------------------------------------------------------

def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """One torch.optim.AdamW step (decoupled decay, lerp'd exp_avg, bias-corrected) in the tensors'
    dtype; hyper-parameters are python floats.  -> (p, m, v)"""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p = p * (1.0 - lr * wd)
    m = m + (1.0 - beta1) * (g - m)
    v = v * beta2 + (1.0 - beta2) * g * g
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adamw_torch(p0, grads, lr, beta1, beta2, eps, wd, dt):
    """torch.optim.AdamW(foreach=False) over the steps of ``grads`` from zero moments.
    -> per step (p, m, v) in ``dt``."""
    p = torch.nn.Parameter(p0.to(dt).clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, foreach=False)
    out = []
    for g in grads:
        p.grad = g.to(dt).clone()
        opt.step()
        s = opt.state[p]
        out.append((p.detach().clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone()))
    return out


# ---- row moves -----------------------------------------------------------------------------------

def gather_rows(x, rows):
    return x[rows.long()]


def expand_rows(src, inv, M):
    out = torch.zeros(M, src.shape[1], dtype=src.dtype)
    sel = inv.long() >= 0
    out[sel] = src[inv.long()[sel]]
    return out
