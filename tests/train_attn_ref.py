"""Reference of the trainer's attention (k_train.hip), forward and backward, per sequence, with the
per-sequence key length of padded rows and a fed dropout mask, in any torch dtype; and the input
families of tests/test_gpu_train_attn.py.  CPU only: tests/test_train_attn_ref.py pins it against
torch float64 autograd.

Per (sequence, head), Q, K, V, dctx of shape [T, 64]:
  S = (Q K^T) 0.125, keys j >= klen masked; P = softmax(S); ctx = (P * m) V        (m = keep / (1 - p))
  dPd = (dctx V^T) * m; dS = P (dPd - rowsum(P dPd)); dQ = 0.125 dS K; dK = 0.125 dS^T Q;
  dV = (P * m)^T dctx
"""
import numpy as np
import torch

TILE = 64          # query- and key-tile size of the tiled kernels


def split_heads(x, heads):
    """[T, heads * 64] -> [heads, T, 64]"""
    return x.view(x.shape[0], heads, 64).transpose(0, 1)


def merge_heads(x):
    """[heads, T, 64] -> [T, heads * 64]"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def attn_seq(qkv, dctx, heads, klen=None, mult=None, dtype=torch.float64):
    """One sequence: qkv [T, 3H], dctx [T, H], mult (nullable) [heads, T, T] dropout multipliers.
    Returns (ctx [T, H], dqkv [T, 3H]) in ``dtype``."""
    T, H = dctx.shape
    x = qkv.to(dtype)
    q, k, v = (split_heads(x[:, i * H:(i + 1) * H], heads) for i in range(3))
    g = split_heads(dctx.to(dtype), heads)
    s = (q @ k.transpose(1, 2)) * 0.125
    if klen is not None and klen < T:
        s[:, :, klen:] = float("-inf")
    p = torch.softmax(s, dim=-1)
    pd = p if mult is None else p * mult.to(dtype)
    ctx = pd @ v
    dpd = g @ v.transpose(1, 2)
    if mult is not None:
        dpd = dpd * mult.to(dtype)
    ds = p * (dpd - (p * dpd).sum(-1, keepdim=True))
    dq = 0.125 * (ds @ k)
    dk = 0.125 * (ds.transpose(1, 2) @ q)
    dv = pd.transpose(1, 2) @ g
    return merge_heads(ctx), torch.cat([merge_heads(dq), merge_heads(dk), merge_heads(dv)], dim=1)


def attn_batch(qkv, dctx, lens, heads, klens=None, mults=None, dtype=torch.float64):
    """Ragged batch (rows back to back).  Returns (ctx [M, H], dqkv [M, 3H])."""
    ctx, dqkv, r0 = [], [], 0
    for i, t in enumerate(lens):
        c, d = attn_seq(qkv[r0:r0 + t], dctx[r0:r0 + t], heads, None if klens is None else int(klens[i]),
                        None if mults is None else mults[i], dtype)
        ctx.append(c)
        dqkv.append(d)
        r0 += t
    return torch.cat(ctx), torch.cat(dqkv)


def autograd_seq(qkv, dctx, heads, klen=None, mult=None):
    """The same through torch float64 autograd of softmax(Q K^T / 8 + mask) V (the additive
    finfo.min mask of transformers' eager attention)."""
    T, H = dctx.shape
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = (split_heads(x[:, i * H:(i + 1) * H], heads) for i in range(3))
    s = q @ k.transpose(1, 2) / 8
    if klen is not None and klen < T:
        m = torch.zeros(T, dtype=torch.float64)
        m[klen:] = torch.finfo(torch.float64).min
        s = s + m
    p = torch.softmax(s, dim=-1)
    if mult is not None:
        p = p * mult.double()
    ctx = merge_heads(p @ v)
    ctx.backward(dctx.double())
    return ctx.detach(), x.grad


def planted(T, klen=None):
    """The peaked family's planted (query row, key) pairs: a maximum in the first key tile, one in
    the last key tile and one at the last unmasked key (distinct rows where T allows)."""
    tk = T if klen is None else klen
    keys = [min(5, tk - 1), TILE * ((tk - 1) // TILE), tk - 1]
    rows = [0, T // 2, T - 1]
    return list(zip(rows, keys))


def make_inputs(lens, heads, family, seed, klens=None):
    """qkv [M, 3H], dctx [M, H] float32.  "normal": scores of spread ~1.4; "peaked": Q, K ~ 2.5 randn
    (score std ~6, extremes near 30) and per sequence three planted rows whose query is 0.6 k_j per
    head: score(i, j) = 0.075 |k_j|^2 ~ 30, above every other key of the row (std ~4)."""
    g = torch.Generator().manual_seed(seed)
    H = heads * 64
    M = int(sum(lens))
    sc = {"normal": 1.2, "peaked": 2.5}[family]
    qkv = torch.randn(M, 3, H, generator=g) * torch.tensor([sc, sc, 1.0]).view(1, 3, 1)
    dctx = torch.randn(M, H, generator=g)
    if family == "peaked":
        r0 = 0
        for i, t in enumerate(lens):
            for row, key in planted(t, None if klens is None else int(klens[i])):
                qkv[r0 + row, 0] = 0.6 * qkv[r0 + key, 1]
            r0 += t
    return qkv.view(M, 3 * H).contiguous(), dctx


def keep_to_mults(keep, lens, heads, p):
    """Keep bits in the saved-P layout (pofs[s] + h T^2 + i T + j) -> per-sequence [heads, T, T]
    float32 multipliers keep / (1 - p)."""
    scale = np.float32(1.0 / (1.0 - p))
    out, o = [], 0
    for t in lens:
        n = heads * t * t
        out.append(torch.from_numpy(keep[o:o + n].astype(np.float32) * scale).view(heads, t, t))
        o += n
    return out
