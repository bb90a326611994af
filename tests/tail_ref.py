"""Helpers shared by the tests of the scoring tail (a plain module, imported by name): the last
layer's one-row-per-sequence kernels and the MLM head — tests/test_gpu_gemm_epi.py,
tests/test_gpu_attn_query.py, checked on the CPU in tests/test_tail_ref.py.

* the K-concatenated three-part operand images (common.h, kx == 3) and their decoding;
* float64 / float32 evaluations of every gemm_f16_kernel epilogue, of the decoder's log-softmax
  and of the scored-row attention, on the values the fp16 operands HOLD (operand quantisation is
  not part of the error);
* the input families of the GPU tests.
"""
import math

import torch

from x3s_image import _split2, _unsplit2

LN_EPS = 1e-12
FP16_MIN_NORMAL = 2.0 ** -14
EPI_GELU_F16, EPI_GELU_F32, EPI_RES_F32, EPI_BIAS_F32, EPI_RESLN_F32 = 1, 2, 3, 5, 6


# ---- three-part images -----------------------------------------------------------------------------

def _parts3(x):
    hi = x.half()
    return hi, (hi.float() / 64.0).half(), ((x - hi.float()) * 64.0).half()


def _split3(x):
    """The activation image of fp32 x [R, K] (common.h put_split, kx == 3): [hi | hi/64 | lo*64],
    lo = x - hi."""
    hi, mid, lo = _parts3(x)
    return torch.cat([hi, mid, lo], dim=1).contiguous()


def _split3w(w):
    """The weight image paired with it: [W_hi | W_lo*64 | W_hi/64], so that the K-concatenated
    product is A_hi.W_hi + A_hi.W_lo + A_lo.W_hi."""
    hi, mid, lo = _parts3(w)
    return torch.cat([hi, lo, mid], dim=1).contiguous()


def _unsplit3(img, dtype=torch.float32):
    """hi + lo / 64 of an activation image [R, 3N] -> [R, N] (float64 is exact)."""
    N = img.shape[1] // 3
    return img[:, :N].to(dtype) + img[:, 2 * N:].to(dtype) / 64.0


def image3_defects(img):
    """Exact checks on a three-part image alone, as a list of messages (empty: consistent):
    section 1 == fp16(float(section 0) / 64) bitwise, and fp16(float(sec0) + float(sec2) / 64) ==
    section 0 bitwise (hi is the RNE of the value the image holds; an exact tie may round to the
    other neighbour, see below)."""
    N = img.shape[1] // 3
    hi, mid, lo = img[:, :N], img[:, N:2 * N], img[:, 2 * N:]
    bad = []
    want_mid = (hi.float() / 64.0).half()
    if not torch.equal(mid.contiguous().view(torch.int16), want_mid.view(torch.int16)):
        bad.append(f"section 1 != fp16(hi / 64) at {int((mid != want_mid).sum())} elements")
    val = hi.double() + lo.double() / 64.0
    back = val.half()                                          # one rounding of the exact value
    # lo is itself rounded to fp16, so lo/64 can land exactly on half a spacing of hi: the held value
    # is then a tie between hi and its neighbour, RNE picks the even one, and hi is still a nearest
    # fp16 number.  Only such exact ties may differ.
    off = (back.view(torch.int16) != hi.contiguous().view(torch.int16)) & \
        ((val - hi.double()).abs() != (back.double() - val).abs())
    if off.any():
        bad.append(f"hi != RNE16(hi + lo / 64) at {int(off.sum())} elements")
    return bad


# ---- GEMM epilogues ------------------------------------------------------------------------------

def gemm_operands(family, M, N, K, seed=0, device="cpu"):
    """A [M, K], W [N, K] fp16.  family "fp16": A = fp16(randn), W = fp16(0.05 randn).  family
    "image3" (K = 3 K0): the real K-concatenated images of fp32 randn [M, K0] and 0.05 randn [N, K0]."""
    gen = torch.Generator(device=device).manual_seed(seed)
    if family == "fp16":
        A = torch.randn(M, K, device=device, generator=gen).half()
        W = (0.05 * torch.randn(N, K, device=device, generator=gen)).half()
        return A, W
    assert family == "image3" and K % 3 == 0, (family, K)
    A = _split3(torch.randn(M, K // 3, device=device, generator=gen))
    W = _split3w(0.05 * torch.randn(N, K // 3, device=device, generator=gen))
    return A, W


def flush_subnormal(t):
    """fp16 t with its subnormal elements replaced by 0 (what the fp16 MFMA does to an operand)."""
    return torch.where(t.float().abs() < FP16_MIN_NORMAL, torch.zeros_like(t), t)


def row_stats(x64, eps=LN_EPS):
    """(mean, 1 / sqrt(var + eps)) per row from a float64 LayerNorm of x, rounded to fp32: [R, 2]."""
    x64 = x64.double()
    mean = x64.mean(dim=1)
    var = ((x64 - mean[:, None]) ** 2).mean(dim=1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=1).float().contiguous()


def ln_apply(x, stats, g, b, dtype):
    """common.h ln_apply's expression ((x - mean) rstd) g + b evaluated in ``dtype`` on the fp32
    inputs given (the statistics are inputs: no variance is formed here)."""
    st = stats.to(dtype)
    return ((x.to(dtype) - st[:, :1]) * st[:, 1:]) * g.to(dtype) + b.to(dtype)


def distinct_affine(N, device="cpu"):
    """gamma[c] = 1 + c/N, beta[c] = c/N - 0.5 (x3s_image's distinct_affine family)."""
    c = torch.arange(N, device=device, dtype=torch.float32)
    return (1.0 + c / N).contiguous(), (c / N - 0.5).contiguous()


def epi_operands(kind, family, M, N, K, seed=0, device="cpu"):
    """Operands of one gemm_f16_kernel launch of epilogue ``kind``:
      res     out = A.W^T + b + res                       (EPI_RES_F32)
      gelu32  out = gelu(A.W^T + b), b spanning +-6       (EPI_GELU_F32)
      bias    out = A.W^T + b                             (EPI_BIAS_F32)
      resln   out = A.W^T + b + LN(res; stats, g, beta)   (EPI_RESLN_F32)
      defer   out = A.W^T + b + LN(LN0(res; stats0, g0, beta0) + o16; stats, g, beta)
      gelu16  image(gelu(A.W^T + b))                      (EPI_GELU_F16)
    """
    A, W = gemm_operands(family, M, N, K, seed, device)
    gen = torch.Generator(device=device).manual_seed(seed + 7919)

    def rn(*s):
        return torch.randn(*s, device=device, generator=gen)

    op = {"A": A, "W": W, "b": (0.1 * rn(N)).contiguous()}
    if kind in ("gelu32", "gelu16"):
        # pre-activations over the whole range the GELU bends in: b from -6 to 6 across the columns
        op["b"] = torch.linspace(-6.0, 6.0, N, device=device).contiguous()
    if kind in ("res", "resln", "defer"):
        op["res"] = (rn(M, N) * 2.0 + 0.5).contiguous()
    if kind in ("resln", "defer"):
        op["g"], op["beta"] = distinct_affine(N, device)
    if kind == "resln":
        op["stats"] = row_stats(op["res"])
    if kind == "defer":
        op["g0"], op["beta0"] = (1.0 + 0.1 * rn(N)).contiguous(), (0.1 * rn(N)).contiguous()
        op["stats0"] = row_stats(op["res"])
        op["o16"] = rn(M, N).half().contiguous()
        x = ln_apply(op["res"], op["stats0"], op["g0"], op["beta0"], torch.float64) + op["o16"].double()
        op["stats"] = row_stats(x)
    return op


def epi_ref(kind, op, dtype, flush=False):
    """The epilogue's expression in ``dtype`` (float64: the reference; float32: the yardstick).
    flush: subnormal operand elements count as 0."""
    A, W = (flush_subnormal(op["A"]), flush_subnormal(op["W"])) if flush else (op["A"], op["W"])
    y = A.to(dtype) @ W.to(dtype).t() + op["b"].to(dtype)
    if kind in ("gelu32", "gelu16"):
        return torch.nn.functional.gelu(y)
    if kind == "res":
        return y + op["res"].to(dtype)
    if kind == "resln":
        return y + ln_apply(op["res"], op["stats"], op["g"], op["beta"], dtype)
    if kind == "defer":
        x = ln_apply(op["res"], op["stats0"], op["g0"], op["beta0"], dtype) + op["o16"].to(dtype)
        return y + ln_apply(x, op["stats"], op["g"], op["beta"], dtype)
    assert kind == "bias", kind
    return y


# ---- decoder ---------------------------------------------------------------------------------------

DECODER_FAMILIES = ("plain", "peaked", "slab_spread", "flat")
POISON_BIAS = 30.0


def vocab_pad(V):
    return (V + 127) // 128 * 128


def decoder_tile(vpad):
    """Column width of the gemm_f16_kernel tile launch_epi gives a decoder of width vpad."""
    return 256 if vpad % 256 == 0 else 128


def decoder_weight(V, K, seed=0, device="cpu"):
    """W [vpad, K] fp16: 0.03 randn rows, the pad rows [V, vpad) poisoned with +-1 (a pad logit of
    about 30 +- sqrt(K))."""
    gen = torch.Generator(device=device).manual_seed(seed)
    vpad = vocab_pad(V)
    W = (0.03 * torch.randn(vpad, K, device=device, generator=gen)).half()
    if vpad > V:
        W[V:] = (torch.randint(0, 2, (vpad - V, K), device=device, generator=gen) * 2 - 1).half()
    return W.contiguous()


def decoder_labels(M, V, vpad, seed=0, device="cpu"):
    """Per row: column 0, 63, 64, V - 1, the first column of the last tile, then random columns,
    repeating with period 8 (three random rows per period)."""
    gen = torch.Generator(device=device).manual_seed(seed + 17)
    lab = torch.randint(0, V, (M,), device=device, generator=gen).to(torch.int32)
    special = [0, 63, 64, V - 1, min(vpad - decoder_tile(vpad), V - 1)]
    for i, c in enumerate(special):
        lab[i::8] = c
    return lab.contiguous()


def decoder_operands(family, M, V, K, W, seed=0, device="cpu"):
    """A [M, K] fp16, bias [vpad] fp32 (pad entries +30), labels [M] int32 for decoder_weight's W.

    plain        A ~ randn, b ~ 0.1 randn
    peaked       plain with b[p] += 80 for one column p; the label is p on even rows
    slab_spread  per 64-column slab: b += +200 on one slab, -200 on odd slabs, 0 on the other even
                 slabs: lse_finalize's rescaling underflows every slab but one
    flat         A = 0: the result is b[label] - logsumexp(b[:V])
    """
    assert family in DECODER_FAMILIES, family
    gen = torch.Generator(device=device).manual_seed(seed + 1)
    vpad = W.shape[0]
    A = torch.randn(M, K, device=device, generator=gen).half()
    b = 0.1 * torch.randn(vpad, device=device, generator=gen)
    lab = decoder_labels(M, V, vpad, seed, device)
    if family == "peaked":
        p = (V // 2) | 1
        b[p] += 80.0
        lab[0::2] = p
        lab[1::2] = torch.where(lab[1::2] == p, p - 1, lab[1::2])
    elif family == "slab_spread":
        slab = torch.arange(vpad, device=device) // 64
        off = torch.where(slab % 2 == 1, -200.0, 0.0)
        off[slab == (V // 64) // 2] = 200.0
        b = b + off
    elif family == "flat":
        A = torch.zeros_like(A)
    b[V:] = POISON_BIAS
    return A.contiguous(), b.float().contiguous(), lab


def decoder_ref(A, W, b, lab, V, dtype):
    """log_softmax(A.W^T + b)[:, :V] gathered at the label, in ``dtype``; also the label logit and
    the logsumexp (the sizes the bound's quantisation term scales with).  Labels outside [0, V)
    give -inf."""
    z = (A.to(dtype) @ W[:V].to(dtype).t() + b[:V].to(dtype))
    lse = torch.logsumexp(z, dim=1)
    ok = (lab >= 0) & (lab < V)
    ll = z.gather(1, lab.clamp(0, V - 1).long()[:, None])[:, 0]
    ll = torch.where(ok, ll, torch.full_like(ll, -math.inf))
    return ll - lse, ll, lse


# ---- scored-row attention --------------------------------------------------------------------------

ATTN_LENGTHS = (1, 2, 3, 63, 64, 65, 128, 129, 512)


def attn_layout(s0=2, tail=1, gap=3):
    """Metadata of sequences [0, s0 + 9 + tail): s0 leading and ``tail`` trailing sequences the
    launch does not cover, the nine ATTN_LENGTHS in between, ``gap`` unused rows between row ranges;
    query = 0, T - 1 or interior in turn.  -> len, row, query (int32 tensors), s0, s1, rows."""
    T = [5] * s0 + list(ATTN_LENGTHS) + [7] * tail
    row, query, r = [], [], gap
    for i, t in enumerate(T):
        row.append(r)
        r += t + gap
        query.append((0, t - 1, t // 2)[i % 3])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return i32(T), i32(row), i32(query), s0, s0 + len(ATTN_LENGTHS), r


def attn_operands(family, H, qkv32, dense_q, layout, seed=0, device="cpu"):
    """qkv [rows, 3H] (fp32, or fp16 values held in fp32) with distinct contents on every row, and
    qd [s1 - s0, H] or None.  With qd the Q columns of qkv keep other values than qd.

    plain   Q, K, V ~ 0.6 randn
    peaked  Q, K ~ 3 randn (score std ~ 9: far-negative scores), V ~ 0.6 randn, and one planted key per
            sequence (T > 1) and head whose score is 80 above the largest of the others: K_j = c q
            with c = 8 (max_other + 80) / |q|^2 per head; for T > 64 the planted key lies in the last
            64-key block, so the online softmax's running maximum changes late
    """
    T, row, query, s0, s1, rows = layout
    gen = torch.Generator(device=device).manual_seed(seed)
    scale = (3.0, 3.0, 0.6) if family == "peaked" else (0.6, 0.6, 0.6)
    qkv = torch.randn(rows, 3, H, device=device, generator=gen) * torch.tensor(scale, device=device).view(1, 3, 1)
    q = torch.stack([qkv[int(row[s]) + int(query[s]), 0] for s in range(s0, s1)]).clone()
    if not qkv32:
        qkv, q = qkv.half().float(), q.half().float()
    if family == "peaked":
        for i, s in enumerate(range(s0, s1)):
            t, r0 = int(T[s]), int(row[s])
            if t == 1:
                continue
            j = 64 * ((t - 1) // 64) + (t - 1 - 64 * ((t - 1) // 64)) // 2
            qh = q[i].double().view(-1, 64)                                        # [heads, 64]
            sc = torch.einsum("thd,hd->th", qkv[r0:r0 + t, 1].double().view(t, -1, 64), qh) / 8
            sc[j] = -math.inf
            c = 8 * (sc.max(dim=0).values + 80.0) / (qh * qh).sum(dim=1)
            qkv[r0 + j, 1] = (c[:, None] * qh).reshape(-1).float()
    for i, s in enumerate(range(s0, s1)):
        # the Q the kernel must use sits in qkv (qd null) or only in qd (the qkv copy differs)
        qkv[int(row[s]) + int(query[s]), 0] = q[i] if not dense_q else -q[i] - 1.0
    if not qkv32:
        qkv = qkv.half().float()
    qkv = qkv.view(rows, 3 * H).contiguous()
    return qkv, (q.contiguous() if dense_q else None), q


def attn_query_ref(qkv, q, layout, H, heads, dtype):
    """softmax(q.K^T / 8).V per head for the scored row of every sequence of [s0, s1) -> [s1 - s0, H]."""
    T, row, query, s0, s1, rows = layout
    out = torch.empty(s1 - s0, H, device=qkv.device, dtype=dtype)
    for i, s in enumerate(range(s0, s1)):
        t, r0 = int(T[s]), int(row[s])
        x = qkv[r0:r0 + t].to(dtype).view(t, 3, heads, 64)
        k, v = x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)          # [heads, t, 64]
        sc = (q[i].to(dtype).view(heads, 1, 64) @ k.transpose(1, 2)) * 0.125
        out[i] = (torch.softmax(sc, dim=-1) @ v).reshape(H)
    return out


def attn_residual_operands(rows, H, seed=0, device="cpu"):
    """Both residual sources of attn_query_kernel, distinct per row: the pre-LN stream x32 [rows, H]
    with its statistics and distinct_affine (g, b), and the two-part image himg [rows, 2H]."""
    gen = torch.Generator(device=device).manual_seed(seed + 5)
    x32 = (torch.randn(rows, H, device=device, generator=gen) * 2.0 + 0.5).contiguous()
    g, b = distinct_affine(H, device)
    himg = _split2(torch.randn(rows, H, device=device, generator=gen))
    return {"x32": x32, "stats": row_stats(x32), "g": g, "b": b, "himg": himg}
