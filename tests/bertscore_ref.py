"""Helpers shared by the tests of the BERTScore kernels (a plain module, imported by name):
bs_recall_kernel (k_bertscore.hip), embed_out_kernel (k_bert.hip) and mbr_scores_bs_kernel
(k_rerank.hip) — tests/test_gpu_bertscore_ops.py, checked on the CPU in tests/test_bertscore_ref.py.

* the planar two-part embedding image [hi | lo*64] (embed_out_kernel<., true>, rs_token_embed) and
  its decoding;
* float64 / float32 evaluations of the recall matrices R and R0 as the kernel header defines them,
  and of the normalised embedding, on the values the buffers HOLD (operand quantisation is not part
  of the error);
* the ragged layouts and the input families of the GPU tests.
"""
import functools

import numpy as np
import torch

from tail_ref import distinct_affine, ln_apply, row_stats
from x3s_image import _split2, _unsplit2

FP16_MIN_NORMAL = 2.0 ** -14
HIDDEN = (256, 512, 768, 1024)


def bs_cols(two):
    """Ref columns per tile of bs_recall_kernel (BsCfg::COLS)."""
    return 32 if two else 64


def bs_groups(H):
    """Cand hypotheses per group of bs_recall_kernel (BsCfg::NG)."""
    return 64 if H == 1024 else 128


# ---- the planar two-part image -------------------------------------------------------------------

def encode_planar(x):
    """fp32 x [R, H] -> fp16 [R, 2H] = [hi | lo*64], hi = fp16(x), lo = x - hi."""
    hi = x.half()
    return torch.cat([hi, ((x - hi.float()) * 64.0).half()], dim=1).contiguous()


def decode_planar(img, dtype=torch.float64):
    """hi + lo/64 of a planar image [R, 2H] -> [R, H] (float64 is exact)."""
    H = img.shape[1] // 2
    return img[:, :H].to(dtype) + img[:, H:].to(dtype) / 64.0


def planar_defects(img):
    """Exact checks on a planar image alone (tail_ref.image3_defects for two parts): lo finite, and
    hi == fp16(hi + lo/64) bitwise except where the held value is an exact tie between hi and its
    neighbour (lo is itself rounded, so lo/64 can land on half a spacing of hi; hi is then still a
    nearest fp16 number)."""
    H = img.shape[1] // 2
    hi, lo = img[:, :H], img[:, H:]
    bad = []
    if not torch.isfinite(lo.float()).all():
        bad.append(f"lo not finite at {int((~torch.isfinite(lo.float())).sum())} elements")
    val = hi.double() + lo.double() / 64.0
    back = val.half()
    off = (back.view(torch.int16) != hi.contiguous().view(torch.int16)) & \
        ((val - hi.double()).abs() != (back.double() - val).abs())
    if off.any():
        bad.append(f"hi != RNE16(hi + lo / 64) at {int(off.sum())} elements")
    return bad


def held_values(emb, two):
    """float64 values of an embedding buffer: fp16 [N, H], or (two) the planar image [N, 2H].  A
    float32 / float64 tensor is taken as the values themselves."""
    if emb.dtype != torch.float16:
        return emb.double()
    return decode_planar(emb, torch.float64) if two else emb.double()


# ---- recall matrices -----------------------------------------------------------------------------

def mat_offsets(utt_off):
    n = np.diff(np.asarray(utt_off, np.int64))
    return np.concatenate([[0], np.cumsum(n * n)]).astype(np.int64)


def recall_ref(emb, hyp_off, utt_off, dtype, two=False):
    """R and R0 of every utterance and ordered pair (cand i, ref j), as k_bertscore.hip's header
    defines them, evaluated in ``dtype`` on the values ``emb`` holds:

        R(i|j)  = 1/(T_j - 2) sum over ref j's tokens t except [CLS], [SEP] of max_{s in i} e_s . e_t
        R0(i|j) = the same with every maximum clamped at 0
        both 0 where T_i <= 2 or T_j <= 2

    float64: the plain expression.  float32 follows the kernel's order: the fp32 matmul, the max, then
    the chain acc += v * w over the columns in order with w = 1.0f / (T_j - 2).  Returns two float64
    vectors holding the utterances' [n, n] blocks one after the other (mat_offsets)."""
    vals = held_values(emb, two).to(dtype)
    hyp_off = [int(v) for v in hyp_off]
    utt_off = [int(v) for v in utt_off]
    moff = mat_offsets(utt_off)
    R = torch.zeros(int(moff[-1]), dtype=dtype)
    R0 = torch.zeros(int(moff[-1]), dtype=dtype)
    for u in range(len(utt_off) - 1):
        h0, h1 = utt_off[u], utt_off[u + 1]
        n = h1 - h0
        if n == 0:
            continue
        r0 = hyp_off[h0]
        ho = [hyp_off[h] - r0 for h in range(h0, h1 + 1)]
        E = vals[r0:hyp_off[h1]]
        S = E @ E.t()                                           # [rows of the cand side, ref columns]
        M = torch.stack([S[ho[i]:ho[i + 1]].max(dim=0).values for i in range(n)])       # [n, columns]
        T = torch.tensor([ho[i + 1] - ho[i] for i in range(n)])
        blk = torch.zeros(n, n, dtype=dtype)
        blk0 = torch.zeros(n, n, dtype=dtype)
        for j in range(n):
            if T[j] <= 2:
                continue
            cols = M[:, ho[j] + 1:ho[j + 1] - 1]
            if dtype == torch.float64:
                blk[:, j] = cols.sum(dim=1) / float(T[j] - 2)
                blk0[:, j] = cols.clamp_min(0.0).sum(dim=1) / float(T[j] - 2)
            else:
                w = torch.tensor(1.0, dtype=dtype) / torch.tensor(float(T[j] - 2), dtype=dtype)
                acc, acc0 = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
                for t in range(cols.shape[1]):
                    acc = acc + cols[:, t] * w
                    acc0 = acc0 + cols[:, t].clamp_min(0.0) * w
                blk[:, j], blk0[:, j] = acc, acc0
        blk[T <= 2] = 0
        blk0[T <= 2] = 0
        R[int(moff[u]):int(moff[u + 1])] = blk.reshape(-1)
        R0[int(moff[u]):int(moff[u + 1])] = blk0.reshape(-1)
    return R.double(), R0.double()


# ---- layouts -------------------------------------------------------------------------------------

def recall_layout(cols, ng):
    """The ragged layout of one bs_recall_kernel instantiation (COLS = cols, NG = ng): the hypothesis
    lengths of every utterance.  Row counts are cand rows of the utterance (32 per MFMA tile, 256 per
    sweep of the 8 waves)."""
    C = cols
    short = (4, 5, 2, 3, 4, 5)                              # cycled through by the many-hypothesis utterances
    utts = [
        [5],                                                # n = 1, fewer than 32 rows
        [2, 3, C - 1, C, C + 1, C + 2, 2 * C, 2 * C + 1],   # every ref length at the tile edge; T = 2 first
        [],                                                 # an empty utterance between two others
        [10, 2, 20],                                        # exactly 32 rows; T = 2 inside
        [4, 27, 2],                                         # 33 rows; T = 2 last
        [20, 70, 40, 60, 65],                               # 255 rows; the 70-row hypothesis spans three tiles
        [50, 100, 106],                                     # 256 rows
        [120, 130, 7],                                      # 257 rows; the last one straddles the sweep boundary
        [200, 2, 150, 129, 40],                             # 521 rows: a third sweep; straddles 256 and 512
        # runs of short hypotheses: exactly C columns (one item), then C + 1 (cut before the last),
        # then a run with a T = 2 inside
        [C // 4] * 4 + [C // 4] * 3 + [C // 4 + 1] + [3, 2, C // 2, C // 2 - 5],
        [short[k % 6] for k in range(ng - 1)],              # n = NG - 1
        [short[(k + 1) % 6] for k in range(ng)],            # n = NG
        [short[(k + 2) % 6] for k in range(ng + 1)],        # n = NG + 1: a second cand group of one
    ]
    hyp_off = np.concatenate([[0], np.cumsum([t for u in utts for t in u])]).astype(np.int32)
    utt_off = np.concatenate([[0], np.cumsum([len(u) for u in utts])]).astype(np.int32)
    return utts, hyp_off, utt_off


# ---- input families of the recall kernel -----------------------------------------------------------

RECALL_FAMILIES = ("plain", "twin", "negative", "onehot", "spiky")
TWIN_COS = 0.9


def _unit(x):
    return x / x.norm(dim=1, keepdim=True)


def twin_plan(utts):
    """The copies of the twin family: a list of (dst_row, src_row).  Every interior row is the unique
    best match of its own column in the pair (i, i).  A [CLS] or [SEP] row of hypothesis i is not an
    interior column of anything, so an interior row of ANOTHER hypothesis j of the utterance is made
    a noisy copy of it: column dst of ref j then has its maximum over cand i at row src.  Slots are
    handed out from hypothesis i + 1 onwards (cyclic); -> (plan, uncovered) where uncovered lists the
    [CLS] / [SEP] rows (of hypotheses with T > 2) left without a copy because the other hypotheses of
    their utterance have no interior row left (n = 1, for instance)."""
    plan, uncovered, r0 = [], [], 0
    for u in utts:
        n = len(u)
        start = np.concatenate([[0], np.cumsum(u)]).astype(np.int64) + r0
        free = [list(range(int(start[j]) + 1, int(start[j + 1]) - 1)) for j in range(n)]
        for i in range(n):
            if u[i] <= 2:
                continue
            for src in (int(start[i]), int(start[i + 1]) - 1):
                for d in range(1, n):
                    j = (i + d) % n
                    if free[j]:
                        plan.append((free[j].pop(0), src))
                        break
                else:
                    uncovered.append(src)
        r0 = int(start[-1])
    return plan, uncovered


def recall_values(family, H, utts, seed=0):
    """fp32 embedding rows [N, H] of one family over the layout ``utts`` (before the buffer's rounding):

    plain     normalised randn rows
    twin      plain, with the interior rows twin_plan names replaced by noisy copies (cosine about
              TWIN_COS) of another hypothesis' [CLS] / [SEP] row
    negative  per utterance a unit direction u; hypothesis h holds normalise(s u + 0.5 z), z unit
              random, s = +1 for even h and -1 for odd h: across signs every cosine is negative
    onehot    unit basis vectors e_k, k seeded random, with rows whose k occurs twice re-pointed so
              that every k in [0, H) occurs
    spiky     8 components of +-0.35, the rest 1e-3 randn, normalised (outlier dimensions)
    """
    assert family in RECALL_FAMILIES, family
    gen = torch.Generator().manual_seed(seed)
    N = sum(sum(u) for u in utts)
    if family in ("plain", "twin"):
        x = _unit(torch.randn(N, H, generator=gen))
        if family == "twin":
            a = (1.0 / TWIN_COS ** 2 - 1.0) ** 0.5
            plan, _ = twin_plan(utts)
            dst = torch.tensor([d for d, _ in plan])
            src = torch.tensor([s for _, s in plan])
            x[dst] = _unit(x[src] + a * _unit(torch.randn(len(plan), H, generator=gen)))
        return x.contiguous()
    if family == "negative":
        x = torch.empty(N, H)
        r = 0
        for u in utts:
            d = _unit(torch.randn(1, H, generator=gen))
            for h, T in enumerate(u):
                s = 1.0 if h % 2 == 0 else -1.0
                x[r:r + T] = _unit(s * d + 0.5 * _unit(torch.randn(T, H, generator=gen)))
                r += T
        return x.contiguous()
    if family == "onehot":
        k = torch.randint(0, H, (N,), generator=gen)
        count = torch.bincount(k, minlength=H)
        r = N - 1
        for m in (count == 0).nonzero().flatten().tolist():      # onto rows whose k occurs elsewhere too
            while count[k[r]] < 2:
                r -= 1
            count[k[r]] -= 1
            k[r] = m
            r -= 1
        x = torch.zeros(N, H)
        x[torch.arange(N), k] = 1.0
        return x
    x = 1e-3 * torch.randn(N, H, generator=gen)
    for r in range(N):
        idx = torch.randperm(H, generator=gen)[:8]
        x[r, idx] = 0.35 * (torch.randint(0, 2, (8,), generator=gen) * 2 - 1).float()
    return _unit(x).contiguous()


def recall_buffer(x, two):
    """The kernel's embedding buffer for fp32 rows x: fp16 [N, H], or the planar image [N, 2H]."""
    return encode_planar(x) if two else x.half().contiguous()


@functools.lru_cache(maxsize=None)
def recall_case(family, H, two, seed=0):
    """One GPU case, computed once: the layout, the embedding buffer (CPU), the float64 reference,
    the float32 evaluation, and the bound's constant term c."""
    utts, hyp_off, utt_off = recall_layout(bs_cols(two), bs_groups(H))
    emb = recall_buffer(recall_values(family, H, utts, seed), two)
    ref = recall_ref(emb, hyp_off, utt_off, torch.float64, two)
    r32 = recall_ref(emb, hyp_off, utt_off, torch.float32, two)
    e32 = max((r32[0] - ref[0]).abs().max().item(), (r32[1] - ref[1]).abs().max().item())
    # the lo.lo/4096 product the split-operand cosine omits by design: each |lo/64| <= 2^-12 |e|
    c = 2.0 ** -24 * held_values(emb, two).norm(dim=1).max().item() ** 2 if two else 0.0
    return {"utts": utts, "hyp_off": hyp_off, "utt_off": utt_off, "emb": emb, "ref": ref, "r32": r32, "e32": e32, "c": c}


# ---- embed_out_kernel ----------------------------------------------------------------------------

EMBED_LENGTHS = (1, 2, 3, 4, 5, 9, 64, 65)


def embed_layout(s0=2, tail=2, gap=3):
    """Metadata of sequences [0, s0 + 8 + tail): s0 leading and ``tail`` trailing sequences the launch
    does not cover, the eight EMBED_LENGTHS in between.  Source rows: ``gap`` unused rows between the
    row ranges, first row row0 + gap.  Token offsets: the sequences laid out in REVERSE order with one
    unused token between them, so tok_off is another ordering than row.
    -> len, row, tok_off (int32 tensors), s0, s1, row0, rows (source rows from row0), tokens."""
    T = [6] * s0 + list(EMBED_LENGTHS) + [7] * tail
    row0 = 11
    row, r = [], row0 + gap
    for t in T:
        row.append(r)
        r += t + gap
    tok, o = [0] * len(T), 1
    for i in reversed(range(len(T))):
        tok[i] = o
        o += T[i] + 1
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    return i32(T), i32(row), i32(tok), s0, s0 + len(EMBED_LENGTHS), row0, r - row0, o


def embed_operands(family, H, rows, seed=0):
    """Both sources of embed_out_kernel, distinct per row.  (x32 [rows, H], stats, g, b): g / b the
    distinct ramps of tail_ref.distinct_affine; family "plain": x ~ 2 randn + 0.5; "offset": x = 30 +
    0.01 randn (row mean much larger than the row's spread).  himg [rows, 2H]: what the split-operand
    layers leave there, the interleaved two-part image of the normalised state — of LN(x2; g, b) in
    fp32 for a second x2 of the same family."""
    assert family in ("plain", "offset"), family
    gen = torch.Generator().manual_seed(seed + 5)
    z, z2 = torch.randn(rows, H, generator=gen), torch.randn(rows, H, generator=gen)
    shape = (lambda v: v * 2.0 + 0.5) if family == "plain" else (lambda v: 30.0 + 0.01 * v)
    x32, x2 = shape(z).contiguous(), shape(z2)
    g, b = distinct_affine(H)
    himg = _split2(ln_apply(x2, row_stats(x2), g, b, torch.float32))
    return {"x32": x32, "stats": row_stats(x32), "g": g, "b": b, "himg": himg}


def embed_out_ref(op, img, dtype):
    """e / ||e||_2 per row in ``dtype``: e = ((x - mean) rstd) g + b on the fp32 inputs given, or
    (img) the decoded interleaved image hi + lo/64."""
    if img:
        y = _unsplit2(op["himg"], torch.float64).to(dtype)
    else:
        y = ln_apply(op["x32"], op["stats"], op["g"], op["b"], dtype)
    return y / y.norm(dim=1, keepdim=True)
