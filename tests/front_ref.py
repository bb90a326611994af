"""Helpers shared by the tests of the scoring front end (a plain module, imported by name): the
layer-0 embedding kernels, the layer-0 dedup attention, the multi-query tail, the gathers and the
two small heads — tests/test_gpu_front_ops.py, tests/test_gpu_attn_plan.py, checked on the CPU in
tests/test_front_ref.py.

* the metadata layouts (the 12-sequence array of the embedding tests, the dedup chunk, the query
  lists) and the restatement of "unique row of (s, t)" as k_attn.hip's SeqRows documents it; the
  unique-row plan itself is the production one (rs_debug_plan_unique -> seq_plan.h plan_unique_rows);
* float64 / float32 references: the embedding sum, the row statistics, attention on materialised
  rows, the sequential float64 segment sum (the LayerNorm is x3s_image.ln_ref64, the per-query
  attention tail_ref.attn_query_ref);
* the exact checks of the interleaved two-part image alone, and the operand families.
"""
import ctypes

import numpy as np
import torch

from x3s_image import _split2, _unsplit2  # noqa: F401  (re-exported: the kx = 2 decoders)

LN_EPS = 1e-12
VOCAB, TYPE_VOCAB, MAX_POS, MASK_ID = 64, 2, 160, 3
HIDDEN = (256, 512, 768, 1024)
META_FIELDS = ("tok_off", "len", "mask_pos", "mask_end", "query", "label", "row", "urow_h", "urow_m", "first", "seq",
               "pos", "qlabel")


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32)


# ---- the interleaved two-part image --------------------------------------------------------------

def deinterleave2(img):
    """(hi, lo) [R, N] of an interleaved image [R, 2N] = [hi 0..31 | lo 0..31 | hi 32..63 | ...]."""
    R, N2 = img.shape
    v = img.view(R, N2 // 64, 2, 32)
    return v[:, :, 0].reshape(R, N2 // 2), v[:, :, 1].reshape(R, N2 // 2)


def image2_defects(img):
    """Exact checks on an interleaved two-part image alone (tail_ref.image3_defects for kx = 2), as a
    list of messages: lo finite, and hi == fp16(hi + lo/64) bitwise except where the held value is an
    exact tie between hi and its neighbour (lo is itself rounded to fp16, so lo/64 can land on half a
    spacing of hi; hi is then still a nearest fp16 number)."""
    hi, lo = deinterleave2(img)
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


def image2_of(v):
    """What put_split writes for fp32 v (kx = 2): hi = RNE16(v), lo = RNE16(64 (v - hi)) — 64 (v - hi)
    is exact in fp32, so this is one rounding."""
    return _split2(v)


# ---- metadata --------------------------------------------------------------------------------------

def meta_struct(meta, device="cuda"):
    """(DebugMeta, keep-alive list) of a dict of int32 tensors; missing / None columns stay null."""
    from asr_rescoring_amd import _lib
    dm, keep = _lib.DebugMeta(), []
    for k, v in meta.items():
        assert k in META_FIELDS, k
        if v is None:
            continue
        t = v.to(device=device, dtype=torch.int32).contiguous()
        keep.append(t)
        setattr(dm, k, t.data_ptr())
    return dm, keep


def plan_unique(tok_off, T, lo, hi, s0, s1):
    """The production plan (seq_plan.h plan_unique_rows through rs_debug_plan_unique, host only) on
    the chunk [s0, s1): urow_h, urow_m (int32 tensors over the whole array; entries outside the chunk
    keep -1) and the chunk's unique-row count."""
    from asr_rescoring_amd import _lib
    a = [np.ascontiguousarray(np.asarray(v), np.int32) for v in (tok_off, T, lo, hi)]
    n = len(a[0])
    uh, um = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    P = ctypes.c_void_p
    urows = _lib.load().rs_debug_plan_unique(*[P(v.ctypes.data) for v in a], n, s0, s1, P(uh.ctypes.data),
                                             P(um.ctypes.data))
    assert urows >= 0, urows
    return torch.from_numpy(uh), torch.from_numpy(um), urows


def pad_to(n, align):
    return (n + align - 1) // align * align


EMBED_LENGTHS = (1, 2, 3, 4, 5, 9, 64, 65, 130)
# per EMBED_LENGTHS: the [MASK] span — none, one position, three wide, ending at T - 1
EMBED_SPANS = ((-1, -1), (-1, -1), (1, 2), (1, 3), (1, 4), (3, 6), (17, 18), (60, 64), (100, 103))
# per EMBED_LENGTHS: the query list of the multi-mask form (1, 2, 3, 4, 5 and 9 positions; position 1 and
# T - 2; adjacent positions in one list)
EMBED_QUERIES = ((0,), (1,), (1,), (1, 2), (1, 2, 3), (1, 3, 4, 7), (1, 2, 30, 31, 62),
                 (1, 5, 6, 7, 20, 40, 41, 62, 63), (64, 128))


def embed_layout(row0=11, s0=2, tail=1, gap=3, sentinel_rows=16):
    """The 12-sequence metadata array of the embedding tests, launched over [s0, s1) = [2, 11): the nine
    EMBED_LENGTHS with their EMBED_SPANS and EMBED_QUERIES, ``gap`` unused rows between the row ranges
    (first row row0 + gap), token offsets in the REVERSE order with one unused token between the
    sequences.  The sequences outside the launch are poisoned: their rows point into the
    ``sentinel_rows`` rows after the launch's last row range, which every output must leave untouched.
    -> dict: meta (int32 tensors: tok_off, len, mask_pos, mask_end, row, first, seq, pos), s0, s1, row0,
    rows (buffer rows counted from row0, the sentinel rows included), n_tok."""
    T = [6] * s0 + list(EMBED_LENGTHS) + [7] * tail
    s1 = s0 + len(EMBED_LENGTHS)
    spans = [(1, 3)] * s0 + list(EMBED_SPANS) + [(2, 5)] * tail
    lists = [(1, 4)] * s0 + list(EMBED_QUERIES) + [(2, 3, 5)] * tail
    row, r = [0] * len(T), row0 + gap
    for s in range(s0, s1):
        row[s] = r
        r += T[s] + gap
    for k, s in enumerate(list(range(s0)) + list(range(s1, len(T)))):
        row[s] = r + 1 + (k % 2)                               # inside the sentinel rows (T <= 7 < 16 - 2)
    rows = r - row0 + sentinel_rows
    tok, o = [0] * len(T), 1
    for s in reversed(range(len(T))):
        tok[s] = o
        o += T[s] + 1
    first, seq, pos = [0], [], []
    for s, ql in enumerate(lists):
        assert all(0 <= p < T[s] for p in ql) and list(ql) == sorted(set(ql))
        seq += [s] * len(ql)
        pos += list(ql)
        first.append(len(pos))
    meta = {"tok_off": i32(tok), "len": i32(T), "mask_pos": i32(a for a, _ in spans), "mask_end": i32(b for _, b in spans),
            "row": i32(row), "first": i32(first), "seq": i32(seq), "pos": i32(pos)}
    return {"meta": meta, "s0": s0, "s1": s1, "row0": row0, "rows": rows, "n_tok": o}


def launch_rows(meta, s0, s1, row0=0):
    """The buffer rows (from row0) the launch over [s0, s1) owns, in (s, t) order, with their s, t."""
    rs, ss, ts = [], [], []
    for s in range(s0, s1):
        T = int(meta["len"][s])
        rs += [int(meta["row"][s]) - row0 + t for t in range(T)]
        ss += [s] * T
        ts += list(range(T))
    return torch.tensor(rs), torch.tensor(ss), torch.tensor(ts)


def expand_queries(lay):
    """For the bit comparison of embed_ln_set with embed_ln: a form-0 layout with, for every sequence s
    of the launch, one unmasked copy (-1 / -1) and one copy per query position p whose one-position
    span is [p, p + 1) — the same tokens (tok_off), rows of their own, row0 = 0.  Also src: for every row
    of the set launch (launch_rows order, row0 = 0) the row of the expanded layout that holds the same
    (sequence, position, masked?)."""
    m, s0, s1 = lay["meta"], lay["s0"], lay["s1"]
    T, tok, row, lo, hi, src = [], [], [], [], [], []
    r = 2
    for s in range(s0, s1):
        t, ql = int(m["len"][s]), [int(p) for p in m["pos"][int(m["first"][s]):int(m["first"][s + 1])]]
        base = {}
        for p in [-1] + ql:
            T.append(t); tok.append(int(m["tok_off"][s])); row.append(r)
            lo.append(p); hi.append(p + 1 if p >= 0 else -1)
            base[p] = r
            r += t + 1
        src += [base[p if p in ql else -1] + p for p in range(t)]
    meta = {"tok_off": i32(tok), "len": i32(T), "mask_pos": i32(lo), "mask_end": i32(hi), "row": i32(row)}
    return {"meta": meta, "s0": 0, "s1": len(T), "row0": 0, "rows": r + 2, "n_tok": lay["n_tok"]}, torch.tensor(src)


# ---- the dedup chunk -------------------------------------------------------------------------------

def pll_spans(T):
    return [(p, p + 1) for p in range(1, T - 1)]


# (T, spans of the copies): the PLL run (one-position spans ascending over 1 .. T - 2); a run cut at the
# chunk start whose first copy masks position 5 and whose copies of positions 8 and 9 are absent (its
# range [5, T - 1) has [MASK] rows no copy reads); a whole-word run with overlapping wide spans; a
# one-copy run with a wide span; a T = 3 hypothesis
RUNS_48 = ((16, pll_spans(16)),
           (17, [(p, p + 1) for p in (5, 6, 7, 10, 11, 12, 13, 14, 15)]),
           (33, [(1, 4), (1, 4), (1, 4), (4, 9), (5, 9), (8, 9), (9, 32), (30, 32)]),
           (48, [(10, 30)]),
           (3, [(1, 2)]))
RUNS_64 = RUNS_48 + ((49, [(1, 2), (20, 48), (47, 48)]), (64, [(5, 6), (6, 7), (40, 63), (62, 63)]))
RUNS_130 = RUNS_64 + ((65, [(1, 2), (60, 64), (63, 64)]), (130, [(1, 2), (60, 70), (64, 65), (100, 129), (128, 129)]))
RUNS = {48: RUNS_48, 64: RUNS_64, 130: RUNS_130}


def dedup_chunk(runs, s0=2, tail=1, gap=2, row0=0, sentinel_rows=16):
    """The chunk [s0, s1) of the masked copies of ``runs`` inside a metadata array with s0 leading and
    ``tail`` trailing sequences the launch does not cover.  The copies of a run share tok_off and T
    (that is how the plan finds a run); rows: one range per copy, ``gap`` unused rows between them, first
    row row0 + gap; urow_h / urow_m / urows from the production plan.  The outside sequences are
    poisoned: rows inside the sentinel rows after the last range, unique rows at and past urows (inside
    the padding of the unique-row buffer), so whatever a kernel does for them shows in a sentinel.
    -> dict: meta, s0, s1, row0, rows (from row0, sentinel rows included), urows, n_tok, run (the run index
    of every sequence, -1 outside), ranges (per run: [min lo, max hi))."""
    T, tok, lo, hi, run = [6] * s0, [0] * s0, [1] * s0, [3] * s0, [-1] * s0
    o, ranges = 7, []
    for k, (t, spans) in enumerate(runs):
        assert t >= 3 and all(1 <= a < b <= t - 1 for a, b in spans), (t, spans)
        for a, b in spans:
            T.append(t); tok.append(o); lo.append(a); hi.append(b); run.append(k)
        ranges.append((min(a for a, _ in spans), max(b for _, b in spans)))
        o += t + 1
    s1 = len(T)
    T += [7] * tail; tok += [o] * tail; lo += [2] * tail; hi += [5] * tail; run += [-1] * tail
    o += 8 * tail
    row, r = [0] * len(T), row0 + gap
    for s in range(s0, s1):
        row[s] = r
        r += T[s] + gap
    outside = list(range(s0)) + list(range(s1, len(T)))
    for k, s in enumerate(outside):
        row[s] = r + 1 + (k % 2)
    rows = r - row0 + sentinel_rows
    uh, um, urows = plan_unique(tok, T, lo, hi, s0, s1)
    assert urows > 0
    for k, s in enumerate(outside):                            # poisoned: unique rows past the plan's
        uh[s] = urows + (k % 2)
        um[s] = urows + 1
    meta = {"tok_off": i32(tok), "len": i32(T), "mask_pos": i32(lo), "mask_end": i32(hi), "row": i32(row),
            "urow_h": uh, "urow_m": um}
    return {"meta": meta, "s0": s0, "s1": s1, "row0": row0, "rows": rows, "urows": urows, "n_tok": o, "run": run,
            "ranges": ranges}


def unique_row(meta, s, t):
    """The unique row of position t of sequence s as SeqRows documents it: urow_m[s] + (t - lo) inside
    the sequence's span [lo, hi), else urow_h[s] + t."""
    lo, hi = int(meta["mask_pos"][s]), int(meta["mask_end"][s])
    return int(meta["urow_m"][s]) + (t - lo) if lo <= t < hi else int(meta["urow_h"][s]) + t


def unique_map(ch):
    """urow [n]: the unique row of every (s, t) of the chunk in launch_rows order, and per unique row of
    [0, urows) its (run, position, masked?) triple (-1s where no (s, t) maps to it) with the number of
    (s, t) that do."""
    m = ch["meta"]
    urow = []
    triple = -torch.ones(ch["urows"], 3, dtype=torch.long)
    count = torch.zeros(ch["urows"], dtype=torch.long)
    for s in range(ch["s0"], ch["s1"]):
        lo, hi = int(m["mask_pos"][s]), int(m["mask_end"][s])
        for t in range(int(m["len"][s])):
            u = unique_row(m, s, t)
            assert 0 <= u < ch["urows"], (s, t, u)
            tr = torch.tensor([ch["run"][s], t, int(lo <= t < hi)])
            assert count[u] == 0 or torch.equal(triple[u], tr), (s, t, u, triple[u], tr)
            triple[u], count[u] = tr, count[u] + 1
            urow.append(u)
    return torch.tensor(urow), triple, count


def unique_triples(ch):
    """The (run, position, masked?) of EVERY unique row of [0, urows) by the plan's statement (seq_plan.h:
    a run's T original rows, then one [MASK] row per position of its range), from the first sequence of
    each run: rows no (s, t) maps to are the [MASK] rows of range positions whose copies are absent."""
    m, out, seen = ch["meta"], -torch.ones(ch["urows"], 3, dtype=torch.long), set()
    for s in range(ch["s0"], ch["s1"]):
        k = ch["run"][s]
        if k in seen:
            continue
        seen.add(k)
        uh, T = int(m["urow_h"][s]), int(m["len"][s])
        rlo, rhi = ch["ranges"][k]
        for t in range(T):
            out[uh + t] = torch.tensor([k, t, 0])
        for p in range(rlo, rhi):
            out[uh + T + (p - rlo)] = torch.tensor([k, p, 1])
    return out


def triple_layout(ch):
    """A form-0 layout holding every (run, position, masked?) once: per run an unmasked copy and a copy
    whose span is the run's whole range.  -> layout, and row_of(triples) -> its rows."""
    m, T, tok, lo, hi, row, base = ch["meta"], [], [], [], [], [], {}
    r = 1
    for s in range(ch["s0"], ch["s1"]):
        k = ch["run"][s]
        if (k, 0) in base:
            continue
        for masked, (a, b) in ((0, (-1, -1)), (1, ch["ranges"][k])):
            T.append(int(m["len"][s])); tok.append(int(m["tok_off"][s])); lo.append(a); hi.append(b); row.append(r)
            base[(k, masked)] = r
            r += int(m["len"][s]) + 1
    meta = {"tok_off": i32(tok), "len": i32(T), "mask_pos": i32(lo), "mask_end": i32(hi), "row": i32(row)}
    lay = {"meta": meta, "s0": 0, "s1": len(T), "row0": 0, "rows": r + 2, "n_tok": ch["n_tok"]}
    return lay, lambda tr: torch.tensor([base[(int(k), int(msk))] + int(t) for k, t, msk in tr])


# ---- embedding operands and references ---------------------------------------------------------------

def embed_tables(family, H, seed=0, device="cpu"):
    """word [VOCAB, H], pos [MAX_POS, H], typetab [TYPE_VOCAB, H] ~ randn ("offset": word + 30, row mean
    much larger than the row's spread), g / b the distinct ramps of tail_ref.distinct_affine."""
    assert family in ("plain", "offset"), family
    from tail_ref import distinct_affine
    gen = torch.Generator().manual_seed(seed + 11)
    word, pos, typ = (torch.randn(n, H, generator=gen) for n in (VOCAB, MAX_POS, TYPE_VOCAB))
    if family == "offset":
        word = word + 30.0
    g, b = distinct_affine(H)
    return {k: v.contiguous().to(device) for k, v in (("word", word), ("pos", pos), ("typetab", typ), ("g", g), ("b", b))}


def embed_tokens(n_tok, seed=0):
    """tok / type [n_tok]: ids in [0, VOCAB) with -5 and VOCAB + 7 at every 7th / 11th token (they clamp
    to rows 0 and VOCAB - 1); types 0 / 1 in blocks of three tokens with -1 and TYPE_VOCAB + 3 at every
    5th / 13th (they clamp to 0 and TYPE_VOCAB - 1).  No id equals MASK_ID."""
    gen = torch.Generator().manual_seed(seed + 3)
    tok = torch.randint(0, VOCAB - 1, (n_tok,), generator=gen)
    tok = torch.where(tok >= MASK_ID, tok + 1, tok)
    tok[3::7], tok[5::11] = -5, VOCAB + 7
    typ = (torch.arange(n_tok) // 3) % 2
    typ[2::5], typ[4::13] = -1, TYPE_VOCAB + 3
    return tok.to(torch.int32), typ.to(torch.int32)


def embed_sum(tok, typ, meta, s0, s1, tab, dtype=torch.float32):
    """(word[id] + type[ty]) + pos[t] in ``dtype`` for every row of sequences [s0, s1) (launch_rows
    order): id = MASK_ID inside [mask_pos, mask_end), else the token, clamped to [0, VOCAB); ty = the
    type at the position ([MASK] rows included), clamped, or row 0 without types."""
    ids, tys, ts = [], [], []
    for s in range(s0, s1):
        T, o, lo, hi = (int(meta[k][s]) for k in ("len", "tok_off", "mask_pos", "mask_end"))
        t = torch.arange(T)
        raw = tok[o:o + T].long()
        ids.append(torch.where((t >= lo) & (t < hi), torch.full_like(raw, MASK_ID), raw).clamp(0, VOCAB - 1))
        tys.append(typ[o:o + T].long().clamp(0, TYPE_VOCAB - 1) if typ is not None else torch.zeros(T, dtype=torch.long))
        ts.append(t)
    dev = tab["word"].device
    ids, tys, ts = (torch.cat(v).to(dev) for v in (ids, tys, ts))
    return (tab["word"][ids].to(dtype) + tab["typetab"][tys].to(dtype)) + tab["pos"][ts].to(dtype)


def row_stats_in(x, dtype, eps=LN_EPS):
    """(mean, 1 / sqrt(var + eps)) per row evaluated in ``dtype`` (two passes, biased variance)."""
    x = x.to(dtype)
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    return mean, 1.0 / torch.sqrt(var + eps)


# ---- attention on materialised rows ------------------------------------------------------------------

def attn_rows_ref(qkv, T, row, H, heads, dtype):
    """softmax(Q K^T / 8) V per (sequence, head) in ``dtype`` on qkv [rows, 3H]: a list of [T, H], one per
    sequence of (T, row)."""
    out = []
    for r0, t in zip([int(v) for v in row], [int(v) for v in T]):
        x = qkv[r0:r0 + t].to(dtype).view(t, 3, heads, 64)
        q, k, v = x[:, 0].transpose(0, 1), x[:, 1].transpose(0, 1), x[:, 2].transpose(0, 1)
        p = torch.softmax(q @ k.transpose(1, 2) * 0.125, dim=-1)
        out.append((p @ v).transpose(0, 1).reshape(t, H))
    return out


def unique_qkv(family, ch, H, alloc, seed=0, device="cpu"):
    """qkv_u [alloc, 3H] fp32 with contents of its own on every row (the rows past urows included).
    flat: 0.6 randn.  peaked (test_gpu_attention._peaked on unique rows): Q, K ~ 3 randn, V ~ 0.6 randn,
    and per run the component 2.5 u (u = +-1 per dimension) added to the Q of every row of the run and to
    the K of one planted position j — of its original row and, where j lies in the run's range, of its
    [MASK] row — so every copy sees +50 on the logit of key j; j lies in the last 64-key block."""
    assert family in ("flat", "peaked"), family
    gen = torch.Generator().manual_seed(seed + 23)
    scale = (3.0, 3.0, 0.6) if family == "peaked" else (0.6, 0.6, 0.6)
    qkv = torch.randn(alloc, 3, H, generator=gen) * torch.tensor(scale).view(1, 3, 1)
    if family == "peaked":
        m, seen = ch["meta"], set()
        for s in range(ch["s0"], ch["s1"]):
            k = ch["run"][s]
            if k in seen:
                continue
            seen.add(k)
            uh, T = int(m["urow_h"][s]), int(m["len"][s])
            rlo, rhi = ch["ranges"][k]
            u = 2.5 * (torch.randint(0, 2, (H,), generator=gen).float() * 2 - 1)
            j = 64 * ((T - 1) // 64) + (T - 1 - 64 * ((T - 1) // 64)) // 2
            qkv[uh:uh + T + (rhi - rlo), 0] += u
            qkv[uh + j, 1] += u
            if rlo <= j < rhi:
                qkv[uh + T + (j - rlo), 1] += u
    return qkv.view(alloc, 3 * H).contiguous().to(device)


# ---- query lists of the multi-query attention --------------------------------------------------------

def mquery_lists(layout):
    """Query lists for tail_ref.attn_layout's twelve sequences (T = 5, 5 | 1, 2, 3, 63, 64, 65, 128, 129, 512 |
    7): 1, 2, 3, 4, 5, 8 and 9 positions per launched sequence (so waves idle in the last round of four),
    with 0 and T - 1 and adjacent positions; the leading sequences have lists too, so q0 = first[s0] != 0.
    -> first [n_seq + 1], seq, pos (int32 tensors)."""
    T = [int(t) for t in layout[0]]
    lists = [(1, 3), (0, 2, 4), (0,), (0, 1), (0, 1, 2), (0, 20, 21, 62), (0, 1, 31, 32, 63),
             (0, 1, 2, 32, 33, 62, 63, 64), (0, 1, 63, 64, 65, 100, 125, 126, 127), (128,),
             (0, 1, 63, 64, 255, 256, 300, 510, 511), (2, 6)]
    assert len(lists) == len(T)
    first, seq, pos = [0], [], []
    for s, ql in enumerate(lists):
        assert all(0 <= p < T[s] for p in ql) and list(ql) == sorted(set(ql)), (s, ql)
        seq += [s] * len(ql)
        pos += list(ql)
        first.append(len(pos))
    return i32(first), i32(seq), i32(pos)


def rank_queries(first, pos, r):
    """query [n_seq]: every sequence's r-th list position (its last where the list is shorter)."""
    return i32(int(pos[int(first[s]) + min(r, int(first[s + 1]) - int(first[s]) - 1)]) for s in range(len(first) - 1))


# ---- heads -------------------------------------------------------------------------------------------

def segsum_ref(row_lp, off):
    """Per segment the float64 sum of float32 row_lp[off[h] .. off[h + 1]) accumulated in row order
    (numpy's cumsum is sequential; np.sum would be pairwise).  An empty segment gives 0.0."""
    x = np.asarray(row_lp, np.float32).astype(np.float64)
    out = np.zeros(len(off) - 1, np.float64)
    for h in range(len(off) - 1):
        a, b = int(off[h]), int(off[h + 1])
        if b > a:
            out[h] = np.cumsum(x[a:b])[-1]
    return out
