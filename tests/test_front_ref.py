"""CPU: the helpers of tests/front_ref.py — the dedup chunk built on the production unique-row plan
(rs_debug_plan_unique, host only) against the restatement of SeqRows' addressing, the layouts'
properties the GPU tests rely on, every reference against plain loops on tiny inputs, and the
decoders of the kx = 1 / 2 / 3 operand images."""
import math

import numpy as np
import pytest
import torch

import front_ref as F
import tail_ref as R
from x3s_image import _split2, _unsplit2, ln_ref64


# ---- the dedup layout ---------------------------------------------------------------------------------

@pytest.mark.parametrize("max_len", sorted(F.RUNS))
def test_dedup_chunk_covers_the_plan(max_len):
    ch = F.dedup_chunk(F.RUNS[max_len])
    m, s0, s1, urows = ch["meta"], ch["s0"], ch["s1"], ch["urows"]
    assert s0 == 2 and max(int(t) for t in m["len"][s0:s1]) == max_len
    # the plan's count: per run T original rows and one [MASK] row per position of its range
    assert urows == sum(t + (ch["ranges"][k][1] - ch["ranges"][k][0]) for k, (t, _) in enumerate(F.RUNS[max_len]))
    urow, triple, count = F.unique_map(ch)        # asserts: two (s, t) on one row carry one triple
    every = F.unique_triples(ch)
    assert (every >= 0).all(), "a unique row outside every run"
    hit = count > 0
    assert torch.equal(triple[hit], every[hit])
    # rows no (s, t) maps to: [MASK] rows of positions inside their run's range whose copies are absent (the
    # cut run's 8 and 9), and original rows of positions that EVERY copy of their run masks (a one-copy run's
    # span: the plan gives each run its T original rows whatever its copies read)
    absent = []
    for u in torch.nonzero(~hit)[:, 0].tolist():
        k, p, masked = (int(v) for v in every[u])
        if masked:
            assert ch["ranges"][k][0] <= p < ch["ranges"][k][1], (u, k, p)
            absent.append((k, p))
        else:
            assert all(a <= p < b for a, b in F.RUNS[max_len][k][1]), (u, k, p)
    assert [p for k, p in absent if k == 1] == [8, 9]                          # the cut run
    # the restatement, position by position, against the definition
    n = 0
    for s in range(s0, s1):
        lo, hi = int(m["mask_pos"][s]), int(m["mask_end"][s])
        for t in range(int(m["len"][s])):
            want = int(m["urow_m"][s]) + t - lo if lo <= t < hi else int(m["urow_h"][s]) + t
            assert F.unique_row(m, s, t) == want == int(urow[n])
            n += 1
    # distinct triples land on distinct rows
    assert len({tuple(v.tolist()) for v in every}) == urows
    # the poisoned sequences stay inside the over-sized buffers and outside the launch's rows
    own = set(F.launch_rows(m, s0, s1, ch["row0"])[0].tolist())
    for s in list(range(s0)) + list(range(s1, len(m["len"]))):
        T = int(m["len"][s])
        rows = set(range(int(m["row"][s]) - ch["row0"], int(m["row"][s]) - ch["row0"] + T))
        assert not rows & own and max(rows) < ch["rows"] and min(rows) >= 0
        assert urows <= int(m["urow_h"][s]) and int(m["urow_h"][s]) + T <= F.pad_to(urows, 256) + 8
        assert urows <= int(m["urow_m"][s]) and int(m["urow_m"][s]) + 3 <= F.pad_to(urows, 256) + 8


def test_dedup_chunk_has_every_run_kind():
    ch = F.dedup_chunk(F.RUNS[48])
    m, s0 = ch["meta"], ch["s0"]
    T0, pll = F.RUNS[48][0]
    assert pll == [(p, p + 1) for p in range(1, T0 - 1)]                       # PLL: ascending over 1 .. T - 2
    # one [MASK] row per copy, in copy order
    assert [int(m["urow_m"][s0 + i]) for i in range(len(pll))] == [int(m["urow_h"][s0]) + T0 + i for i in range(len(pll))]
    assert F.RUNS[48][1][1][0] == (5, 6)                                       # the cut run starts at position 5
    wide = F.RUNS[48][2][1]
    assert any(a < c < b for a, b in wide for c, _ in wide)                    # overlapping wide spans
    assert len(F.RUNS[48][3][1]) == 1 and F.RUNS[48][4][0] == 3
    lay, row_of = F.triple_layout(ch)
    rows = row_of(F.unique_triples(ch))
    assert len(set(rows.tolist())) == ch["urows"] and int(rows.max()) < lay["rows"]


def test_plan_entry_rejects_bad_arguments():
    from asr_rescoring_amd import _lib
    a = np.zeros(4, np.int32)
    P = a.ctypes.data
    lib = _lib.load()
    assert lib.rs_debug_plan_unique(None, P, P, P, 4, 0, 4, P, P) < 0
    assert lib.rs_debug_plan_unique(P, P, P, P, 4, 2, 2, P, P) < 0
    assert lib.rs_debug_plan_unique(P, P, P, P, 4, 0, 5, P, P) < 0
    # a sequence without a mask position: dedup not applicable
    uh, um, urows = F.plan_unique([0, 0], [5, 5], [1, -1], [2, -1], 0, 2)
    assert urows == 0 and (uh == -1).all()


# ---- the embedding layouts ----------------------------------------------------------------------------

def test_embed_layout_properties():
    lay = F.embed_layout()
    m, s0, s1, row0 = lay["meta"], lay["s0"], lay["s1"], lay["row0"]
    assert len(m["len"]) == 12 and (s0, s1) == (2, 11) and row0 != 0
    assert tuple(int(t) for t in m["len"][s0:s1]) == F.EMBED_LENGTHS == (1, 2, 3, 4, 5, 9, 64, 65, 130)
    rows, ss, ts = F.launch_rows(m, s0, s1, row0)
    assert len(set(rows.tolist())) == len(rows) and int(rows.min()) > 0          # disjoint, a gap before the first
    assert sorted(rows.tolist()) != list(range(int(rows.min()), int(rows.max()) + 1))   # gaps between ranges
    for s in list(range(s0)) + list(range(s1, 12)):                              # poisoned: inside the sentinel rows
        r = int(m["row"][s]) - row0
        assert r > int(rows.max()) and r + int(m["len"][s]) <= lay["rows"]
    spans = {(int(m["mask_pos"][s]), int(m["mask_end"][s]), int(m["len"][s])) for s in range(s0, s1)}
    assert any(a == -1 for a, b, t in spans) and any(b - a == 1 for a, b, t in spans)
    assert any(b - a == 3 for a, b, t in spans) and any(b == t - 1 for a, b, t in spans)
    counts = sorted({int(m["first"][s + 1] - m["first"][s]) for s in range(s0, s1)})
    assert counts == [1, 2, 3, 4, 5, 9]
    for s in range(s0, s1):
        T, ql = int(m["len"][s]), m["pos"][int(m["first"][s]):int(m["first"][s + 1])].tolist()
        assert all(0 <= p < T for p in ql) and ql == sorted(set(ql))
        assert all(int(m["seq"][q]) == s for q in range(int(m["first"][s]), int(m["first"][s + 1])))
        if T >= 9:
            assert 1 in ql or T == 130
            assert any(b - a == 1 for a, b in zip(ql, ql[1:])) or T == 130
    assert any(int(m["len"][s]) - 2 in m["pos"][int(m["first"][s]):int(m["first"][s + 1])].tolist() for s in range(s0, s1))
    tok, typ = F.embed_tokens(lay["n_tok"])
    used = torch.cat([tok[int(m["tok_off"][s]):int(m["tok_off"][s]) + int(m["len"][s])] for s in range(s0, s1)])
    usedt = torch.cat([typ[int(m["tok_off"][s]):int(m["tok_off"][s]) + int(m["len"][s])] for s in range(s0, s1)])
    assert {-5, F.VOCAB + 7} <= set(used.tolist()) and F.MASK_ID not in used.tolist()
    assert {-1, F.TYPE_VOCAB + 3, 0, 1} <= set(usedt.tolist())
    # a [MASK] position whose type is not that of position 0
    assert any(int(typ[int(m["tok_off"][s]) + int(m["mask_pos"][s])].clamp(0, 1)) != int(typ[int(m["tok_off"][s])].clamp(0, 1))
               for s in range(s0, s1) if int(m["mask_pos"][s]) >= 0)


def test_expand_queries_maps_every_row():
    lay = F.embed_layout(row0=0)
    ex, src = F.expand_queries(lay)
    m, em = lay["meta"], ex["meta"]
    rows, ss, ts = F.launch_rows(m, lay["s0"], lay["s1"], 0)
    assert len(src) == len(rows) and int(src.max()) < ex["rows"]
    erows, ess, ets = F.launch_rows(em, 0, ex["s1"], 0)
    where = {int(r): (int(s), int(t)) for r, s, t in zip(erows, ess, ets)}
    for r, s, t in zip(src.tolist(), ss.tolist(), ts.tolist()):
        es, et = where[r]
        ql = m["pos"][int(m["first"][s]):int(m["first"][s + 1])].tolist()
        assert et == t and int(em["tok_off"][es]) == int(m["tok_off"][s]) and int(em["len"][es]) == int(m["len"][s])
        span = (int(em["mask_pos"][es]), int(em["mask_end"][es]))
        assert span == ((t, t + 1) if t in ql else (-1, -1))


# ---- references against plain loops -------------------------------------------------------------------

def test_embed_sum_against_a_loop():
    lay = F.embed_layout()
    m, s0, s1 = lay["meta"], lay["s0"], lay["s1"]
    tab = F.embed_tables("plain", 256, seed=1)
    tok, typ = F.embed_tokens(lay["n_tok"], seed=1)
    for types in (typ, None):
        got = F.embed_sum(tok, types, m, s0, s1, tab)
        n = 0
        for s in range(s0, s0 + 6):
            o = int(m["tok_off"][s])
            for t in range(int(m["len"][s])):
                i = F.MASK_ID if int(m["mask_pos"][s]) <= t < int(m["mask_end"][s]) else int(tok[o + t])
                i = min(max(i, 0), F.VOCAB - 1)
                ty = min(max(int(types[o + t]), 0), F.TYPE_VOCAB - 1) if types is not None else 0
                want = (tab["word"][i] + tab["typetab"][ty]) + tab["pos"][t]
                assert torch.equal(got[n], want), (s, t)
                n += 1
    x = F.embed_sum(tok, typ, m, s0, s1, tab)
    x64 = F.embed_sum(tok, typ, m, s0, s1, tab, torch.float64)
    assert x64.dtype == torch.float64 and (x64 - x.double()).abs().max() <= 2.0 ** -22 * x64.abs().max()
    off = F.embed_tables("offset", 256, seed=1)
    xo = F.embed_sum(tok, typ, m, s0, s1, off)
    assert (xo.mean(dim=1).abs() > 10 * xo.std(dim=1)).all()                  # row mean >> row std


def test_layernorm_and_row_stats_against_loops():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 256, generator=g) * 2 + 0.5
    ga, be = R.distinct_affine(256)
    y = ln_ref64(x, ga, be, F.LN_EPS)
    mean, rstd = F.row_stats_in(x, torch.float64)
    for r in range(5):
        v = [float(e) for e in x[r]]
        mu = math.fsum(v) / 256
        var = math.fsum((e - mu) ** 2 for e in v) / 256
        assert abs(float(mean[r]) - mu) <= 1e-15 * max(1, abs(mu))
        assert abs(float(rstd[r]) - 1 / math.sqrt(var + F.LN_EPS)) <= 1e-14 / math.sqrt(var)
        for c in (0, 100, 255):
            want = (v[c] - mu) / math.sqrt(var + F.LN_EPS) * float(ga[c]) + float(be[c])
            assert abs(float(y[r, c]) - want) <= 1e-13
    m32, r32 = F.row_stats_in(x, torch.float32)
    assert m32.dtype == torch.float32 and (m32.double() - mean).abs().max() < 1e-6
    assert ((r32.double() - rstd).abs() / rstd).max() < 1e-6


def test_attn_rows_ref_against_a_loop():
    g = torch.Generator().manual_seed(4)
    T, row, H, heads = [3, 1, 5], [1, 6, 8], 128, 2
    qkv = torch.randn(14, 3 * H, generator=g)
    got = F.attn_rows_ref(qkv, T, row, H, heads, torch.float64)
    for out, t, r0 in zip(got, T, row):
        assert out.shape == (t, H)
        for h in range(heads):
            for i in range(t):
                q = qkv[r0 + i, h * 64:(h + 1) * 64].double()
                sc = [float(q @ qkv[r0 + j, H + h * 64:H + (h + 1) * 64].double()) / 8 for j in range(t)]
                mx = max(sc)
                w = [math.exp(v - mx) for v in sc]
                want = sum(wj / sum(w) * qkv[r0 + j, 2 * H + h * 64:2 * H + (h + 1) * 64].double() for j, wj in enumerate(w))
                assert (out[i, h * 64:(h + 1) * 64] - want).abs().max() < 1e-12


def test_per_query_reference_through_the_lists():
    """tail_ref.attn_query_ref per rank reproduces attention on materialised rows at every list position."""
    layout = R.attn_layout()
    T, row, query, s0, s1, rows = layout
    first, seq, pos = F.mquery_lists(layout)
    counts = sorted({int(first[s + 1] - first[s]) for s in range(s0, s1)})
    assert counts == [1, 2, 3, 4, 5, 8, 9] and int(first[s0]) != 0
    for s in range(s0, s1):
        ql = pos[int(first[s]):int(first[s + 1])].tolist()
        assert int(T[s]) > 3 and len(ql) == 1 or 0 in ql
    assert any(int(T[s]) - 1 in pos[int(first[s]):int(first[s + 1])].tolist() for s in range(s0, s1))
    H, heads = 128, 2
    qkv = torch.randn(rows, 3 * H, generator=torch.Generator().manual_seed(5)) * 0.6
    full = F.attn_rows_ref(qkv, T[s0:s1], row[s0:s1], H, heads, torch.float64)
    for r in (0, 3, 8):
        qr = F.rank_queries(first, pos, r)
        lay = (T, row, qr, s0, s1, rows)
        q = torch.stack([qkv[int(row[s]) + int(qr[s]), :H] for s in range(s0, s1)])
        got = R.attn_query_ref(qkv, q, lay, H, heads, torch.float64)
        for i, s in enumerate(range(s0, s1)):
            n = int(first[s + 1] - first[s])
            assert int(qr[s]) == int(pos[int(first[s]) + min(r, n - 1)])
            assert (got[i] - full[i][int(qr[s])]).abs().max() < 1e-12


def test_unique_qkv_families():
    ch = F.dedup_chunk(F.RUNS[130])
    alloc = F.pad_to(ch["urows"], 256) + 8
    H, heads = 128, 2
    flat = F.unique_qkv("flat", ch, H, alloc)
    assert flat.shape == (alloc, 3 * H) and len({float(v) for v in flat[:, 0]}) == alloc     # distinct rows
    pk = F.unique_qkv("peaked", ch, H, alloc)
    assert pk.half().float().abs().max() < 100
    # every copy sees one key far above the others: its softmax row is peaked on one position
    m = ch["meta"]
    urow, _, _ = F.unique_map(ch)
    rows, ss, ts = F.launch_rows(m, ch["s0"], ch["s1"], 0)
    full = torch.zeros(ch["rows"], 3 * H)
    full[rows] = pk[urow]
    for s in (ch["s0"], ch["s0"] + 14, ch["s1"] - 1):
        t, r0 = int(m["len"][s]), int(m["row"][s])
        x = full[r0:r0 + t].double().view(t, 3, heads, 64)
        sc = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) / 8
        top = sc.argmax(dim=2)
        j = 64 * ((t - 1) // 64) + (t - 1 - 64 * ((t - 1) // 64)) // 2
        assert (top == j).float().mean() > 0.9, (s, t, j)


def test_segsum_ref_is_sequential():
    x = (np.random.default_rng(6).standard_normal(700) * 10).astype(np.float32)
    off = [0, 0, 1, 3, 303, 303, 700]
    got = F.segsum_ref(x, off)
    for h in range(len(off) - 1):
        acc = 0.0
        for v in x[off[h]:off[h + 1]]:
            acc += float(v)
        assert got[h] == acc
    assert got[0] == 0.0 and got[4] == 0.0


# ---- decoders -------------------------------------------------------------------------------------------

def test_image2_decoder_and_exact_checks():
    g = torch.Generator().manual_seed(7)
    mag = torch.exp2(torch.rand(6, 256, generator=g) * 18 - 6)
    v = mag * torch.where(torch.rand(6, 256, generator=g) < 0.5, -1.0, 1.0)
    img = F.image2_of(v)
    hi, lo = F.deinterleave2(img)
    assert torch.equal(hi, v.half())                                             # hi == RNE16(v)
    assert torch.equal(lo, ((v - hi.float()) * 64.0).half())                     # lo == RNE16(64 (v - hi))
    assert torch.equal(img[:, :32], hi[:, :32]) and torch.equal(img[:, 32:64], lo[:, :32])
    assert torch.equal(img[:, 64:96], hi[:, 32:64])
    back = _unsplit2(img, torch.float64)
    assert torch.equal(back, hi.double() + lo.double() / 64)
    assert ((back - v.double()).abs() <= 2.0 ** -21 * v.double().abs()).all()
    assert F.image2_defects(img) == []
    bad = img.clone()
    bad[2, 32 + 5] = (bad[2, 5].float() * 8).half()                              # lo/64 = hi/8: hi is not the RNE
    assert any("RNE16" in m for m in F.image2_defects(bad))
    bad = img.clone()
    bad[1, 32] = float("inf")
    assert any("finite" in m for m in F.image2_defects(bad))
    planar = torch.cat([hi, lo], dim=1)                                          # the planar order is another image
    assert F.image2_defects(planar) != []
    tie = F.image2_of(torch.full((1, 64), 1.0 + 2.0 ** -10))
    tie[0, 32 + 7] = 2.0 ** -5                                                   # an exact tie: no defect
    assert F.image2_defects(tie) == []


def test_image13_decoders():
    v = torch.randn(4, 256, generator=torch.Generator().manual_seed(8))
    img3 = R._split3(v)
    assert R.image3_defects(img3) == []
    assert torch.equal(R._unsplit3(img3, torch.float64), _unsplit2(_split2(v), torch.float64))
    assert torch.equal(img3[:, :256], v.half())                                  # kx = 1 is section 0 alone
