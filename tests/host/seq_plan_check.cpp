// Host check of the scoring calls' plan (csrc/seq_plan.h): built with -fsanitize=address,undefined
// by tests/test_seq_plan_host.py and run as its own process, no GPU.  It builds the sequence lists
// of rs_pll_score and of rs_pll_score_spans (original / word_l2r / whole_word rows and free-form
// rows) over seeded hypotheses, cuts them at 512 and 65536 rows, plans the layer-0 unique rows
// of every chunk and restates the two device sides of the plan on the host:
//   writers  embed_unique_kernel, through the shared unique_rows_owned: every unique row of a
//            dedup chunk has exactly one writer, and a block writes at most 2T rows;
//   readers  SeqRows<., true> / embed_ln: position t of sequence s reads row
//            (lo <= t < hi ? urow_m + (t - lo) : urow_h + t), which must be < urows and must hold
//            what the reader expects (the hypothesis, the position, masked or not).
// The unique rows padded to the GEMM row alignment fit the reserved rows, or the chunk is marked
// non-dedup (170 one-word hypotheses at 512 rows have 680 unique rows).  rs_pll_score's list gets
// the numbering of the single-position plan this one replaced (literal copy below).
// Exit 0 and "seq plan ok" = no finding.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../asr-rescoring_amd/csrc/seq_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (g_fail < 20) {                            \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
            ++g_fail;                                     \
        }                                                 \
    } while (0)

static const int ALIGN = 256;   // gemm_row_align()

// The plan before spans (one masked position per sequence), copied literally.
static int parent_plan_unique_rows(std::vector<int>& urow_h, std::vector<int>& urow_m, const SeqList& sl, int s0, int s1) {
    int u = 0, base = 0;
    for (int s = s0; s < s1; ++s) {
        if (sl.mask[s] < 0) return 0;
        if (s == s0 || sl.tok_off[s] != sl.tok_off[s - 1] || sl.len[s] != sl.len[s - 1]) {
            base = u;
            u += sl.len[s];
        }
        urow_h[s] = base;
        urow_m[s] = u++;
    }
    return u;
}

struct Hyps {
    std::vector<int> off;                 // [n + 1]
    std::vector<unsigned char> ws;        // per token: 1 where a word begins
};

static Hyps make_hyps(const std::vector<int>& L, std::mt19937& rng, int max_word) {
    Hyps h;
    h.off.push_back(0);
    for (int l : L) {
        h.ws.push_back(1);                // [CLS]
        for (int p = 1; p <= l;) {
            int w = 1 + (int)(rng() % (unsigned)max_word);
            if (max_word > 510) w = l;    // one word: the whole hypothesis
            for (int k = 0; k < w && p <= l; ++k, ++p) h.ws.push_back(k == 0);
        }
        h.ws.push_back(1);                // [SEP]
        h.off.push_back((int)h.ws.size());
    }
    return h;
}

enum Form { PLL, ORIGINAL, WORD_L2R, WHOLE_WORD, FREE };

static void build(const Hyps& hy, Form f, std::mt19937& rng, SeqList* sl) {
    const int n = (int)hy.off.size() - 1;
    for (int h = 0; h < n; ++h) {
        const int o = hy.off[h], T = hy.off[h + 1] - o, L = T - 2;
        auto wbeg = [&](int p) { while (p > 1 && !hy.ws[o + p]) --p; return p; };
        auto wend = [&](int p) { ++p; while (p < T - 1 && !hy.ws[o + p]) ++p; return p; };
        if (f == FREE) {
            const int kind = h % 5;
            if (kind == 0) continue;                                              // no rows
            if (kind == 1) for (int p = L; p >= 1; --p) sl->push(o, T, wbeg(p), wend(p), p, -1);   // descending
            if (kind == 2) for (int p = 1; p <= L; ++p) for (int k = 0; k < 2; ++k) sl->push(o, T, p, wend(p), p, -1);
            if (kind == 3) for (int p = std::max(1, L - 4); p <= L; ++p) sl->push(o, T, p, p + 1, p, -1);   // a tail
            if (kind == 4) {                                                      // whole span + strided
                sl->push(o, T, 1, T - 1, 1 + L / 2, -1);
                for (int p = 1; p <= L; p += 3) sl->push(o, T, p, std::min(p + 1 + (int)(rng() % 4), T - 1), p, -1);
            }
            continue;
        }
        for (int p = 1; p <= L; ++p) {
            const int lo = f == WHOLE_WORD ? wbeg(p) : p;
            const int hi = f == PLL || f == ORIGINAL ? p + 1 : wend(p);
            sl->push(o, T, lo, hi, p, -1);
        }
    }
    for (size_t s = 0; s < sl->size(); ++s)
        CHECK(span_ok(sl->len[s], sl->mask[s], sl->mask_end[s], sl->query[s]), "span of sequence %zu", s);
}

// One unique row as its writer made it / as a reader expects it.
struct RowDesc {
    int tok_off = -1, pos = -1, masked = -1, writers = 0;
};

static void check_list(const char* name, const SeqList& in, long long cap, bool is_pll, bool expect_fallback) {
    SeqList sl = in;
    std::vector<Chunk> chunks;
    cut_rows(sl, cap, (int)(cap / 3) + 1, &chunks);
    int n_dedup = 0, n_plain = 0;
    for (Chunk& c : chunks) {
        CHECK(c.rows <= cap, "%s: chunk of %d rows > cap", name, c.rows);
        const int u = plan_unique_rows(sl, c.s0, c.s1);
        CHECK(u > 0, "%s: masked sequences gave no plan", name);
        c.urows = unique_rows_fit(u, ALIGN, cap);
        CHECK(c.urows == 0 || pad_to(c.urows, ALIGN) <= cap, "%s: %d unique rows pad past %lld", name, c.urows, cap);
        CHECK(c.urows == u || (c.urows == 0 && pad_to(u, ALIGN) > cap), "%s: fallback without need (%d)", name, u);
        if (is_pll) {
            std::vector<int> ph(sl.size(), 0), pm(sl.size(), 0);
            const int pu = parent_plan_unique_rows(ph, pm, sl, c.s0, c.s1);
            CHECK(pu == u, "%s: %d unique rows, single-position plan %d", name, u, pu);
            for (int s = c.s0; s < c.s1; ++s)
                CHECK(ph[s] == sl.urow_h[s] && pm[s] == sl.urow_m[s], "%s: numbering of sequence %d: (%d, %d) vs (%d, %d)",
                      name, s, sl.urow_h[s], sl.urow_m[s], ph[s], pm[s]);
        }
        if (!c.urows) {
            ++n_plain;
            continue;
        }
        ++n_dedup;
        // writers: the embed_unique launch of the chunk, one block per sequence
        std::vector<RowDesc> rows((size_t)c.urows);
        for (int s = c.s0; s < c.s1; ++s) {
            const bool first = s == c.s0, last = s == c.s1 - 1;
            const int T = sl.len[s];
            const UniqueOwn w = unique_rows_owned(first, last, first ? 0 : sl.urow_h[s - 1], sl.urow_h[s],
                                                  last ? 0 : sl.urow_h[s + 1], sl.urow_m[s], T, sl.mask[s], c.urows);
            CHECK(w.n_orig + w.n_mask <= 2 * T, "%s: block %d writes %d rows, T = %d", name, s, w.n_orig + w.n_mask, T);
            for (int k = 0; k < w.n_orig + w.n_mask; ++k) {
                const bool masked = k >= w.n_orig;
                const int j = k - w.n_orig, t = masked ? w.mask_pos + j : k;
                const long long r = masked ? (long long)w.mask_row + j : (long long)sl.urow_h[s] + k;
                CHECK(r >= 0 && r < c.urows, "%s: block %d writes row %lld of %d", name, s, r, c.urows);
                CHECK(t >= 0 && t < T && (!masked || (t >= 1 && t < T - 1)), "%s: block %d writes position %d", name, s, t);
                if (r < 0 || r >= c.urows) continue;
                RowDesc& d = rows[(size_t)r];
                d.tok_off = sl.tok_off[s]; d.pos = t; d.masked = masked; ++d.writers;
            }
        }
        for (int r = 0; r < c.urows; ++r)
            CHECK(rows[(size_t)r].writers == 1, "%s: unique row %d has %d writers", name, r, rows[(size_t)r].writers);
        // readers: every position of every sequence
        for (int s = c.s0; s < c.s1; ++s) {
            const int lo = sl.mask[s], n = sl.mask_end[s] - lo;
            for (int t = 0; t < sl.len[s]; ++t) {
                const bool in = (unsigned)(t - lo) < (unsigned)n;
                const long long r = in ? (long long)sl.urow_m[s] - lo + t : (long long)sl.urow_h[s] + t;
                CHECK(r >= 0 && r < c.urows, "%s: sequence %d position %d reads row %lld of %d", name, s, t, r, c.urows);
                if (r < 0 || r >= c.urows) continue;
                const RowDesc& d = rows[(size_t)r];
                CHECK(d.tok_off == sl.tok_off[s] && d.pos == t && d.masked == (int)in,
                      "%s: sequence %d position %d reads row %lld = (%d, %d, %d)", name, s, t, r, d.tok_off, d.pos, d.masked);
            }
        }
    }
    if (expect_fallback) CHECK(n_plain > 0, "%s at %lld: no chunk fell back", name, cap);
    else CHECK(n_dedup > 0, "%s at %lld: no chunk kept the dedup", name, cap);
    std::printf("%-28s cap %6lld: %3zu chunks, %d dedup, %d plain\n", name, cap, chunks.size(), n_dedup, n_plain);
}

int main() {
    std::mt19937 rng(20231);
    // lengths: one word, around the attention tiles, a chunk and more, the longest (T = 512)
    std::vector<int> L = {1, 1, 2, 3, 14, 15, 16, 17, 18, 31, 33, 46, 47, 62, 63, 130, 510, 1, 255, 509, 510, 7};
    for (int i = 0; i < 40; ++i) L.push_back(1 + (int)(rng() % 60));
    const Hyps words = make_hyps(L, rng, 5), single = make_hyps(L, rng, 1), whole = make_hyps(L, rng, 1 << 20);
    const long long caps[2] = {512, 65536};
    const char* fname[5] = {"pll", "original", "word_l2r", "whole_word", "free"};
    for (long long cap : caps) {
        for (int f = PLL; f <= FREE; ++f) {
            int k = 0;
            for (const Hyps* hy : {&words, &single, &whole}) {
                SeqList sl;
                build(*hy, (Form)f, rng, &sl);
                const std::string name = std::string(fname[f]) + (k == 0 ? "/words" : k == 1 ? "/one-token" : "/one-word");
                check_list(name.c_str(), sl, cap, f == PLL || f == ORIGINAL, false);
                ++k;
            }
        }
    }
    // 170 hypotheses of one word: 510 token rows, 680 unique rows.  At 512 reserved rows the chunk
    // must run without dedup; at 65536 it keeps it.
    {
        const Hyps hy = make_hyps(std::vector<int>(170, 1), rng, 1);
        SeqList sl;
        build(hy, PLL, rng, &sl);
        SeqList probe = sl;
        CHECK(plan_unique_rows(probe, 0, (int)probe.size()) == 680, "170 x (L = 1): unique rows");
        check_list("170 x (L = 1)", sl, 512, true, true);
        check_list("170 x (L = 1)", sl, 65536, true, false);
    }
    // one copy with a wide span: T + w unique rows
    {
        SeqList sl;
        sl.push(0, 512, 1, 511, 200, -1);
        check_list("one copy, span [1, T - 1)", sl, 512, false, true);
        check_list("one copy, span [1, T - 1)", sl, 65536, false, false);
    }
    // span validation
    CHECK(span_ok(5, 1, 4, 3) && span_ok(3, 1, 2, 1), "valid spans");
    CHECK(!span_ok(5, 0, 2, 1) && !span_ok(5, 1, 5, 2) && !span_ok(5, 2, 4, 1) && !span_ok(5, 2, 3, 3) &&
              !span_ok(5, 3, 3, 3) && !span_ok(2, 1, 2, 1),
          "invalid spans");
    if (g_fail) {
        std::printf("%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("seq plan ok\n");
    return 0;
}
