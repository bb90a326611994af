// Host check of the query-list plan of the multi-mask calls (csrc/seq_plan.h: QueryList,
// positions_ok, cut_rows_queries): built with -fsanitize=address,undefined by
// tests/test_multimask_plan.py and run as its own process, no GPU.  It builds the sequence and
// query lists of rs_pll_score_sets for strided and seeded free plans, cuts them under several
// (cap, s_cap) pairs and checks every cut:
//   no chunk exceeds cap rows, s_cap sequences or s_cap queries (the per-query workspace);
//   the chunks partition the sequences, and with them the queries, in order;
//   sl.row restarts at 0 in every chunk and max_len is the chunk's longest sequence;
//   a cut that could hold one more sequence was not cut early (the cutter is greedy);
//   a row with more than s_cap queries is reported by its index.
// Exit 0 and "multimask plan ok" = no finding.
#include <cstdio>
#include <cstdlib>
#include <random>
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

// rows of data.pll_strided: hypothesis of L words, row j masks 1 + j, 1 + j + stride, ...
static void push_strided(SeqList& sl, QueryList& ql, int tok_off, int L, int stride) {
    const int n_rows = stride < L ? stride : L;
    for (int j = 0; j < n_rows; ++j) {
        std::vector<int> p;
        for (int t = 1 + j; t <= L; t += stride) p.push_back(t);
        CHECK(positions_ok(p.data(), (int)p.size(), 1, L), "strided row not valid (L %d stride %d row %d)", L, stride, j);
        sl.push(tok_off, L + 2, -1, -1, 0, -1);
        ql.push(p.data(), (int)p.size(), -1);
    }
}

// a seeded subset of n of the positions 1..L, ascending
static void push_random(SeqList& sl, QueryList& ql, int tok_off, int L, int n, std::mt19937& rng) {
    std::vector<int> all(L), p;
    for (int i = 0; i < L; ++i) all[i] = i + 1;
    for (int i = 0; i < n; ++i) {
        std::uniform_int_distribution<int> d(i, L - 1);
        std::swap(all[i], all[d(rng)]);
    }
    p.assign(all.begin(), all.begin() + n);
    std::sort(p.begin(), p.end());
    CHECK(positions_ok(p.data(), n, 1, L), "random row not valid");
    sl.push(tok_off, L + 2, -1, -1, 0, -1);
    ql.push(p.data(), n, -1);
}

static void check_cut(SeqList& sl, const QueryList& ql, long long cap, int s_cap, const char* what) {
    std::vector<Chunk> chunks;
    const int bad = cut_rows_queries(sl, ql, cap, s_cap, &chunks);
    CHECK(bad == -1, "%s: cap %lld s_cap %d reports row %d", what, cap, s_cap, bad);
    if (bad != -1) return;
    const int S = (int)sl.size();
    CHECK(ql.first.size() == (size_t)S + 1, "%s: first has %zu entries for %d sequences", what, ql.first.size(), S);
    CHECK((S == 0) == chunks.empty(), "%s: %zu chunks for %d sequences", what, chunks.size(), S);
    int s_next = 0, q_next = 0;
    for (size_t k = 0; k < chunks.size(); ++k) {
        const Chunk& c = chunks[k];
        CHECK(c.s0 == s_next && c.s1 > c.s0 && c.s1 <= S, "%s: chunk %zu is [%d, %d), expected start %d", what, k, c.s0, c.s1, s_next);
        CHECK(c.q0 == q_next && c.q0 == ql.first[c.s0], "%s: chunk %zu starts at query %d, expected %d", what, k, c.q0, q_next);
        CHECK(c.nq == ql.first[c.s1] - ql.first[c.s0], "%s: chunk %zu holds %d queries", what, k, c.nq);
        CHECK(c.rows <= cap, "%s: chunk %zu has %d rows > cap %lld", what, k, c.rows, cap);
        CHECK(c.s1 - c.s0 <= s_cap, "%s: chunk %zu has %d sequences > %d", what, k, c.s1 - c.s0, s_cap);
        CHECK(c.nq <= s_cap && c.nq >= c.s1 - c.s0, "%s: chunk %zu has %d queries (s_cap %d, %d sequences)", what, k, c.nq, s_cap, c.s1 - c.s0);
        CHECK(c.urows == 0, "%s: chunk %zu plans dedup", what, k);
        int rows = 0, max_len = 0;
        for (int s = c.s0; s < c.s1; ++s) {
            CHECK(sl.row[s] == rows, "%s: sequence %d starts at row %d, expected %d", what, s, sl.row[s], rows);
            rows += sl.len[s];
            max_len = std::max(max_len, sl.len[s]);
        }
        CHECK(rows == c.rows && max_len == c.max_len, "%s: chunk %zu rows %d / %d, max_len %d / %d", what, k, c.rows, rows, c.max_len, max_len);
        if (c.s1 < S)       // greedy: the next sequence did not fit
            CHECK(c.rows + sl.len[c.s1] > cap || c.s1 - c.s0 >= s_cap || c.nq + ql.count(c.s1) > s_cap,
                  "%s: chunk %zu was cut before it was full", what, k);
        s_next = c.s1;
        q_next = c.q0 + c.nq;
    }
    CHECK(s_next == S && q_next == (int)ql.size(), "%s: the chunks end at sequence %d / %d, query %d / %zu", what, s_next, S, q_next, ql.size());
}

int main() {
    std::mt19937 rng(20240607);
    // positions_ok
    {
        const int a[] = {1, 2, 5}, d[] = {2, 1}, r[] = {3, 3}, z[] = {0, 1}, e[] = {4};
        CHECK(positions_ok(a, 3, 1, 5), "ascending positions refused");
        CHECK(!positions_ok(a, 3, 1, 4), "position past the end accepted");
        CHECK(!positions_ok(d, 2, 1, 5), "descending positions accepted");
        CHECK(!positions_ok(r, 2, 1, 5), "repeated position accepted");
        CHECK(!positions_ok(z, 2, 1, 5), "position 0 accepted");
        CHECK(positions_ok(z, 2, 0, 5), "position 0 refused where allowed");
        CHECK(!positions_ok(e, 0, 1, 5), "empty row accepted");
        CHECK(!positions_ok(e, 1, 1, 2), "position in an empty range accepted");
    }
    // strided plans over mixed lengths, every cap
    const int lens[] = {1, 2, 14, 15, 16, 17, 18, 31, 33, 46, 47, 62, 63, 130};
    for (int stride : {1, 2, 3, 4, 16, 200}) {
        SeqList sl;
        QueryList ql;
        int to = 0;
        for (int rep = 0; rep < 3; ++rep)
            for (int L : lens) {
                push_strided(sl, ql, to, L, stride);
                to += L + 2;
            }
        for (long long cap : {512LL, 1024LL, 65536LL})
            for (int s_cap : {(int)(cap / 3) + 1, 131, 140})
                check_cut(sl, ql, cap, s_cap, "strided");
    }
    // a 512-row plan (s_cap = 512 / 3 + 1 = 171) of rows with 130 queries each: one such row and
    // 41 more queries fit a chunk, never two such rows
    {
        SeqList sl;
        QueryList ql;
        for (int i = 0; i < 12; ++i) {
            push_random(sl, ql, i * 132, 130, 130, rng);
            if (i % 3 == 1) push_random(sl, ql, i * 132, 130, 41, rng);
            if (i % 3 == 2) push_random(sl, ql, i * 132, 130, 42, rng);
        }
        check_cut(sl, ql, 512, 171, "130-query rows");
        std::vector<Chunk> chunks;
        CHECK(cut_rows_queries(sl, ql, 512, 171, &chunks) == -1, "130-query rows refused");
        for (const Chunk& c : chunks) {
            int big = 0;
            for (int s = c.s0; s < c.s1; ++s) big += ql.count(s) == 130;
            CHECK(big <= 1, "two 130-query rows in one chunk of 171");
        }
        // the same list under a roomy cap: the query cap alone cuts it
        check_cut(sl, ql, 65536, 171, "130-query rows, query cap only");
        check_cut(sl, ql, 65536, 21846, "130-query rows, one chunk");
    }
    // seeded free plans
    for (int it = 0; it < 50; ++it) {
        SeqList sl;
        QueryList ql;
        int to = 0;
        const int n_seq = 1 + (int)(rng() % 300);
        for (int s = 0; s < n_seq; ++s) {
            const int L = 1 + (int)(rng() % 140), n = 1 + (int)(rng() % L);
            push_random(sl, ql, to, L, n, rng);
            if (rng() % 4 == 0) to += L + 2;
        }
        const long long cap = 512 + (long long)(rng() % 4096);
        check_cut(sl, ql, cap, (int)(cap / 3) + 1, "free");
    }
    // an empty list
    {
        SeqList sl;
        QueryList ql;
        check_cut(sl, ql, 512, 171, "empty");
    }
    // a row with more than s_cap queries is reported by its index
    {
        SeqList sl;
        QueryList ql;
        push_random(sl, ql, 0, 200, 171, rng);
        push_random(sl, ql, 0, 200, 5, rng);
        push_random(sl, ql, 0, 200, 172, rng);
        push_random(sl, ql, 0, 200, 1, rng);
        std::vector<Chunk> chunks;
        const int bad = cut_rows_queries(sl, ql, 512, 171, &chunks);
        CHECK(bad == 2, "the 172-query row was reported as %d", bad);
        chunks.clear();
        CHECK(cut_rows_queries(sl, ql, 65536, 172, &chunks) == -1, "172 queries refused at s_cap 172");
    }
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("multimask plan ok\n");
    return 0;
}
