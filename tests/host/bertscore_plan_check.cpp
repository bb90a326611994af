// Host check of the BERTScore recall plan (csrc/bertscore_plan.h: bertscore_layout_error,
// plan_bertscore_items, the packed upload): built with -fsanitize=address,undefined by
// tests/test_bertscore_plan.py and run as its own process, no GPU.  Over edge and seeded random
// layouts, for COLS = 64 and 32, every plan is checked:
//   the items of an utterance are ordered, do not overlap and cover every ref hypothesis once;
//   a multi-hypothesis item spans <= COLS columns, a hypothesis of > COLS columns is alone;
//   the cut is greedy (the next hypothesis did not fit an item that ended before it);
//   moff is the running sum of n^2;
//   the packed upload holds the four sections at their offsets, mat_off 8-byte and items 16-byte
//   aligned, and the offsets and the size are the ones the entry point used before the move.
// Exit 0 and "bertscore plan ok" = no finding.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../asr-rescoring_amd/csrc/bertscore_plan.h"

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

// utts: the hypothesis lengths of every utterance
static void check_plan(const std::vector<std::vector<int>>& utts, int cols, const char* what) {
    std::vector<int> hyp_off{0}, utt_off{0};
    for (const auto& u : utts) {
        for (int T : u) hyp_off.push_back(hyp_off.back() + T);
        utt_off.push_back((int)hyp_off.size() - 1);
    }
    const int n_utt = (int)utts.size(), n_hyp = utt_off.back();
    CHECK(bertscore_layout_error(hyp_off.data(), utt_off.data(), n_utt).empty(), "%s: layout refused", what);
    BertscorePlan plan;
    plan.items.assign(7, -5);            // stale contents must not survive
    plan.moff.assign(3, 99);
    plan_bertscore_items(hyp_off.data(), utt_off.data(), n_utt, cols, &plan);
    CHECK(plan.items.size() % 4 == 0, "%s: %zu item words", what, plan.items.size());
    CHECK(plan.moff.size() == (size_t)n_utt + 1 && plan.moff[0] == 0, "%s: moff has %zu entries", what, plan.moff.size());
    long long mo = 0;
    for (int u = 0; u < n_utt; ++u) {
        const long long n = (long long)utts[u].size();
        mo += n * n;
        CHECK(plan.moff[u + 1] == mo, "%s: moff[%d] = %lld, expected %lld", what, u + 1, plan.moff[u + 1], mo);
    }
    std::vector<int> seen(n_hyp, 0);
    int u_prev = 0, j_next = 0;
    for (int k = 0; k < plan.n_items(); ++k) {
        const int u = plan.items[4 * k], j0 = plan.items[4 * k + 1], j1 = plan.items[4 * k + 2];
        CHECK(plan.items[4 * k + 3] == 0, "%s: item %d word 3 = %d", what, k, plan.items[4 * k + 3]);
        CHECK(u >= 0 && u < n_utt, "%s: item %d names utterance %d", what, k, u);
        if (u < 0 || u >= n_utt) return;
        const int h0 = utt_off[u], n = utt_off[u + 1] - h0;
        if (u != u_prev) {
            CHECK(u > u_prev, "%s: item %d goes back to utterance %d", what, k, u);
            // the utterances in between had every hypothesis planned (or none to plan)
            CHECK(j_next == utt_off[u_prev + 1] - utt_off[u_prev], "%s: utterance %d ends at hypothesis %d", what, u_prev, j_next);
            for (int v = u_prev + 1; v < u; ++v)
                CHECK(utt_off[v + 1] == utt_off[v], "%s: utterance %d has no item", what, v);
            u_prev = u;
            j_next = 0;
        }
        CHECK(j0 == j_next && j1 > j0 && j1 <= n, "%s: item %d is [%d, %d) of %d, expected start %d", what, k, j0, j1, n, j_next);
        if (!(j0 >= 0 && j1 > j0 && j1 <= n)) return;
        const int c = hyp_off[h0 + j1] - hyp_off[h0 + j0];
        if (j1 - j0 > 1) CHECK(c <= cols, "%s: item %d holds %d hypotheses over %d > %d columns", what, k, j1 - j0, c, cols);
        for (int j = j0; j < j1; ++j) {
            ++seen[h0 + j];
            if (hyp_off[h0 + j + 1] - hyp_off[h0 + j] > cols)
                CHECK(j1 - j0 == 1, "%s: hypothesis %d of %d columns shares item %d", what, j, hyp_off[h0 + j + 1] - hyp_off[h0 + j], k);
        }
        if (j1 < n)      // greedy: the next hypothesis did not fit
            CHECK(c > cols || c + hyp_off[h0 + j1 + 1] - hyp_off[h0 + j1] > cols, "%s: item %d was cut before it was full", what, k);
        j_next = j1;
    }
    if (n_hyp > 0) {
        CHECK(plan.n_items() > 0, "%s: no item for %d hypotheses", what, n_hyp);
        CHECK(j_next == utt_off[u_prev + 1] - utt_off[u_prev], "%s: the last planned utterance %d ends at hypothesis %d", what, u_prev, j_next);
        for (int v = u_prev + 1; v < n_utt; ++v)
            CHECK(utt_off[v + 1] == utt_off[v], "%s: utterance %d has no item", what, v);
    } else {
        CHECK(plan.n_items() == 0, "%s: %d items for no hypothesis", what, plan.n_items());
    }
    for (int h = 0; h < n_hyp; ++h) CHECK(seen[h] == 1, "%s: hypothesis %d is in %d items", what, h, seen[h]);

    // the packed upload
    const BertscoreUpload w = bertscore_upload_layout(plan, n_hyp, n_utt);
    const size_t w_items = plan.items.size(), w_moff = 2 * (size_t)(n_utt + 1);
    CHECK(w.items == 0 && w.moff == w_items && w.hyp_off == w_items + w_moff && w.utt_off == w_items + w_moff + n_hyp + 1 &&
              w.n_int == w_items + w_moff + (size_t)(n_hyp + 1) + (size_t)(n_utt + 1),
          "%s: upload layout %zu %zu %zu %zu / %zu", what, w.items, w.moff, w.hyp_off, w.utt_off, w.n_int);
    CHECK(w.moff % 2 == 0 && w.items % 4 == 0, "%s: misaligned sections", what);
    std::vector<int> buf(w.n_int, -7);   // exactly n_int words: an overrun is the sanitizer's finding
    bertscore_upload_pack(plan, w, hyp_off.data(), utt_off.data(), n_hyp, n_utt, buf.data());
    for (size_t i = 0; i < w_items; ++i) CHECK(buf[w.items + i] == plan.items[i], "%s: packed item word %zu", what, i);
    for (int u = 0; u <= n_utt; ++u) {
        long long v;
        std::memcpy(&v, &buf[w.moff + 2 * (size_t)u], 8);
        CHECK(v == plan.moff[u], "%s: packed moff[%d]", what, u);
    }
    for (int h = 0; h <= n_hyp; ++h) CHECK(buf[w.hyp_off + h] == hyp_off[h], "%s: packed hyp_off[%d]", what, h);
    for (int u = 0; u <= n_utt; ++u) CHECK(buf[w.utt_off + u] == utt_off[u], "%s: packed utt_off[%d]", what, u);
}

int main() {
    std::mt19937 rng(20240911);
    for (int cols : {64, 32}) {
        const int C = cols;
        // every ref length at the tile edge, alone and in a run
        check_plan({{2, 3, C - 1, C, C + 1, C + 2, 2 * C, 2 * C + 1}}, cols, "edge lengths");
        check_plan({{C}, {C + 1}, {2}, {3 * C + 5}}, cols, "one hypothesis each");
        // runs summing to exactly C, to C + 1, and a long one between short ones
        check_plan({std::vector<int>(C / 2, 2), {C - 3, 3, C - 3, 4}, {2, C + 1, 2}, {C / 2, C / 2, C / 2 + 1, C / 2}}, cols, "runs");
        // empty utterances: first, between two others, last, and nothing but empty ones
        check_plan({{}, {3, 4}, {}, {}, {5}, {}}, cols, "empty utterances");
        check_plan({{}, {}}, cols, "only empty utterances");
        check_plan({}, cols, "no utterance");
        check_plan({std::vector<int>(129, 2), std::vector<int>(65, 3)}, cols, "many short hypotheses");
        for (int it = 0; it < 200; ++it) {
            std::vector<std::vector<int>> utts(rng() % 6);
            for (auto& u : utts) {
                u.resize(rng() % 40);
                for (int& T : u) {
                    const unsigned k = rng() % 8;
                    T = k == 0 ? 2 : k == 1 ? C + (int)(rng() % 3) - 1 : k == 2 ? 2 + (int)(rng() % (4 * C)) : 2 + (int)(rng() % 12);
                }
            }
            check_plan(utts, cols, "random");
        }
    }
    // the layout checks, in the order the entry points report them
    {
        const int ho[] = {0, 3, 5, 9}, uo[] = {0, 1, 3};
        CHECK(bertscore_layout_error(ho, uo, 2).empty(), "valid layout refused");
        const int uo1[] = {1, 1, 3};
        CHECK(bertscore_layout_error(ho, uo1, 2) == "utt_off[0] must be 0", "utt_off[0] = 1 accepted");
        const int uo2[] = {0, 2, 1};
        CHECK(bertscore_layout_error(ho, uo2, 2) == "utt_off not ascending", "descending utt_off accepted");
        const int ho1[] = {1, 3, 5, 9};
        CHECK(bertscore_layout_error(ho1, uo, 2) == "hyp_off[0] must be 0", "hyp_off[0] = 1 accepted");
        const int ho2[] = {0, 3, 4, 9};
        CHECK(bertscore_layout_error(ho2, uo, 2) == "hypothesis 1 has fewer than 2 tokens ([CLS] [SEP])", "one-token hypothesis accepted");
        const int ho3[] = {0, 3, 2, 9};
        CHECK(!bertscore_layout_error(ho3, uo, 2).empty(), "descending hyp_off accepted");
        // only the hypotheses the utterances name are read
        const int uo3[] = {0, 1};
        CHECK(bertscore_layout_error(ho2, uo3, 1).empty(), "a hypothesis past utt_off[n_utt] was checked");
    }
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("bertscore plan ok\n");
    return 0;
}
