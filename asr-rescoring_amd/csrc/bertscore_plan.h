// Host-side plan of one BERTScore recall launch (k_bertscore.hip): the layout checks of its entry
// points, the work items and the packed upload.  Standard library only: rs_api.hip includes it, and
// so does the stand-alone check tests/host/bertscore_plan_check.cpp, which runs without a GPU.
#pragma once
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

// hyp_off [n_hyp + 1] token offsets of the hypotheses, utt_off [n_utt + 1] hypothesis offsets of the
// utterances (n_utt >= 1).  Returns the message of the first violated rule, or an empty string.
inline std::string bertscore_layout_error(const int* hyp_off, const int* utt_off, int n_utt) {
    if (utt_off[0] != 0) return "utt_off[0] must be 0";
    const int n_hyp = utt_off[n_utt];
    for (int u = 0; u < n_utt; ++u)
        if (utt_off[u + 1] < utt_off[u]) return "utt_off not ascending";
    if (hyp_off[0] != 0) return "hyp_off[0] must be 0";
    for (int h = 0; h < n_hyp; ++h)
        if (hyp_off[h + 1] - hyp_off[h] < 2)
            return "hypothesis " + std::to_string(h) + " has fewer than 2 tokens ([CLS] [SEP])";
    return std::string();
}

// items: (utterance, j0, j1, 0) per work item = the ref hypotheses [j0, j1) of the utterance, a run
// of whole hypotheses whose tokens fit one tile of `cols` columns, or one longer hypothesis alone
// (the kernel walks it in sub-tiles).  moff [n_utt + 1]: offset of utterance u's n x n block in the
// recall matrices, the running sum of n^2.
struct BertscorePlan {
    std::vector<int> items;
    std::vector<long long> moff;
    int n_items() const { return (int)(items.size() / 4); }
};

inline void plan_bertscore_items(const int* hyp_off, const int* utt_off, int n_utt, int cols, BertscorePlan* plan) {
    plan->items.clear();
    plan->moff.assign((size_t)n_utt + 1, 0);
    for (int u = 0; u < n_utt; ++u) {
        const int h0 = utt_off[u], n = utt_off[u + 1] - h0;
        plan->moff[u + 1] = plan->moff[u] + (long long)n * n;
        for (int j = 0; j < n;) {
            int j1 = j + 1, c = hyp_off[h0 + j + 1] - hyp_off[h0 + j];
            while (c <= cols && j1 < n && c + hyp_off[h0 + j1 + 1] - hyp_off[h0 + j1] <= cols) {
                c += hyp_off[h0 + j1 + 1] - hyp_off[h0 + j1];
                ++j1;
            }
            plan->items.insert(plan->items.end(), {u, j, j1, 0});
            j = j1;
        }
    }
}

// The one upload of a launch, in int words: items | mat_off (int64) | hyp_off | utt_off.
struct BertscoreUpload {
    size_t items, moff, hyp_off, utt_off;   // word offset of each section
    size_t n_int;                           // words in all
};
inline BertscoreUpload bertscore_upload_layout(const BertscorePlan& plan, int n_hyp, int n_utt) {
    BertscoreUpload w{};
    w.items = 0;
    w.moff = plan.items.size();
    w.hyp_off = w.moff + 2 * (size_t)(n_utt + 1);
    w.utt_off = w.hyp_off + (size_t)(n_hyp + 1);
    w.n_int = w.utt_off + (size_t)(n_utt + 1);
    return w;
}
// p: w.n_int ints
inline void bertscore_upload_pack(const BertscorePlan& plan, const BertscoreUpload& w, const int* hyp_off,
                                  const int* utt_off, int n_hyp, int n_utt, int* p) {
    std::memcpy(p + w.items, plan.items.data(), plan.items.size() * 4);
    std::memcpy(p + w.moff, plan.moff.data(), (size_t)(n_utt + 1) * 8);
    std::memcpy(p + w.hyp_off, hyp_off, (size_t)(n_hyp + 1) * 4);
    std::memcpy(p + w.utt_off, utt_off, (size_t)(n_utt + 1) * 4);
}
