// Host-side plan of one scoring call: the sequence list, its cut into launch chunks and the
// layer-0 unique-row plan (dedup), and the query list of the multi-mask calls with its chunk cut.
// No HIP types: rs_api.hip includes it, and so do the stand-alone checks
// tests/host/seq_plan_check.cpp and tests/host/multimask_plan_check.cpp, which run without a GPU.
//
// The one function both the host and the device use is unique_rows_owned: which unique rows the
// embed_unique block of a sequence writes.  The check restates the launch with it and counts the
// writers of every row.
#pragma once
#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define RS_PLAN_HD __host__ __device__
#else
#define RS_PLAN_HD
#endif

// Host-side sequence list (structure of arrays) for one call.  A sequence is one BERT input;
// positions [mask, mask_end) are replaced by [MASK] on the device (mask = mask_end = -1: none).
struct SeqList {
    std::vector<int> tok_off, len, mask, query, label, row, urow_h, urow_m, mask_end;
    void push(int to, int T, int lo, int hi, int q, int lb) {
        tok_off.push_back(to); len.push_back(T); mask.push_back(lo); query.push_back(q);
        label.push_back(lb); row.push_back(0); urow_h.push_back(0); urow_m.push_back(0);
        mask_end.push_back(hi);
    }
    size_t size() const { return len.size(); }
};

struct Chunk {
    int s0, s1, rows;
    int urows = 0;     // layer-0 unique rows (dedup mode), 0 = dedup off for this chunk
    int max_len = 0;   // longest sequence of the chunk (attention kernel choice)
    int q0 = 0, nq = 0;   // query-list calls (QueryList): first query of the chunk, and their count
};

// Row r of rs_pll_score_spans: 1 <= lo <= query < hi <= T - 1 ([CLS] and [SEP] are never masked).
inline bool span_ok(int T, int lo, int hi, int query) {
    return 1 <= lo && lo <= query && query < hi && hi <= T - 1;
}

inline int pad_to(long long rows, int align) { return (int)((rows + align - 1) / align * align); }

// Chunks of <= cap rows and <= s_cap sequences (every len in [1, cap]); sets sl.row (first row of
// a sequence in its chunk).
inline void cut_rows(SeqList& sl, long long cap, int s_cap, std::vector<Chunk>* chunks) {
    const size_t S = sl.size();
    int rows = 0, s0 = 0, max_len = 0;
    for (size_t s = 0; s < S; ++s) {
        const int T = sl.len[s];
        if (rows + T > cap || (int)s - s0 >= s_cap) {
            chunks->push_back({s0, (int)s, rows, 0, max_len});
            s0 = (int)s;
            rows = 0;
            max_len = 0;
        }
        sl.row[s] = rows;
        rows += T;
        max_len = std::max(max_len, T);
    }
    if (S) chunks->push_back({s0, (int)S, rows, 0, max_len});
}

// Query list of a multi-mask call (rs_pll_score_sets, rs_masked_logprob_multi), beside the
// sequence list: sequence s scores the positions pos[first[s] .. first[s + 1]), strictly ascending,
// each against label[q] (-1: the token at the position).  masked: the positions are also the
// sequence's [MASK] set (the embedding replaces them on the device); the list's mask / query
// columns are then unused (-1 / 0).
struct QueryList {
    std::vector<int> first{0}, pos, label;   // first: [S + 1] once every sequence is pushed
    bool masked = false;
    // the queries of the next sequence: n positions p[0 .. n)
    void push(const int* p, int n, int lb) {
        pos.insert(pos.end(), p, p + n);
        label.insert(label.end(), (size_t)n, lb);
        first.push_back((int)pos.size());
    }
    int count(size_t s) const { return first[s + 1] - first[s]; }
    size_t size() const { return pos.size(); }
};

// 0 <= lo <= p[0] < p[1] < ... < p[n - 1] <= hi, n >= 1
inline bool positions_ok(const int* p, int n, int lo, int hi) {
    if (n < 1 || p[0] < lo || p[n - 1] > hi) return false;
    for (int i = 1; i < n; ++i)
        if (p[i] <= p[i - 1]) return false;
    return true;
}

// cut_rows for a query-list call: chunks of <= cap rows, <= s_cap sequences and <= s_cap queries
// (the per-query workspace holds s_cap rows, as the per-sequence one does); sets sl.row and the
// chunks' q0 / nq.  A sequence with more than s_cap queries fits no chunk: returns its index
// (nothing usable in *chunks then), else -1.
inline int cut_rows_queries(SeqList& sl, const QueryList& ql, long long cap, int s_cap, std::vector<Chunk>* chunks) {
    const size_t S = sl.size();
    int rows = 0, s0 = 0, max_len = 0;
    for (size_t s = 0; s < S; ++s) {
        const int T = sl.len[s], n = ql.count(s);
        if (n > s_cap) return (int)s;
        if (rows + T > cap || (int)s - s0 >= s_cap || ql.first[s + 1] - ql.first[s0] > s_cap) {
            chunks->push_back({s0, (int)s, rows, 0, max_len, ql.first[s0], ql.first[s] - ql.first[s0]});
            s0 = (int)s;
            rows = 0;
            max_len = 0;
        }
        sl.row[s] = rows;
        rows += T;
        max_len = std::max(max_len, T);
    }
    if (S) chunks->push_back({s0, (int)S, rows, 0, max_len, ql.first[s0], ql.first[S] - ql.first[s0]});
    return -1;
}

// Layer-0 dedup (MLM_PLL): the masked copies of one hypothesis share every layer-0 input row
// except the masked ones, so the layer-0 QKV projection runs over UNIQUE rows.  A run of copies
// of one hypothesis inside the chunk gets its T original rows, then one [MASK] row for every
// position of [min lo, max hi) over the run: "[MASK] at position q" is the same row whichever
// copy masks q.  urow_h[s] = first unique row of the run, urow_m[s] = the [MASK] row of the
// sequence's first masked position (chunk-local); its span reads urow_m[s] + (t - lo).  A
// hypothesis cut across chunks may mask positions whose own copies sit in the neighbouring
// chunk: the range covers them.  One-position spans in ascending order (rs_pll_score) number
// their [MASK] rows one per copy, in copy order.  Returns the chunk's unique-row count, or 0
// when a sequence has no mask position (dedup not applicable).
inline int plan_unique_rows(SeqList& sl, int s0, int s1) {
    int u = 0;
    for (int s = s0; s < s1;) {
        if (sl.mask[s] < 0) return 0;
        int e = s + 1, lo = sl.mask[s], hi = sl.mask_end[s];
        for (; e < s1 && sl.tok_off[e] == sl.tok_off[s] && sl.len[e] == sl.len[s]; ++e) {
            if (sl.mask[e] < 0) return 0;
            lo = std::min(lo, sl.mask[e]);
            hi = std::max(hi, sl.mask_end[e]);
        }
        const int base = u, mbase = u + sl.len[s];
        for (int k = s; k < e; ++k) {
            sl.urow_h[k] = base;
            sl.urow_m[k] = mbase + (sl.mask[k] - lo);
        }
        u = mbase + (hi - lo);
        s = e;
    }
    return u;
}

// The unique rows are the rows of the layer-0 QKV GEMM, which pads them to its row alignment and
// reads and writes workspace reserved for `reserved` rows (a multiple of the alignment).  A run
// with one copy and a w-token span has T + w > T unique rows, and a chunk of many one-copy runs
// (170 hypotheses of one word at 512 rows: 680 unique rows) exceeds its token rows; where the
// padded count would exceed the reservation the chunk runs without dedup (the same scores: the
// dedup is exact).  Returns urows, or 0.
inline int unique_rows_fit(int urows, int align, long long reserved) {
    return pad_to(urows, align) <= reserved ? urows : 0;
}

// embed_unique: the unique rows that the block of sequence s writes.  The first sequence of a
// run writes the hypothesis' T original rows [urow_h, urow_h + T); the last sequence of a run
// writes the run's n_mask [MASK] rows [mask_row, mask_row + n_mask), positions mask_pos + j.
// Every unique row of the chunk has exactly one writer, and no block writes more than
// T + (T - 2) rows.  urow_h_prev / urow_h_next: urow_h of the neighbouring sequences of the
// chunk (ignored for its first / last sequence); urows: the chunk's unique-row count.
struct UniqueOwn {
    int n_orig, n_mask, mask_row, mask_pos;
};
RS_PLAN_HD inline UniqueOwn unique_rows_owned(bool first_in_chunk, bool last_in_chunk, int urow_h_prev, int urow_h,
                                              int urow_h_next, int urow_m, int T, int lo, int urows) {
    UniqueOwn w{0, 0, 0, 0};
    if (first_in_chunk || urow_h_prev != urow_h) w.n_orig = T;
    if (last_in_chunk || urow_h_next != urow_h) {
        w.mask_row = urow_h + T;
        w.mask_pos = lo - (urow_m - w.mask_row);
        w.n_mask = (last_in_chunk ? urows : urow_h_next) - w.mask_row;
    }
    return w;
}
