/*
 * librescore — C ABI of the MI355X-native N-best LM rescorer (gfx950 HIP kernels).
 *
 * The reference (ishine/ASR-Rescoring) is pure Python with no FFI; its seams on the hot
 * path are Python calls.  Each entry point below names the reference interface it
 * replaces (file:line, relative to the reference repo).  The Python host mirror in
 * asr-rescoring_amd/ binds these with ctypes (see INTEGRATION.md for the binding a
 * maintainer would add to the reference).
 *
 * Conventions
 *   - d_* pointers are device memory owned by the caller (e.g. the PyTorch caching
 *     allocator); h_* pointers are host memory read during the call only.
 *   - stream is a hipStream_t (torch.cuda.current_stream().cuda_stream); every call is
 *     asynchronous on it unless stated (the scoring calls synchronise at their end: range
 *     guard below).  No C++ exception crosses the ABI.
 *   - return 0 on success, a negative RS_E* code on failure; rs_last_error() gives a
 *     thread-local message.
 *   - A model handle is bound to one device and must not be used by two host threads
 *     at once.  Calls on one handle are ORDERED even across streams: they share the handle's
 *     workspace, LayerNorm gang-ticket words and flags, so a call issued on a different stream
 *     than the previous call first makes its stream wait (device-side) for the previous call's
 *     work.  Results are deterministic (no float atomics, fixed reduction orders).
 *   - The fused residual + LayerNorm GEMM (fp16x3 mode) exchanges row statistics between the
 *     N_pad / 256 workgroups of a row panel inside one launch (a gang).  Gangs are formed only
 *     from workgroups that have started, and the row panels come in lists that a gang takes from a
 *     counter, so the lists of gangs that never formed (workgroups held off by another tenant) are
 *     computed by those that did: the launch completes on whatever CUs it gets, with 3 free
 *     workgroup slots anywhere on the GPU for bert-base.  The hardware dispatches a grid's
 *     workgroups round-robin over the 32 shader engines (8 XCDs x 4); while another tenant fills a
 *     whole engine, the workgroups dispatched to it (of this kernel or any other) wait for it.
 *     Every wait inside a launch is bounded (statistics 1 s, gang formation 10 s): one that runs
 *     out ends the call in RS_EHIP instead of hanging.
 */
#ifndef RESCORE_H_
#define RESCORE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_OK 0
#define RS_EARG (-1)      /* bad argument / shape */
#define RS_EHIP (-2)      /* HIP runtime error */
#define RS_ESTATE (-3)    /* call order (e.g. scoring before rs_model_finalize) */
#define RS_ENOMEM (-4)
#define RS_EUNSUP (-5)    /* shape outside what the kernels support */

#define RS_DT_F32 0

#define RS_HEAD_MLM 1     /* BertForMaskedLM head: cls.predictions.* (MLM_PLL) */
#define RS_HEAD_CLS 2     /* RescoreBert head: linear.weight [1,H], linear.bias [1] */
#define RS_HEAD_EMB 4     /* encoder only: token embeddings (BERTScore, bert_score.utils.bert_encode) */

#define RS_LOSS_MD 0      /* RescoreBert training methods (RescoreBert/main.py:104-147) */
#define RS_LOSS_MWER 1    /* MD_MWER: MWER + md_loss_weight * MD */
#define RS_LOSS_MWED 2    /* MD_MWED: MWED + md_loss_weight * MD */

#define RS_BS_P 0         /* BERTScore component used as the MBR utility */
#define RS_BS_R 1
#define RS_BS_F 2

#define RS_FUSE_NORM 0    /* (1-w)*am/len + w*lm/len      rescore.py:51 */
#define RS_FUSE_LEGACY 1  /* (1-w)*am + w*lm              rescore_result/MLM_PLL/rescore.log:28 */
#define RS_FUSE_AM_NORM 2 /* (1-w)*am/len + w*lm          rescore_result/RMBR/BertScore/rescore_mbr_normalize.log:29 */

typedef struct rs_model rs_model;

/* transformers.BertConfig fields used by the reference (bert-base-chinese:
 * 21128/768/12/12/3072/512/2, eps 1e-12, [MASK] = 103). */
typedef struct rs_bert_cfg {
    int32_t vocab, hidden, layers, heads, intermediate, max_pos, type_vocab;
    float ln_eps;
    int32_t mask_id;
    int32_t heads_mask;   /* RS_HEAD_MLM | RS_HEAD_CLS */
    int32_t precision;    /* RS_PREC_FP16 or RS_PREC_FP16X3 */
} rs_bert_cfg;

/* GEMM operand precision.  FP16X3 (the default of every scorer): each fp32 operand x is
 * split into fp16 hi + lo (lo scaled by 64) and the three significant products
 * A_hi.W_hi + A_hi.W_lo + A_lo.W_hi are accumulated in fp32 on the fp16 MFMA — by the
 * split-operand kernel from two-part images, the third product's factors formed in registers
 * (fp32-level accuracy: PLL ~1e-7 relative of the fp32 reference, 3 MFMA products per
 * algorithmic one).  FP16: fp16 MFMA inputs, fp32 accumulation (opt-in reduced-precision
 * mode: per-row log-probs within ~1e-4 relative).  Both modes hold operands in fp16 images,
 * so |x| <= 65504: weights beyond it fail rs_model_finalize, activations beyond it make the
 * scoring call fail with RS_EUNSUP (range guard, below). */
#define RS_PREC_FP16 0
#define RS_PREC_FP16X3 1

int rs_version(void);
const char* rs_last_error(void);

/* Replaces BertForMaskedLM.from_pretrained / RescoreBert(...) construction
 * (MLM_PLL/main.py:184, RescoreBert/model.py:5-11).  Requires hidden % 256 == 0,
 * head_dim == 64, intermediate % 128 == 0. */
int rs_model_create(const rs_bert_cfg* cfg, int device, rs_model** out);

/* Replaces model.load_state_dict(torch.load(checkpoint)) (MLM_PLL/main.py:185-186,
 * RescoreBert/main.py:250-251): one HF state_dict tensor by key, host fp32. */
int rs_model_set_tensor(rs_model* m, const char* hf_key, const void* host_ptr, int dtype,
                        const int64_t* shape, int ndim);

/* Packs the tensors into the kernel layouts (fp16 GEMM weights, fused QKV) on device.
 * Fails with RS_ESTATE naming the first missing key, RS_EUNSUP for a weight outside the fp16 range.
 * fp16x3: the split-operand GEMMs form 64 W_hi in fp16, so a model with a projection weight of
 * |w| >= 1023.75 is packed without them and runs the K-concatenated fp16x3 form (same accuracy,
 * slower); scores are never affected. */
int rs_model_finalize(rs_model* m);

/* Sizes the activation workspace for up to max_rows token rows per launch chunk
 * (>= 512).  Optional: scoring calls reserve a default on first use. */
int rs_model_reserve(rs_model* m, int64_t max_rows);

/* Range guard of the scoring calls (rs_pll_score, rs_pll_score_spans, rs_masked_logprob, rs_masked_topk, rs_pll_topk,
 * rs_cls_score, rs_token_embed, rs_bertscore_recall): after the last launch the call checks its outputs
 * for non-finite values (an operand image that overflowed fp16 turns every dependent score
 * into inf / NaN), synchronises `stream` and returns RS_EUNSUP with a message instead of
 * handing back non-finite scores.  These calls therefore return with their work complete.
 * The same report carries RS_EHIP when a fused residual-LayerNorm GEMM timed out waiting for
 * its row statistics (each call reports only its own).
 *
 * rs_model_set_sync_check(m, 0) defers that report: the calls only enqueue the check (they stay
 * asynchronous on `stream`), the flags accumulate on the device, and rs_check(m, stream)
 * synchronises `stream`, reports (RS_EUNSUP / RS_EHIP) and clears them.  on = 1 restores the
 * default; call rs_check first so nothing pending is dropped.  In deferred mode a statistics-wait
 * timeout (RS_EHIP) is sticky on the device until rs_check: every fused-LayerNorm launch after it
 * drains at once (fail-fast: no further waits), so EVERY result produced between the timeout and
 * the rs_check that reports it is invalid and must be discarded — not only the timed-out call's.  No reference counterpart (the
 * reference's forward is synchronous PyTorch-CPU, MLM_PLL/main.py:83-107). */
int rs_model_set_sync_check(rs_model* m, int on);
int rs_check(rs_model* m, void* stream);

/* Segment ids (transformers token_type_ids) for the NEXT scoring call on this handle:
 * d_type int32 [n] device, d_type[i] = type of d_tok[i] / d_ids[i] of that call.
 * Reference seam: BertEmbeddings (modeling_bert.py:53-108) with token_type_ids as
 * Nbest_Align/model.py:21-26 passes them: row = word[id] + token_type[type] + position[t]; a
 * [MASK] row of the PLL calls takes the type of the position it stands at.
 * One-shot: the setting applies to the next call that runs the encoder (rs_pll_score,
 * rs_pll_score_spans, rs_masked_logprob, rs_masked_topk, rs_pll_topk, rs_cls_score, rs_token_embed,
 * rs_bertscore_recall) and is cleared when that call returns, whatever it returns (a call with
 * n_hyp == 0 consumes it as well).  d_type == NULL clears a pending setting.  d_type must stay valid
 * until that call's work on its stream is complete, like d_tok.
 * The consuming call fails with RS_EARG when n differs from the number of tokens it addresses
 * (h_off[n_seq]).  Values outside [0, type_vocab) are clamped on the device, like token ids, and never
 * read out of bounds.  Without a setting every row has type 0 and scores are those of a handle that
 * never heard of segment ids, bit for bit.  Precision modes, chunking, layer-0 dedup (a unique row is
 * keyed by hypothesis and position, and so is its type), the last-layer query path, the range guard,
 * deferred checks and call ordering are unchanged. */
int rs_model_set_token_types(rs_model* m, const int32_t* d_type, int64_t n);

/* MLM_PLL scoring (MLM_PLL/preprocess.py:9-30 + MLM_PLL/main.py:83-107):
 *   d_tok      int32 [h_hyp_off[n_hyp]]  hypotheses as [CLS] w_1..w_L [SEP]
 *   h_hyp_off  int32 [n_hyp + 1]         host offsets into d_tok (T_h = L_h + 2 >= 3)
 *   d_pll      float64 [n_hyp]           sum_p log p(w_p | w_{\p}) accumulated in row
 *                                        order p = 1..L (== output_score[u][h])
 *   d_row_lp   float32 [sum_h L_h] or NULL: per masked row log-prob (== token_score)
 * The L masked copies are expanded on device. */
int rs_pll_score(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                 double* d_pll, float* d_row_lp, void* stream);

/* Span-masked PLL: rs_pll_score with a caller-given list of scored rows per hypothesis, each row
 * masking a range of positions instead of one.  Reference seam: MLM_PLL/preprocess.py:9-30
 * generalised (do_job masks exactly position p in row p); the word variants are Kauf & Ivanova
 * 2023, "A Better Way to Do Masked Language Model Scoring" (no reference counterpart).
 *   h_row_off  int32 [n_hyp + 1] host   rows of hypothesis h: [h_row_off[h], h_row_off[h+1]);
 *                                       ascending, h_row_off[0] == 0
 *   h_lo, h_hi, h_query  int32 [h_row_off[n_hyp]] host, positions relative to the hypothesis:
 *                        row r is the hypothesis with positions [lo_r, hi_r) replaced by [MASK],
 *                        scored at query_r; 1 <= lo <= query < hi <= T - 1 ([CLS] and [SEP] are
 *                        never masked), anything else RS_EARG with a message naming the row
 *   d_row_lp   float32 [h_row_off[n_hyp]] or NULL: log_softmax(logits[query_r])[tok[query_r]]
 *   d_pll      float64 [n_hyp]: the sum of the hypothesis' rows in row order; no rows: 0.0
 * Rows of a hypothesis may come in any order, repeat and skip positions (a scored sub-range, a
 * strided approximation).  Rows (p, p + 1, p) for p = 1..L are rs_pll_score's, bit for bit.
 *   PLL-word-l2r:    row p masks [p, end of p's word)
 *   PLL-whole-word:  row p masks [begin of p's word, end of p's word)
 * Precision modes, chunking, layer-0 dedup (a run of copies shares one [MASK] row per masked
 * position), the last-layer query path, the range guard and deferred checks are those of
 * rs_pll_score; a model without the MLM head: RS_ESTATE. */
int rs_pll_score_spans(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                       const int32_t* h_row_off, const int32_t* h_lo, const int32_t* h_hi,
                       const int32_t* h_query, double* d_pll, float* d_row_lp, void* stream);

/* Row-level MLM drop-in (MLM_PLL/main.py:89-105 for an arbitrary batch):
 *   d_ids      int32 ragged sequences (already masked), h_seq_off int32 [n_seq+1] host
 *   h_query    int32 [n_seq] host   position of the masked token in each sequence
 *   d_label    int32 [n_seq]        label id at that position
 *   d_out      float32 [n_seq]      log_softmax(logits[query])[label]
 * A label outside [0, vocab) here (except -1, which takes the token id at the position), or a
 * token id outside [0, vocab) at a scored position of rs_pll_score, has log-probability -inf: the
 * call fails with RS_EUNSUP (the range guard above). */
int rs_masked_logprob(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off,
                      const int32_t* h_query, const int32_t* d_label, int32_t n_seq,
                      float* d_out, void* stream);

/* Multi-mask rows: several [MASK] positions in one row, every one of them scored from that row's
 * single forward.  Reference seam: BertForMaskedLM(input_ids, labels) with labels at every masked
 * position and -100 elsewhere (MLM_PLL/main.py:89-97 passes labels for all positions); the strided
 * PLL approximation masks every k-th token of one copy and scores all of them from it, min(k, L)
 * forwards per hypothesis instead of L.
 *   h_row_off  int32 [n_hyp + 1] host   rows (forwards) of hypothesis h: [h_row_off[h], h_row_off[h+1]);
 *                                       ascending, h_row_off[0] == 0
 *   h_pos_off  int32 [n_rows + 1] host  positions of row r: h_pos[h_pos_off[r] .. h_pos_off[r+1])
 *   h_pos      int32 [n_pos] host       relative to the hypothesis, strictly ascending within a row,
 *                                       1 <= p <= T - 2, at least one per row; anything else RS_EARG
 *                                       with a message naming the row
 *   d_pos_lp   float32 [n_pos] or NULL: log_softmax(logits[pos_i])[tok[pos_i]] of the row that holds
 *                                       position i, that row being the hypothesis with all of ITS
 *                                       positions replaced by [MASK] on the device
 *   d_pll      float64 [n_hyp]: the sum of the hypothesis' entries in list order; no rows: 0.0
 * One position per row, p = 1..L, is rs_pll_score's row list.  A position's value does not depend on
 * which of its row's other [MASK] positions are scored, and results are bitwise reproducible.
 * The last layer and the head run one state row per POSITION; a launch chunk holds at most
 * max_rows / 3 + 1 of them (the per-sequence workspace of the other calls), so a single row with
 * more positions than that is RS_EARG (the message names the max_rows that fits it).
 * Layer-0 dedup does not apply: these calls run layer 0 over all token rows (the dedup is exact, so
 * no score depends on it).  No top-k form.  Precision modes, chunking, rs_model_set_token_types,
 * the last-layer query path, the range guard, deferred checks and call ordering are those of
 * rs_pll_score.  A model without the MLM head: RS_ESTATE; with fewer than 2 layers: RS_EUNSUP. */
int rs_pll_score_sets(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                      const int32_t* h_row_off, const int32_t* h_pos_off, const int32_t* h_pos,
                      double* d_pll, float* d_pos_lp, void* stream);
/* rs_masked_logprob with any number (>= 1) of query positions per row; the rows are already masked by
 * the caller.
 *   h_q_off    int32 [n_seq + 1] host   queries of row s: h_qpos[h_q_off[s] .. h_q_off[s+1])
 *   h_qpos     int32 [n_q] host         strictly ascending within a row, 0 <= p < T (else RS_EARG)
 *   d_label    int32 [n_q]              label id per query; -1 = the token id at the position
 *   d_out      float32 [n_q]            log_softmax(logits[qpos_i])[label_i]
 * A label outside [0, vocab) has log-probability -inf: RS_EUNSUP through the range guard. */
int rs_masked_logprob_multi(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                            const int32_t* h_q_off, const int32_t* h_qpos, const int32_t* d_label,
                            float* d_out, void* stream);
/* rs_masked_logprob_multi with a candidate list per query in place of one label: the log-probability
 * of every listed vocabulary id at the query's position, from the row's one forward (the decoder
 * keeps the listed columns of the logit row it has formed; the [n_q, vocab] logits are never stored).
 * No reference counterpart; the seam is the slot question of Nbest_Align/model.py:20-45.
 *   h_c_off    int32 [n_q + 1] host     candidates of query q: h_cand[h_c_off[q] .. h_c_off[q+1]);
 *                                       starts at 0, never descends (else RS_EARG); an empty list is
 *                                       allowed and scores nothing
 *   h_cand     int32 [n_c] host         vocabulary ids in any order, duplicates allowed (each entry gets
 *                                       its value); an id outside [0, vocab) is RS_EARG with a message
 *                                       naming the query
 *   d_out      float32 [n_c]            d_out[c] = log_softmax(logits[qpos of c's query])[h_cand[c]], in
 *                                       the caller's order
 * d_out[c] equals, bit for bit, what rs_masked_logprob_multi returns for that query with h_cand[c] as
 * its label; it does not depend on the query's other candidates, on the chunking (max_rows) or on
 * the run.  Rows, queries, precision modes, chunking, rs_model_set_token_types, the range guard over
 * d_out, deferred checks, call ordering and the RS_ESTATE / RS_EUNSUP cases are those of
 * rs_masked_logprob_multi.  The candidate workspace (the call's lists and one chunk's logits) is
 * allocated at the first such call and kept on the handle (RS_ENOMEM if it cannot be). */
int rs_masked_logprob_cands(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                            const int32_t* h_q_off, const int32_t* h_qpos, const int32_t* h_c_off,
                            const int32_t* h_cand, float* d_out, void* stream);

/* Top-k token candidates at masked positions: the model's k preferred vocabulary entries of a row
 * and their log-probabilities.  Reference seam: logits[range(B), mask_pos] of MLM_PLL/main.py:101-105
 * BEFORE the label gather — the reference forms the whole [B, vocab] row and keeps one entry; these
 * calls return the k best of log_softmax of that row (torch.topk order: best first) without ever
 * materialising it: the decoder GEMM's epilogue keeps the best k (logit, column) pairs of every
 * 64-column slab, and one merge per row orders them.
 *   k          1 .. RS_TOPK_MAX, k <= vocab (else RS_EARG; a null output: RS_EARG)
 *   d_top_id   int32   [rows, k] row-major   vocabulary ids, best first
 *   d_top_lp   float32 [rows, k]             their log-probabilities, non-increasing along k
 * Order: larger logit first; equal logits (fp32) by the lower id — a total order, so the result does
 * not depend on chunking or tile shape and is bitwise reproducible (no atomics).  The log-prob of
 * an id is formed from the same logit and the same logsumexp as rs_masked_logprob / rs_pll_score
 * form for that id as a label: equal bit for bit.  Precision modes, chunking, layer-0 dedup and the
 * last-layer query path are those of rs_pll_score; a model without the MLM head: RS_ESTATE.
 * The range guard covers d_top_lp (and d_row_lp): a non-finite value is RS_EUNSUP, deferred by
 * rs_model_set_sync_check(m, 0) like every scoring call's.
 * Workspace: the first top-k call on a handle allocates the candidate buffer, 2048 rows x
 * (vocab padded to 128) / 64 slabs x RS_TOPK_MAX x 8 bytes (bert-base-chinese: 87 MB), kept until
 * rs_model_destroy; RS_ENOMEM if it does not fit.  The decoder of a top-k call runs over sub-batches
 * of 2048 rows so that this size does not grow with max_rows; handles that never ask pay nothing. */
#define RS_TOPK_MAX 16
/* fill-mask on already-masked rows (arguments as rs_masked_logprob, no labels): rows = n_seq */
int rs_masked_topk(rs_model* m, const int32_t* d_ids, const int32_t* h_seq_off, const int32_t* h_query,
                   int32_t n_seq, int32_t k, int32_t* d_top_id, float* d_top_lp, void* stream);
/* rs_pll_score plus the candidates of every masked row (rows ordered as d_row_lp: hypothesis by
 * hypothesis, p = 1..L).  d_pll and d_row_lp (both nullable here) are rs_pll_score's, bit for bit. */
int rs_pll_topk(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp, int32_t k,
                double* d_pll, float* d_row_lp, int32_t* d_top_id, float* d_top_lp, void* stream);

/* RescoreBert scoring (RescoreBert/model.py:13-21, RescoreBert/main.py:156-158):
 * CLS hidden of the last layer -> Linear(H, 1).  d_out float32 [n_hyp]. */
int rs_cls_score(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                 float* d_out, void* stream);

/* Per-kernel-kind device timing (HIP events around every launch of that kind, on the
 * call's stream).  Enable before a scoring call; read after it (synchronises).
 * kind: RS_K_QKV, RS_K_OPROJ, RS_K_FFN1, RS_K_FFN2, RS_K_DECODER, RS_K_ATTN, RS_K_OTHER.
 * flops = algorithmic FLOPs of the launches of that kind (2*M*N*K over valid rows). */
#define RS_K_QKV 0
#define RS_K_OPROJ 1
#define RS_K_FFN1 2
#define RS_K_FFN2 3
#define RS_K_DECODER 4
#define RS_K_ATTN 5
#define RS_K_OTHER 6
#define RS_K_COUNT 7
int rs_profile_enable(rs_model* m, int on);
int rs_profile_read(rs_model* m, int kind, double* ms, int64_t* launches, double* flops);

void rs_model_destroy(rs_model* m);

/* RMBR CER utility (RMBR/utility_functions.py:28-33 via RMBR/mbr.py:5-28): the
 * pairwise Levenshtein matrix of every utterance's hypotheses, computed once.
 *   d_chars   int32 symbols, d_str_off int32 [n_str+1], d_utt_off int32 [n_utt+1]
 *             (strings of utterance u = utt_off[u]..utt_off[u+1])
 *   d_mat_off int64 [n_utt+1] offsets of each n_u x n_u block in d_ed (row-major)
 *   d_ed      int32 out: d_ed[mat_off[u] + i*n_u + j] = ed(string_i, string_j)
 * Myers/Hyyro bit-parallel: one 64-bit word when the shorter string of a pair has <= 64
 * symbols, 64-row words with carried horizontal deltas beyond; exact when the shorter
 * string has <= 16384 symbols, -1 otherwise (the Python wrappers reject such inputs). */
int rs_pairwise_edit(const int32_t* d_chars, const int32_t* d_str_off, const int32_t* d_utt_off,
                     const int64_t* d_mat_off, int32_t n_utt, int32_t max_n, int32_t* d_ed,
                     void* stream);

/* Token embeddings of the BERTScore utility (RMBR/utility_functions.py:9-22 ->
 * bert_score.utils.get_bert_embedding / bert_encode with the model truncated to cfg.layers
 * layers — bert_score uses 8 for bert-base-chinese — and greedy_cos_idf's per-token L2
 * normalisation), row = token position in d_tok (h_hyp_off: host int32 [n_hyp+1], hypotheses
 * as [CLS] w.. [SEP]).  d_emb layout by the model's precision: RS_PREC_FP16X3 — the two-part
 * image fp16 [hyp_off[n_hyp], 2*hidden], row = [hi | lo*64], e = hi + lo/64 (fp32-class, ~22
 * bits); RS_PREC_FP16 — fp16 [hyp_off[n_hyp], hidden]. */
int rs_token_embed(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                   void* d_emb, void* stream);

/* bert_score.score(cands=[hyp_i], refs=[hyp_j], idf=False) for every ordered pair of each
 * utterance's hypotheses, as the recall matrix
 *   d_rmat[mat_off(u) + i*n_u + j] = R(cand = hyp_i, ref = hyp_j),
 *   mat_off(u) = sum_{v<u} n_v^2 (n_u = h_utt_off[u+1] - h_utt_off[u]);
 * P(i|j) = R(j|i), F = 2PR/(P+R).  R = mean over ref j's tokens except [CLS]/[SEP] of the max
 * cosine over all of cand i's tokens; 0 when either hypothesis is empty (T == 2).  Cosines:
 * RS_PREC_FP16X3 three fp16 products of the two-part embeddings, fp32 accumulation (fp32-class);
 * RS_PREC_FP16 one.
 * d_rmat0 (optional, same layout): each maximum taken as max(m, 0) — bert_score's value when
 * the cand is shorter than the longest cand of its pair batch (the padded positions' masked
 * cosine 0 joins the max, bert_score/utils.py greedy_cos_idf); the caller picks R or R0 per
 * pair from its batch layout (bertscore.py).
 * h_hyp_off[0] == 0, h_utt_off[0] == 0 (host arrays); every hypothesis has T >= 2. */
int rs_bertscore_recall(rs_model* m, const int32_t* d_tok, const int32_t* h_hyp_off,
                        const int32_t* h_utt_off, int32_t n_utt, float* d_rmat, float* d_rmat0, void* stream);

/* RMBR mbr_decode (RMBR/mbr.py:5-28) with the BERTScore utility component `which`
 * (RS_BS_P/R/F) of cand hyp_i against ref hyp_j, from the rs_bertscore_recall matrix;
 * summation and argmax as rs_mbr_scores. */
int rs_mbr_scores_bs(const float* d_rmat, const int64_t* d_mat_off, const int32_t* d_utt_off, int32_t n_utt,
                     int32_t k, int32_t which, float* d_scores, int32_t* d_argmax, void* stream);

/* ---- Levenshtein alignment with backtrace (espnet_data/preprocess/align.py:5-97
 * levenshtein_distance_alignment) -----------------------------------------
 * Pair p aligns ref tokens d_ref[d_ref_off[p] .. d_ref_off[p+1]) with hyp tokens
 * d_hyp[d_hyp_off[p] .. ) (int32 token ids, any values; 0 <= length <= 4096, max_len = the
 * longest list of the call).  Reference rules: rows = hyp, columns = ref, both with a start
 * sentinel; equal tokens take the diagonal cost as "U"; otherwise S = diag + 1, replaced only
 * by a strictly smaller I = left + 1, then by a strictly smaller D = up + 1; first column D,
 * first row I; traceback from the end: U / S consume both, D = hyp-only token (ref "*"),
 * I = ref-only token (hyp "*"); output in forward order (the reference reverses its lists).
 * Outputs at d_out_off[p] (int64, room for len(ref) + len(hyp) entries): d_ops int8
 * (RS_AL_U / _S / _I / _D), d_ref_idx / d_hyp_idx int32 (index into the pair's ref / hyp
 * tokens, -1 = "*"), d_n[p] = the alignment's length.  d_lab: uint8 scratch of
 * (len(hyp) + 1) * (len(ref) + 1) bytes per pair at d_lab_off[p] (int64).  Async on `stream`. */
#define RS_AL_U 0
#define RS_AL_S 1
#define RS_AL_I 2
#define RS_AL_D 3
int rs_align(const int32_t* d_ref, const int32_t* d_ref_off, const int32_t* d_hyp, const int32_t* d_hyp_off,
             int32_t n_pairs, const int64_t* d_lab_off, uint8_t* d_lab, const int64_t* d_out_off, int8_t* d_ops,
             int32_t* d_ref_idx, int32_t* d_hyp_idx, int32_t* d_n, int32_t max_len, void* stream);

/* ---- N-best confusion network (Nbest_Align/preprocess.py:41-64,92-139; CorrectBart/get_feature.py) ----
 * Utterance u owns hypotheses d_utt_off[u] .. d_utt_off[u+1]) (N >= 1), the first being the top-1 of L1
 * tokens.  A table of S slots x N columns holds, per column n, the index of a token inside hypothesis n
 * or -1 for a gap ("*"); column 0 is the top-1.  All calls are asynchronous on `stream`, use no atomics
 * and give the same bits on every run.
 *
 * rs_cn_merge — new_merge_alignments folded over hypotheses 2..N (preprocess.py:41-64,103-108), in
 * closed form: hypothesis n places k[n][g] tokens in gap g of the top-1 (g = 0..L1) and a[n][g] against
 * position g; gap g gives K[g] = max_n k[n][g] slots, then position g one slot.  In gap slot m column n
 * holds the m-th token hypothesis n has there; else, in RS_CN_REFERENCE and for g < L1, a copy of
 * a[n][g] when m < max_{n' < n} k[n'][g] (the reference's "*" branch appends the other alignment's entry
 * without advancing it); else a gap.  RS_CN_EXACT leaves a gap for those copies, so every hypothesis
 * token appears exactly once.
 *   d_ref_idx, d_hyp_idx, d_out_off, d_n   rs_align outputs for the pairs (top-1, hypothesis n), pair
 *                order utterance-major with n ascending: pair of (u, column c >= 1) is
 *                d_utt_off[u] - u + c - 1
 *   d_hyp_len    int32 [n_hyp] token counts; max_len = the longest (<= 4096, else RS_EUNSUP)
 *   d_gap_off    int64 [n_utt + 1], K of utterance u at d_K[d_gap_off[u] .. + L1 + 1)
 * Two launches.  Count (d_src == NULL): writes d_K and d_n_slots[u] = S.  The caller forms
 * d_slot_off int32 [n_utt + 1] (prefix sum of S) and d_cell_off int64 [n_utt + 1] (prefix sum of S * N).
 * Fill (d_src != NULL): reads d_K, writes d_src[d_cell_off[u] + slot * N + n]; nothing is written at or
 * beyond src_cap cells, and an utterance whose d_slot_off does not match its counts is left unwritten. */
#define RS_CN_REFERENCE 0
#define RS_CN_EXACT 1
int rs_cn_merge(const int32_t* d_ref_idx, const int32_t* d_hyp_idx, const int64_t* d_out_off, const int32_t* d_n,
                const int32_t* d_utt_off, const int32_t* d_hyp_len, int32_t n_utt, int32_t max_len,
                const int64_t* d_gap_off, int32_t* d_K, int32_t* d_n_slots, const int32_t* d_slot_off,
                const int64_t* d_cell_off, int32_t* d_src, int64_t src_cap, int32_t mode, void* stream);
/* rs_cn_oracle — the search of preprocess.py:112-139 (every combination, jiwer.cer, tokens.index) as a DP.
 * d_tok / d_hyp_off: the hypotheses' token ids (>= 0); d_ref / d_ref_off int32 [n_utt + 1]: one
 * transcript per utterance, as token ids of the same vocabulary.  d_dist[u] = the minimum, over every
 * path that picks one distinct entry per slot, of the token-level Levenshtein distance between the
 * transcript and the path without its gaps.  d_label[d_slot_off[u] + s] = the lowest column holding the
 * picked entry; among all minimum-distance paths the lexicographically smallest label vector.
 * d_E: int32 scratch of (S + 1) * (len(ref) + 1) per utterance at d_e_off[u] (int64).
 * Limits: max_n (most hypotheses of an utterance) <= 1024, max_ref (longest transcript) <= 4096, else
 * RS_EUNSUP. */
int rs_cn_oracle(const int32_t* d_src, const int32_t* d_slot_off, const int64_t* d_cell_off,
                 const int32_t* d_utt_off, const int32_t* d_tok, const int32_t* d_hyp_off, int32_t n_utt,
                 int32_t max_n, const int32_t* d_ref, const int32_t* d_ref_off, int32_t max_ref,
                 const int64_t* d_e_off, int32_t* d_E, int32_t* d_dist, int32_t* d_label, void* stream);
/* rs_cn_vote — ROVER-style vote per slot (no counterpart in the reference, which stops at the labels).
 * A slot's candidates are its distinct entries, the gap being one; a candidate's mass is the float64 sum
 * of d_w[hypothesis] over the columns holding it, added in ascending column order; the largest mass
 * wins, ties go to the candidate whose first column is lowest.  Per slot: d_win_tok (token id, -1 = gap),
 * d_win_col (the winner's first column), d_share (mass / sum of the utterance's weights, added in
 * ascending column order).  The decode without gaps of utterance u is d_dec[d_slot_off[u] .. + d_dec_len[u]).
 * max_n <= 1024, else RS_EUNSUP. */
int rs_cn_vote(const int32_t* d_src, const int32_t* d_slot_off, const int64_t* d_cell_off,
               const int32_t* d_utt_off, const int32_t* d_tok, const int32_t* d_hyp_off, int32_t n_utt,
               int32_t max_n, const double* d_w, int32_t* d_win_tok, int32_t* d_win_col, double* d_share,
               int32_t* d_dec, int32_t* d_dec_len, void* stream);

/* ---- RescoreBert training (RescoreBert/main.py:82-229) ---------------------------------
 * A trainer holds fp32 parameters (HF keys as for rs_model; bert.pooler.* is accepted and
 * ignored — RescoreBert's loss never reaches it), their gradients and AdamW moments.
 * rs_train_step_cls runs forward (activations kept), the distillation loss, the full
 * backward and (opts->update) one torch.optim.AdamW step.  Losses (RescoreBert/main.py:104-147;
 * train.h), over utterance groups g given by h_utt_off (the reference's reshape(-1, n_best)):
 *   MD      = sum_i (s_i - t_i)^2                            (MSELoss(reduction="sum"))
 *   MD_MWER = sum_g sum_i softmax(c_g)_i (cer_i - mean_g cer) + md_loss_weight * MD
 *   MD_MWED = sum_g KL(softmax(cer_g) || softmax(c_g / T_g)) + md_loss_weight * MD,
 *             T_g = sum c_g / sum cer_g (differentiated through), c = s + am.
 * Dropout (BERT train mode; the reference trains under model.train(), p = 0.1 by default):
 * hidden_dropout after the embedding LayerNorm and on the BertSelfOutput / BertOutput dense
 * outputs, attn_dropout on the attention probabilities, inverted scaling, on steps with
 * update >= 0 (the dev-loss pass, update = -1, is eval mode).  The keep bits are
 * counter-based (Philox4x32-10 keyed by dropout_seed and the trainer's dropout-step counter,
 * rs_trainer_dropout_step), so a step is bitwise reproducible; torch's RNG stream cannot be
 * matched, and the fixture-pinned runs use p = 0. */
typedef struct rs_trainer rs_trainer;
typedef struct rs_train_opts {
    int32_t loss;          /* RS_LOSS_MD / RS_LOSS_MWER / RS_LOSS_MWED */
    float md_loss_weight;  /* weight of MD in MD_MWER / MD_MWED (MD alone has weight 1) */
    float lr, beta1, beta2, eps, weight_decay;   /* torch.optim.AdamW arguments */
    int32_t update;        /* 1: backward + AdamW step; 0: backward only (gradients kept);
                              -1: forward + loss only (the reference's dev-loss pass) */
    float hidden_dropout;  /* BertConfig.hidden_dropout_prob (0 = off) */
    float attn_dropout;    /* BertConfig.attention_probs_dropout_prob (0 = off) */
    uint32_t dropout_seed;
} rs_train_opts;

/* cfg->heads_mask: RS_HEAD_CLS (RescoreBert) or RS_HEAD_MLM (MLM fine-tuning); shapes as
 * rs_model_create (T <= max_pos per sequence).  A step keeps the attention probabilities of every
 * layer for its backward: layers * sum_s heads * T_s^2 * 4 bytes over the batch's sequences (32
 * rows of 512 tokens on the BERT-base shape: 4.8 GB), plus one layer's worth of scratch when the
 * batch has a sequence of more than 128 tokens; a step whose buffers do not fit fails with
 * RS_ENOMEM.  RS_TRAIN_ATTN (read here): auto (default: the whole-head attention kernels while
 * every sequence of a batch has at most 128 tokens, the tiled kernels for a batch with a longer
 * one), tiled (the tiled kernels at every length) or legacy (the whole-head kernels only: longer
 * sequences fail with RS_EUNSUP); any other value fails with RS_EARG. */
int rs_trainer_create(const rs_bert_cfg* cfg, int device, rs_trainer** out);
int rs_trainer_set_tensor(rs_trainer* t, const char* hf_key, const void* host_ptr, int dtype,
                          const int64_t* shape, int ndim);
int rs_trainer_finalize(rs_trainer* t);
/* d_tok/h_hyp_off as rs_cls_score; h_utt_off int32 [n_utt+1] groups hypotheses by utterance;
 * d_target (mlm_pll_score), d_am (hyps_am_score), d_err (hyps_cer) float32 [n_hyp] (am/err
 * only for MWER/MWED);
 * d_scores (nullable) float32 [n_hyp] out; d_loss float32 [1] out.  Synchronises `stream`. */
int rs_train_step_cls(rs_trainer* t, const int32_t* d_tok, const int32_t* h_hyp_off, int32_t n_hyp,
                      const int32_t* h_utt_off, int32_t n_utt, const float* d_target, const float* d_am,
                      const float* d_err, const rs_train_opts* opts, float* d_scores, float* d_loss,
                      void* stream);
/* MLM fine-tuning step (MLM_PLL/main.py:73-161 run_one_epoch / mlm_finetune_bert; trainer
 * created with heads_mask RS_HEAD_MLM — cls.predictions.* with the decoder tied to the word
 * embeddings): d_ids / d_labels int32 rows (h_seq_off host int32 [n_seq+1]).  h_key_len (host
 * int32 [n_seq], nullable = whole rows): row s attends to its first h_key_len[s] tokens only —
 * the reference's padded batch (collate MLM_PLL/main.py:28-54: ids / labels padded with 0,
 * attention_mask 0) is rows of the batch's longest length whose pad positions are queries but
 * not keys.  loss = mean over ALL positions of the rows (pads included, label 0) of the CE of
 * BertForMaskedLM's logits (modeling_bert CrossEntropyLoss, MLM_PLL/main.py:89-97).
 * Synchronises `stream`. */
int rs_train_step_mlm(rs_trainer* t, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                      const int32_t* h_key_len, const int32_t* d_labels, const rs_train_opts* opts,
                      float* d_loss, void* stream);
/* The same step with labels at a caller-given list of token rows only — CrossEntropyLoss's
 * ignore_index = -100 convention of BertForMaskedLM(input_ids, labels) (modeling_bert.py:972-975),
 * the -100 positions simply left out of the list.  d_ids, h_seq_off, n_seq, h_key_len, opts, d_loss,
 * stream: as rs_train_step_mlm.  h_lab_row: host int32 [n_lab], the labelled token rows, indices
 * into the batch's M = h_seq_off[n_seq] rows, strictly ascending in [0, M); a row past its
 * sequence's key length (a pad position) is allowed — a query, not a key.  d_lab_id: device int32
 * [n_lab], the label of each listed row, clamped on the device to [0, vocab).
 *   loss = (1 / n_lab) sum over the listed rows of (logsumexp(logits) - logits[label]),
 * the mean over the non-ignored positions.  The transform and the tied decoder run on the n_lab
 * gathered hidden rows only ([n_lab, vocab] fp32 logits instead of [M, vocab]); the head's gradient
 * w.r.t. the hidden state is zero at every other row.  Gradients, AdamW, dropout sites and the
 * dropout-step counter, opts->update in {1, 0, -1}, rs_trainer_set_token_types, the attention form
 * above 128 tokens and the final synchronise are those of rs_train_step_mlm.  With n_lab == M and
 * h_lab_row = 0..M-1 the step equals rs_train_step_mlm on the same ids and labels bit for bit (loss,
 * every gradient, every parameter after the update).
 * Errors: RS_EARG for n_lab <= 0 (HF's loss is NaN there) and for a row index out of range or not
 * above its predecessor (the message names the first offending index); RS_ESTATE for a trainer
 * without the MLM head.  These are raised before any trainer state moves: no parameter, moment or
 * gradient changes and the dropout-step counter keeps its value, so the next step is the step it
 * would have been.  The batch errors shared with rs_train_step_mlm (offsets, key lengths, lengths
 * above max_position_embeddings) change no parameter either but, as there, are raised after a
 * dropout-active step has taken its key: the counter is then one further. */
int rs_train_step_mlm_labeled(rs_trainer* t, const int32_t* d_ids, const int32_t* h_seq_off, int32_t n_seq,
                              const int32_t* h_key_len, const int32_t* h_lab_row, int32_t n_lab,
                              const int32_t* d_lab_id, const rs_train_opts* opts, float* d_loss, void* stream);
/* Segment ids (token_type_ids) of the NEXT rs_train_step_cls / rs_train_step_mlm(_labeled): d_type int32 [n]
 * device, one per token row of that step (n must equal its h_off[n_seq], else the step fails with
 * RS_EARG).  One-shot like rs_model_set_token_types: cleared when that step returns, whatever it
 * returns; d_type == NULL clears a pending setting; values are clamped to [0, type_vocab).
 * The gradient of token_type_embeddings.weight[k] is the column sum of the embedding gradient over
 * the rows of type k, in the fixed row order of every other column sum (no atomics; a type without
 * rows gets exactly 0).  With nothing set the step is unchanged, bit for bit (all rows into row 0). */
int rs_trainer_set_token_types(rs_trainer* t, const int32_t* d_type, int64_t n);
/* The dropout-step counter: the key the next dropout-active step uses (then incremented). */
int64_t rs_trainer_dropout_step(const rs_trainer* t);
/* Sets it (0 .. 2^63-1; a 64-bit counter whose high word is a Philox counter word and low word
 * the second key word): part of the resume state — the CLI starts epoch k at k << 32, so every
 * epoch has 2^32 dropout steps of its own and a run resumed at epoch k draws the masks of the
 * straight run. */
int rs_trainer_set_dropout_step(rs_trainer* t, int64_t step);
/* d_keep uint8 [n]: the keep bit the trainer's kernels use for element e of dropout site
 * `site` (0 = embeddings; layer l: 1 + 3l attention probabilities in the saved-P layout,
 * 2 + 3l self-output, 3 + 3l output, element = row * hidden + column) in dropout step `step`
 * with probability p.  Test / export entry (masks fed to the CPU oracle). */
int rs_dropout_keep(uint32_t seed, uint64_t step, uint32_t site, float p, int64_t n, uint8_t* d_keep, void* stream);
/* Synchronous copies of one parameter / its last gradient (numel must match). */
int rs_trainer_get_tensor(rs_trainer* t, const char* hf_key, void* host_out, int64_t numel);
int rs_trainer_get_grad(rs_trainer* t, const char* hf_key, void* host_out, int64_t numel);
/* ---- Gradient accumulation, clipping and frozen tensors ------------------------------------
 * None of these changes a step that does not use them: with no entry below called, every
 * rs_train_step_* is what it was, bit for bit (kernels, launches, dropout keys).
 *
 * Frozen tensors: torch's requires_grad = False (the reference's util/freezer.py).  Every tensor
 * whose key equals hf_key_prefix or starts with hf_key_prefix + "." (whole dotted components: a
 * trailing '.' is ignored, "bert.encoder.layer.1" does not match layer 10) becomes trainable (1) or
 * frozen (0); on an MLM trainer cls.predictions.decoder.weight / .bias are the word embeddings /
 * cls.predictions.bias (one Parameter in HF), so freezing "cls" freezes the word embeddings.  A
 * prefix that matches nothing is RS_EARG; a call while the accumulator is non-empty RS_ESTATE.
 * Callable before or after rs_trainer_finalize; it takes effect at the next step, and the last
 * step's gradient is dropped (accumulate / apply / grad_norm on it are RS_ESTATE until a step has
 * run).  AdamW never touches a frozen tensor (no decay, moments kept), the gradient norm and the
 * accumulation leave it out, rs_trainer_get_grad / _get_accum on it fail with RS_ESTATE, and the
 * backward launches none of its gradient kernels: layers below the lowest one with a trainable
 * tensor run no backward at all unless an embedding tensor is trainable.  Gradients and updates of
 * the trainable tensors are bitwise those of the all-trainable step.  A step with update >= 0 while
 * every tensor is frozen is RS_ESTATE, raised before any state (dropout counter included) moves. */
int rs_trainer_set_trainable(rs_trainer* t, const char* hf_key_prefix, int32_t trainable);
int rs_trainer_is_trainable(const rs_trainer* t, const char* hf_key);   /* 1 / 0 / negative error */
/* acc = fmaf(weight, g, acc) over the trainable tensors, g the gradient of the last step (run with
 * update = 0), enqueued on `stream`.  The accumulator is one more flat fp32 buffer (4 bytes per
 * parameter), allocated and zeroed at the first call (RS_ENOMEM if it does not fit).  Micro-batches
 * add in the order of the calls: bitwise reproducible.  RS_ESTATE before any backward. */
int rs_trainer_accumulate(rs_trainer* t, float weight, void* stream);
int rs_trainer_zero_accum(rs_trainer* t);
/* Synchronous copy of one tensor of the accumulator (RS_ESTATE while it is empty). */
int rs_trainer_get_accum(rs_trainer* t, const char* hf_key, void* host_out, int64_t numel);
typedef struct rs_apply_opts {
    int32_t source;        /* 0: the last step's gradient; 1: the accumulator */
    float grad_scale;      /* the gradient is grad_scale * source (1/k, 1/sum n_i, ...) */
    float max_grad_norm;   /* <= 0: no clipping */
} rs_apply_opts;
/* One AdamW step (opts: lr, betas, eps, weight_decay; opts->update is not read) on the gradient
 * grad_scale * source, clipped like torch's clip_grad_norm_: n = the float64 norm of that gradient
 * over the trainable tensors, c = min(1, max_grad_norm / (n + 1e-6)), and the update uses
 * (float)(grad_scale * c) * source, the product rounded to fp32 once per element.  *h_norm = n (before
 * clipping), *h_applied = 1; both nullable.  A non-finite n skips the step: no parameter, moment
 * or step count moves, *h_applied = 0, RS_OK.  source = 1 clears the accumulator either way.
 * After a step with update = 0, {source 0, grad_scale 1, max_grad_norm 0} leaves parameters, moments
 * and step count exactly as that step with update = 1 would have.  RS_ESTATE for source 0 before
 * any backward and for source 1 on an empty accumulator.  Synchronises `stream`. */
int rs_trainer_apply(rs_trainer* t, const rs_train_opts* opts, const rs_apply_opts* a, double* h_norm,
                     int32_t* h_applied, void* stream);
/* *h_norm = sqrt(sum g^2) over the trainable tensors of the source, in float64: each fp32 square is
 * exact, and the sum is a fixed two-stage ordered reduction without atomics (the same buffer gives
 * the same bits on every run and every device).  Synchronises `stream`. */
int rs_trainer_grad_norm(rs_trainer* t, int32_t source, double* h_norm, void* stream);
/* A fresh AdamW state (moments and step count zeroed; MLM_PLL/main.py:76 builds its
 * optimizer inside every epoch). */
int rs_trainer_reset_optimizer(rs_trainer* t);
void rs_trainer_destroy(rs_trainer* t);

/* RMBR mbr_decode scores for top-k (RMBR/mbr.py:17-22):
 *   score[u][i] = float32 torch-CPU-order sum over j != i (j < k) of
 *                 float32(1 - ed(hyp_j, hyp_i) / len(hyp_j));  argmax[u] = first max.
 * d_len int32 [n_str]; d_scores float32 [n_utt * k]; d_argmax int32 [n_utt]. */
int rs_mbr_scores(const int32_t* d_ed, const int64_t* d_mat_off, const int32_t* d_utt_off,
                  const int32_t* d_len, int32_t n_utt, int32_t k, float* d_scores,
                  int32_t* d_argmax, void* stream);

/* Fusion + argmax over a weight grid (rescore.py:37-58), fp64 with the reference's
 * operation order, no contraction.  Utterance u has hypotheses utt_off[u]..utt_off[u+1]
 * (first n_best of them used).  d_argmax int32 [n_w * n_utt] (first max). */
int rs_fuse_rerank(const double* d_am, const double* d_lm, const int32_t* d_len,
                   const int32_t* d_utt_off, int32_t n_utt, int32_t n_best, const double* d_w,
                   int32_t n_w, int32_t mode, int32_t* d_argmax, void* stream);

/* Corpus-CER numerators for every weight (jiwer.cer at rescore.py:40): edits[w] =
 * sum_u ed_ref[utt_off[u] + argmax[w][u]] over d_ed_ref int32 [n_hyp] (edit distance of
 * each hypothesis to its reference).  d_edits int64 [n_w]. */
int rs_corpus_edits(const int32_t* d_ed_ref, const int32_t* d_utt_off, const int32_t* d_argmax,
                    int32_t n_utt, int32_t n_w, int64_t* d_edits, void* stream);

/* Edit distance of every hypothesis to its utterance's reference (the per-hypothesis
 * table behind jiwer.cer's numerator): d_ref_chars/d_ref_off int32 [n_utt+1] are the
 * references, hypotheses as in rs_pairwise_edit (any number per utterance; the same length
 * limit).  d_ed_ref int32 [n_hyp]. */
int rs_ref_edit(const int32_t* d_chars, const int32_t* d_str_off, const int32_t* d_utt_off,
                const int32_t* d_ref_chars, const int32_t* d_ref_off, int32_t n_utt,
                int32_t* d_ed_ref, void* stream);

/* ---- Native host front end (host-only, no GPU) ------------------------
 * Replaces the tokenizer calls of MLM_PLL/preprocess.py:9-30 (BertTokenizer.tokenize +
 * convert_tokens_to_ids per hypothesis text) and RescoreBert/preprocess.py:8-55, and the
 * score writer util/saving.py:14-16. */

/* Load a BERT vocab.txt (one token per line, id = line index, later duplicates win).
 * Returns an opaque handle or NULL (rs_last_error-style message not set: path unreadable). */
void* rs_vocab_load(const char* path);
int rs_vocab_size(const void* vocab);
void rs_vocab_free(void* vocab);

/* out[i] = 1 where the vocabulary entry of ids[i] starts with "##" (a WordPiece continuation piece:
 * the token continues the word of the token before it), else 0; ids outside [0, size) give 0.
 * ids int32 [n], out uint8 [n].  A word of the tokenised text begins at every token whose flag is
 * 0 ([CLS], [SEP] and [UNK] included): the word boundaries rs_pll_score_spans' word variants mask
 * by.  Returns 0, or -1 on bad arguments. */
int rs_vocab_continuation(const void* vocab, const int32_t* ids, int64_t n, uint8_t* out);

/* BertTokenizer(vocab, do_lower_case=True).tokenize + convert_tokens_to_ids for n NFC UTF-8
 * texts, optionally wrapped in [CLS] .. [SEP] (add_special != 0): the ragged token layout
 * rs_pll_score / rs_cls_score consume.  ids int32 [cap], off int64 [n+1].  Returns the total
 * id count (> cap: only the first cap ids were written; call again with a larger buffer),
 * or < 0 on bad arguments. */
int64_t rs_tokenize_batch(const void* vocab, const char* const* texts, int32_t n, int32_t add_special,
                          int32_t* ids, int64_t cap, int64_t* off);

/* {utt_id: {hyp_id: score}} written byte-identical to json.dump(obj, f, indent=4,
 * ensure_ascii=False) (util/saving.py:14-16); hyp_off int32 [n_utt+1] indexes hyp_ids and
 * scores (float64, Python repr formatting).  Returns 0 or -1 (file not writable). */
int rs_json_write_scores(const char* path, int32_t n_utt, const char* const* utt_ids,
                         const int32_t* hyp_off, const char* const* hyp_ids, const double* scores);

#ifdef __cplusplus
}
#endif
#endif /* RESCORE_H_ */
