"""ctypes binding of ``librescore.so`` (declared in ``include/rescore.h``).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  ``torch`` is
imported first so that the HIP runtime ``librescore.so`` links against is the one torch
already loaded (both carry the soname ``libamdhip64.so.7``): device pointers and the
``hipStream_t`` of ``torch.cuda.current_stream()`` are then valid inside the library.
There is no CPU fallback: a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must load torch's HIP runtime before librescore.so)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# RS_LIBRESCORE: another in-tree build of the same library (A/B timing of two builds in one GPU
# session); default the library build.py writes.  The override is announced on stderr.
LIB_PATH = os.environ.get("RS_LIBRESCORE") or os.path.join(PKG_DIR, "librescore.so")

RS_HEAD_MLM, RS_HEAD_CLS, RS_HEAD_EMB = 1, 2, 4
RS_FUSE = {"norm": 0, "legacy": 1, "am_norm": 2}
KINDS = ["qkv", "oproj", "ffn1", "ffn2", "decoder", "attn", "other"]


class RsBertCfg(ctypes.Structure):
    _fields_ = [("vocab", ctypes.c_int32), ("hidden", ctypes.c_int32), ("layers", ctypes.c_int32),
                ("heads", ctypes.c_int32), ("intermediate", ctypes.c_int32),
                ("max_pos", ctypes.c_int32), ("type_vocab", ctypes.c_int32),
                ("ln_eps", ctypes.c_float), ("mask_id", ctypes.c_int32),
                ("heads_mask", ctypes.c_int32), ("precision", ctypes.c_int32)]


RS_PREC = {"fp16": 0, "fp16x3": 1}
RS_LOSS = {"MD": 0, "MD_MWER": 1, "MD_MWED": 2}


class RsTrainOpts(ctypes.Structure):
    _fields_ = [("loss", ctypes.c_int32), ("md_loss_weight", ctypes.c_float), ("lr", ctypes.c_float),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("update", ctypes.c_int32),
                ("hidden_dropout", ctypes.c_float), ("attn_dropout", ctypes.c_float),
                ("dropout_seed", ctypes.c_uint32)]


class RsApplyOpts(ctypes.Structure):
    _fields_ = [("source", ctypes.c_int32), ("grad_scale", ctypes.c_float), ("max_grad_norm", ctypes.c_float)]


class RescoreError(RuntimeError):
    """A failed library call; ``code`` is the RS_E* value (``RS_ESTATE`` = -3, ...)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


_lib = None
P = ctypes.c_void_p
I32, I64 = ctypes.c_int32, ctypes.c_int64

_SIGS = {
    "rs_version": (ctypes.c_int, []),
    "rs_last_error": (ctypes.c_char_p, []),
    "rs_model_create": (ctypes.c_int, [ctypes.POINTER(RsBertCfg), ctypes.c_int, ctypes.POINTER(P)]),
    "rs_model_set_tensor": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int, ctypes.POINTER(I64), ctypes.c_int]),
    "rs_model_finalize": (ctypes.c_int, [P]),
    "rs_model_reserve": (ctypes.c_int, [P, I64]),
    "rs_pll_score": (ctypes.c_int, [P, P, P, I32, P, P, P]),
    "rs_pll_score_spans": (ctypes.c_int, [P, P, P, I32, P, P, P, P, P, P, P]),
    "rs_pll_score_sets": (ctypes.c_int, [P, P, P, I32, P, P, P, P, P, P]),
    "rs_masked_logprob_multi": (ctypes.c_int, [P, P, P, I32, P, P, P, P, P]),
    # (m, d_ids, h_seq_off, n_seq, h_q_off, h_qpos, h_c_off, h_cand, d_out, stream)
    "rs_masked_logprob_cands": (ctypes.c_int, [P, P, P, I32, P, P, P, P, P, P]),
    "rs_masked_logprob": (ctypes.c_int, [P, P, P, P, P, I32, P, P]),
    "rs_masked_topk": (ctypes.c_int, [P, P, P, P, I32, I32, P, P, P]),
    "rs_pll_topk": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, P, P]),
    "rs_cls_score": (ctypes.c_int, [P, P, P, I32, P, P]),
    "rs_profile_enable": (ctypes.c_int, [P, ctypes.c_int]),
    "rs_profile_read": (ctypes.c_int, [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(I64), ctypes.POINTER(ctypes.c_double)]),
    "rs_model_set_sync_check": (ctypes.c_int, [P, ctypes.c_int]),
    "rs_check": (ctypes.c_int, [P, P]),
    "rs_model_set_token_types": (ctypes.c_int, [P, P, I64]),
    "rs_model_destroy": (None, [P]),
    "rs_pairwise_edit": (ctypes.c_int, [P, P, P, P, I32, I32, P, P]),
    "rs_mbr_scores": (ctypes.c_int, [P, P, P, P, I32, I32, P, P, P]),
    "rs_mbr_scores_bs": (ctypes.c_int, [P, P, P, I32, I32, I32, P, P, P]),
    "rs_token_embed": (ctypes.c_int, [P, P, P, I32, P, P]),
    "rs_trainer_create": (ctypes.c_int, [ctypes.POINTER(RsBertCfg), ctypes.c_int, ctypes.POINTER(P)]),
    "rs_trainer_set_tensor": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int, ctypes.POINTER(I64), ctypes.c_int]),
    "rs_trainer_finalize": (ctypes.c_int, [P]),
    "rs_train_step_cls": (ctypes.c_int, [P, P, P, I32, P, I32, P, P, P, ctypes.POINTER(RsTrainOpts), P, P, P]),
    "rs_train_step_mlm": (ctypes.c_int, [P, P, P, I32, P, P, ctypes.POINTER(RsTrainOpts), P, P]),
    "rs_train_step_mlm_labeled": (ctypes.c_int, [P, P, P, I32, P, P, I32, P, ctypes.POINTER(RsTrainOpts), P, P]),
    "rs_trainer_get_tensor": (ctypes.c_int, [P, ctypes.c_char_p, P, I64]),
    "rs_trainer_get_grad": (ctypes.c_int, [P, ctypes.c_char_p, P, I64]),
    "rs_trainer_set_trainable": (ctypes.c_int, [P, ctypes.c_char_p, I32]),
    "rs_trainer_is_trainable": (ctypes.c_int, [P, ctypes.c_char_p]),
    "rs_trainer_accumulate": (ctypes.c_int, [P, ctypes.c_float, P]),
    "rs_trainer_zero_accum": (ctypes.c_int, [P]),
    "rs_trainer_get_accum": (ctypes.c_int, [P, ctypes.c_char_p, P, I64]),
    "rs_trainer_apply": (ctypes.c_int, [P, ctypes.POINTER(RsTrainOpts), ctypes.POINTER(RsApplyOpts),
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(I32), P]),
    "rs_trainer_grad_norm": (ctypes.c_int, [P, I32, ctypes.POINTER(ctypes.c_double), P]),
    "rs_trainer_reset_optimizer": (ctypes.c_int, [P]),
    "rs_trainer_set_token_types": (ctypes.c_int, [P, P, I64]),
    "rs_trainer_dropout_step": (I64, [P]),
    "rs_trainer_set_dropout_step": (ctypes.c_int, [P, I64]),
    "rs_dropout_keep": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, I64, P, P]),
    "rs_trainer_destroy": (None, [P]),
    "rs_bertscore_recall": (ctypes.c_int, [P, P, P, P, I32, P, P, P]),
    "rs_align": (ctypes.c_int, [P, P, P, P, I32, P, P, P, P, P, P, P, I32, P]),
    "rs_cn_merge": (ctypes.c_int, [P, P, P, P, P, P, I32, I32, P, P, P, P, P, P, I64, I32, P]),
    "rs_cn_oracle": (ctypes.c_int, [P, P, P, P, P, P, I32, I32, P, P, I32, P, P, P, P, P]),
    "rs_cn_vote": (ctypes.c_int, [P, P, P, P, P, P, I32, I32, P, P, P, P, P, P, P]),
    "rs_fuse_rerank": (ctypes.c_int, [P, P, P, P, I32, I32, P, I32, I32, P, P]),
    "rs_corpus_edits": (ctypes.c_int, [P, P, P, I32, I32, P, P]),
    "rs_ref_edit": (ctypes.c_int, [P, P, P, P, P, I32, P, P]),
    "rs_vocab_load": (P, [ctypes.c_char_p]),
    "rs_vocab_size": (ctypes.c_int, [P]),
    "rs_vocab_free": (None, [P]),
    "rs_vocab_continuation": (ctypes.c_int, [P, P, I64, P]),
    "rs_tokenize_batch": (I64, [P, ctypes.POINTER(ctypes.c_char_p), I32, I32, P, I64, P]),
    "rs_json_write_scores": (ctypes.c_int, [ctypes.c_char_p, I32, ctypes.POINTER(ctypes.c_char_p), P,
                                            ctypes.POINTER(ctypes.c_char_p), P]),
}

# Diagnostic / test entries (not declared in include/rescore.h, not part of the scoring path).
# Typed here so that every caller passes 64-bit pointers: an untyped ctypes call converts a Python
# int to a 32-bit C int, and a truncated device pointer faults the kernel that dereferences it
# (the round-5 "interleaved-W" illegal address: a test called rs_debug_gemm untyped).
CI = ctypes.c_int
_DEBUG_SIGS = {
    "rs_debug_gemm": (CI, [CI, CI, P, P, P, P, CI, CI, CI, P]),
    "rs_debug_attention": (CI, [CI, P, P, P, CI, CI, CI, P, P]),
    "rs_debug_ln": (CI, [CI, CI] + [P] * 9),
    "rs_debug_stamps": (CI, [CI, P]),
    "rs_debug_occupy": (CI, [CI, CI, P, P]),
    "rs_debug_sgemm_cfg": (CI, [CI] * 4 + [P, CI, CI, P, CI, CI, P, CI, CI, P]),
    "rs_debug_sgemm": (CI, [CI] * 3 + [P, CI, CI, P, CI, CI, P, CI, CI, P]),
    "rs_debug_sgemm_pick": (CI, [CI] * 5),
    "rs_debug_gelu": (CI, [P, P, CI, P]),
    # (epi, A2, W2, bias, gamma, beta, eps, out, ldc, M_pad, m_valid, N, K, lnx, lncnt, lnerr, stream)
    "rs_debug_x3s": (CI, [CI, P, P, P, P, P, ctypes.c_float, P, CI, CI, CI, CI, CI, P, P, P, P]),
    "rs_debug_lnres_sizes": (CI, [CI, CI, ctypes.POINTER(I64)]),
    # (qkv32, len, row, n_seq, max_len, H, heads, kx, ctx, stream)
    "rs_debug_attention_full": (CI, [P, P, P, CI, CI, CI, CI, CI, P, P]),
    # (epi, A, W, M_pad, N_pad, K, DebugGemmEpi*, stream)
    "rs_debug_gemm_epi": (CI, [CI, P, P, CI, CI, CI, P, P]),
    # (A, W, bias, label, M_pad, m_valid, vpad, vocab, K, lab, part, llog, out, stream)
    "rs_debug_decoder": (CI, [P, P, P, P, CI, CI, CI, CI, CI, P, P, P, P, P]),
    # rs_debug_decoder's arguments up to out, then (k, cand, top_id, top_lp, stream)
    "rs_debug_decoder_topk": (CI, [P, P, P, P, CI, CI, CI, CI, CI, P, P, P, P, CI, P, P, P, P]),
    # (A, W, bias, M_pad, m_valid, vpad, vocab, K, part, c_off, cand_id, perm, cand_logit, out, stream)
    "rs_debug_decoder_cands": (CI, [P, P, P, CI, CI, CI, CI, CI, P, P, P, P, P, P, P]),
    # (qkv, qkv32, len, row, query, s0, s1, row0, H, heads, kx, qd, x32, stats, g, b, himg, ctxq, resq, stream)
    "rs_debug_attention_query": (CI, [P, CI, P, P, P, CI, CI, CI, CI, CI, CI, P, P, P, P, P, P, P, P, P]),
    # (himg, tq, wkf, wvt, bv, len, row, query, s0, s1, row0, H, heads, kx, work, work_bytes, ctxq, resq, stream)
    "rs_debug_attention_fold": (CI, [P, P, P, P, P, P, P, P, CI, CI, CI, CI, CI, CI, P, ctypes.c_longlong, P, P, P]),
    # (form, qkv, seq_off, klen, n_seq, H, heads, dctx, seed, step, site, p, ctx, dqkv, stream)
    "rs_debug_train_attn": (CI, [CI, P, P, P, CI, CI, CI, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                                 ctypes.c_float, P, P, P]),
    # The trainer's other kernels (csrc/k_train.hip, tests/test_gpu_train_ops.py); dropout = (seed, step, site, p)
    # (row_tok, row_pos, row_type, M, vocab, type_vocab, max_pos, word, pos, typetab, g, b, eps, H, dropout,
    #  x0, st, h0, stream)
    "rs_debug_train_embed_ln": (CI, [P, P, P, CI, CI, CI, CI, P, P, P, P, P, ctypes.c_float, CI, ctypes.c_uint32,
                                     ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, P, P, P, P]),
    # (y, bias, res, M, g, b, eps, H, dropout, st, h, stream)
    "rs_debug_train_bias_res_ln": (CI, [P, P, P, CI, P, P, ctypes.c_float, CI, ctypes.c_uint32, ctypes.c_uint64,
                                        ctypes.c_uint32, ctypes.c_float, P, P, P]),
    # (dy, x, st, g, dx, M, H, stream)
    "rs_debug_train_ln_bwd": (CI, [P, P, P, P, P, CI, CI, P]),
    # (op, a, v, c, M, N, stream): 0 bias_gelu(pre, bias, act), 1 gelu_bwd(d, pre), 2 bias(y, bias)
    "rs_debug_train_pointwise": (CI, [CI, P, P, P, CI, CI, P]),
    # (op, dy, x, st, M, N, out, out_b, accumulate, rtype, want, stream): 0 / 1 tr_colsum mode, 2 tr_colsum_ln
    "rs_debug_train_colsum": (CI, [CI, P, P, P, CI, CI, P, P, CI, P, CI, P]),
    # (dx0, utok, toff, rows, n_uniq, M, vocab, H, dword, stream)
    "rs_debug_train_word_grad": (CI, [P, P, P, P, CI, CI, CI, CI, P, P]),
    # (dx0, seq_off, S, M, tmax, H, dpos, stream)
    "rs_debug_train_pos_grad": (CI, [P, P, CI, CI, CI, CI, P, P]),
    # (h, seq_off, S, M, H, w, b, out, stream)
    "rs_debug_train_cls_fwd": (CI, [P, P, CI, CI, CI, P, P, P, P]),
    # (dsc, h, seq_off, S, M, H, w, dh, dw, db, stream)
    "rs_debug_train_cls_bwd": (CI, [P, P, P, CI, CI, CI, P, P, P, P, P]),
    # (sc, tgt, am, cer, utt_off, n_utt, n_hyp, kind, md_w, dsc, uloss, loss, stream)
    "rs_debug_train_loss": (CI, [P, P, P, P, P, CI, CI, CI, ctypes.c_float, P, P, P, P]),
    # (logits, labels, M, V, row_loss, loss, stream)
    "rs_debug_train_ce": (CI, [P, P, CI, CI, P, P, P]),
    # (op, src, idx, n, M, H, dst, stream): 0 gather_rows, 1 expand_rows
    "rs_debug_train_move_rows": (CI, [CI, P, P, CI, CI, CI, P, P]),
    # (p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, stream)
    "rs_debug_train_adamw": (CI, [P, P, P, P, I64] + [ctypes.c_float] * 5 + [I64, P]),
    # (p, g, m, v, n, gmul, lr, beta1, beta2, eps, weight_decay, step, stream)
    "rs_debug_train_adamw_scaled": (CI, [P, P, P, P, I64] + [ctypes.c_float] * 6 + [I64, P]),
    # (acc, g, h_off, h_n, n_ranges, n_total, w, stream): host int64 range lists
    "rs_debug_train_accum": (CI, [P, P, P, P, CI, I64, ctypes.c_float, P]),
    # (g, h_off, h_n, n_ranges, n_total, h_out, stream): h_out host float64 [1]
    "rs_debug_train_sumsq": (CI, [P, P, P, CI, I64, P, P]),
    # The BERTScore kernels without an encoder (tests/test_gpu_bertscore_ops.py)
    # (d_emb, H, two, h_hyp_off, h_utt_off, n_utt, d_rmat, d_rmat0, stream)
    "rs_debug_bertscore_recall": (CI, [P, CI, CI, P, P, CI, P, P, P]),
    # (x32, stats, g, b, himg, len, row, tok_off, s0, s1, row0, H, two, d_out, stream)
    "rs_debug_embed_out": (CI, [P, P, P, P, P, P, P, P, CI, CI, CI, CI, CI, P, P]),
    # The layer-0 front end, dedup / multi-query attention, gathers and small heads
    # (tests/test_gpu_front_ops.py, tests/test_gpu_attn_plan.py); meta = DebugMeta*
    # (tok_off, len, mask, mask_end, n_seq, s0, s1, urow_h, urow_m): host int32 arrays -> urows
    "rs_debug_plan_unique": (CI, [P, P, P, P, CI, CI, CI, P, P]),
    # (form, tok, type, meta, s0, s1, row0, urows, mask_id, vocab, type_vocab, word, pos, typetab, g, b, eps, H,
    #  x32, stats, h16, kx, stream): form 0 embed_ln, 1 embed_ln_set, 2 embed_unique
    "rs_debug_embed": (CI, [CI, P, P, P, CI, CI, CI, CI, CI, CI, CI, P, P, P, P, P, ctypes.c_float, CI, P, P, P, CI, P]),
    # (qkv, qkv32, meta, s0, s1, row0, max_len, H, heads, kx, dedup, ctx, stream)
    "rs_debug_attention_plan": (CI, [P, CI, P, CI, CI, CI, CI, CI, CI, CI, CI, P, P]),
    # (qkv, qkv32, meta, s0, s1, H, heads, kx, qd, x32, stats, g, b, himg, ctxq, resq, stream)
    "rs_debug_attention_mquery": (CI, [P, CI, P, CI, CI, CI, CI, CI, P, P, P, P, P, P, P, P, P]),
    # (op, src, ld, tok, meta, a0, a1, row0, dst, lab, llog, stream): 0 / 1 query rows per sequence / per query,
    # 2 / 3 labels per sequence / per query; (a0, a1) = (s0, s1) or (q0, n)
    "rs_debug_gather": (CI, [CI, P, CI, P, P, CI, CI, CI, P, P, P, P]),
    # (h, rows, H, w, b, out, stream)
    "rs_debug_cls_linear": (CI, [P, CI, CI, P, P, P, P]),
    # (row_lp, off, n, out, stream)
    "rs_debug_segsum": (CI, [P, P, CI, P, P]),
}


class DebugGemmEpi(ctypes.Structure):
    """The EpiArgs fields rs_debug_gemm_epi takes (csrc/k_gemm.hip DebugGemmEpi)."""
    _fields_ = [(n, P) for n in ("bias", "res", "res_stats", "res_g", "res_b", "out", "res_o16", "res_stats0",
                                 "res_g0", "res_b0")] + [(n, CI) for n in ("ldc", "m_valid", "kx", "nlog")]


class DebugMeta(ctypes.Structure):
    """Device int32 metadata arrays of the front-end / attention test entries (csrc/common.h DebugMeta):
    SeqMeta's columns, then QueryMeta's (qlabel = its label).  Unused ones stay null."""
    _fields_ = [(n, P) for n in ("tok_off", "len", "mask_pos", "mask_end", "query", "label", "row", "urow_h", "urow_m",
                                 "first", "seq", "pos", "qlabel")]



EXPORTED = tuple(_SIGS)          # the shipped library's entries (include/rescore.h)
_SIGS.update(_DEBUG_SIGS)


def load(path: str = LIB_PATH):
    """Load and type the library; raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
    if os.environ.get("RS_LIBRESCORE"):
        import sys
        print(f"librescore: RS_LIBRESCORE override {path}", file=sys.stderr)
    lib = ctypes.CDLL(path)
    if not hasattr(lib, "rs_version"):
        raise ImportError(f"{path} is not a librescore build (no rs_version)")
    for name, (res, args) in _SIGS.items():
        if name in _DEBUG_SIGS and not hasattr(lib, name):
            continue                          # RS_DIAG-only entry (rs_debug_stamps) in the shipped build
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise RescoreError(f"librescore error {rc}: {load().rs_last_error().decode()}", rc)


def bert_cfg(shape, heads: int, precision: str = "fp16") -> RsBertCfg:
    """``rs_bert_cfg`` of a ``weights.BertShape`` with a head mask and a precision mode."""
    return RsBertCfg(shape.vocab, shape.hidden, shape.layers, shape.heads, shape.intermediate, shape.max_pos,
                     shape.type_vocab, shape.ln_eps, shape.mask_id, heads, RS_PREC[precision])


def upload_tensors(fn, handle, weights, keys=None) -> None:
    """``fn`` (``rs_model_set_tensor`` / ``rs_trainer_set_tensor``) on every tensor of the HF-keyed
    ``weights`` (only those in ``keys``, when given), as contiguous float32."""
    for k, v in weights.items():
        if keys is not None and k not in keys:
            continue
        a = np.ascontiguousarray(v, dtype=np.float32)
        check(fn(handle, k.encode(), a.ctypes.data, 0, (ctypes.c_int64 * a.ndim)(*a.shape), a.ndim))


def ptr(t) -> int:
    """Device/host pointer of a tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        return t.data_ptr()
    return t.ctypes.data


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
