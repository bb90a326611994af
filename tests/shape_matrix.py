"""The accepted-shape matrix of the whole-model parity tests (tests/test_gpu_shapes.py,
tests/test_gpu_shapes_train.py) and its CPU oracles.  A helper module, not a conftest: it imports
without a GPU and every oracle is computed once per shape and never modified.

check_bert_shape (csrc/host_util.h) accepts hidden 256 / 512 / 768 / 1024 with heads = hidden / 64, any
intermediate that is a multiple of 128 (scorer) or 4 (trainer) and any layers >= 1; the rest of the
suite runs BERT_BASE and BERT_TINY end to end.  The shapes here are the smallest models that reach the
host code those two never reach:

    id      vocab  hidden/heads  layers  intermediate  exists for
    h512    1100   512 / 8       3       2048          gangs of 2, odd layer count, decoder on the 256 x 128 tile
    h1024   1000   1024 / 16     2       4096          gangs of 4, attn_fold_kernel<4>
    f640    1000   256 / 4       2       640           F % 256 != 0 fallback forms
    h768n   1000   768 / 12      2       1024          F != 4 H at the production hidden size
    l1      1000   256 / 4       1       1024          last layer = first layer
    t1000   1000   256 / 4       2       1000          F % 4 only (trainer only)

max_pos is 96 everywhere (small tables; no test here needs longer sequences).

Weights: make_weights(shape, seed=5, with_cls_linear=True, with_pooler=True).  Scorer inputs:
data.synthetic_nbest(4, 6, seed=2, vocab, len_lo=1, len_hi=70): 1042 masked sequences, 49762 token rows.
Its four utterances draw base lengths 60, 42, 33 and 42, so T runs from 31 to 63: both sides of the 48-key
attention boundary, none past 64 keys and none short.  The "edges" inputs add what it lacks, one utterance
of L = 1, 63 and 70 (T = 3, 65, 72: the shortest row, the first past 64 keys, and the longest the trainer
batch also holds), scored in calls of their own with their own e32.

Oracles: oracle.bert_ref.TorchBert in fp32 and the same class on the weights cast to float64 (it runs
unchanged on float64 arrays), one hypothesis' masked copies per forward (no padding: a padded key has
probability exactly 0 in the reference, so the values are those of its padded batches).  e32, the fp32
oracle's error against the float64 one on the same inputs, is the yardstick of the fp16x3 rule

    err <= 4 max(e32, 2^-23 max |ref|)

for rows (absolute) and for the PLL.  Measured on the CPU: e32 on rows 1.9e-6 .. 5.7e-6 absolute, on the
PLL 2.4e-8 .. 7.9e-8 relative; |row| >= 3.09 everywhere.
"""
import functools

import numpy as np
import torch

from asr_rescoring_amd import data as D
from asr_rescoring_amd.weights import BertShape, make_weights

MAX_POS = 96
SHAPES = {
    "h512": BertShape(vocab=1100, hidden=512, heads=8, layers=3, intermediate=2048, max_pos=MAX_POS),
    "h1024": BertShape(vocab=1000, hidden=1024, heads=16, layers=2, intermediate=4096, max_pos=MAX_POS),
    "f640": BertShape(vocab=1000, hidden=256, heads=4, layers=2, intermediate=640, max_pos=MAX_POS),
    "h768n": BertShape(vocab=1000, hidden=768, heads=12, layers=2, intermediate=1024, max_pos=MAX_POS),
    "l1": BertShape(vocab=1000, hidden=256, heads=4, layers=1, intermediate=1024, max_pos=MAX_POS),
    "t1000": BertShape(vocab=1000, hidden=256, heads=4, layers=2, intermediate=1000, max_pos=MAX_POS),
}
SCORER_IDS = ["h512", "h1024", "f640", "h768n", "l1"]
TRAINER_IDS = ["h512", "h1024", "f640", "l1", "t1000"]
PRECISIONS = ["fp16x3", "fp16"]
REL = 1e-3                    # the north-star tolerance of tests/test_gpu_bert.py
X3_FACTOR = 4.0               # fp16x3: err <= X3_FACTOR * max(e32, 2^-23 max |ref|)


@functools.lru_cache(maxsize=None)
def weights(sid):
    return make_weights(SHAPES[sid], seed=5, with_cls_linear=True, with_pooler=True)


@functools.lru_cache(maxsize=None)
def _inputs(vocab):
    return D.synthetic_nbest(4, 6, seed=2, vocab=vocab, len_lo=1, len_hi=70)


def inputs(sid):
    """The scorer N-best of a shape (one per vocabulary size)."""
    return _inputs(SHAPES[sid].vocab)


EDGE_L = (1, 63, 70)


@functools.lru_cache(maxsize=None)
def _edge_inputs(vocab):
    rng = np.random.default_rng(72)
    return D.from_lists([[rng.integers(D.FIRST_WORD_ID, vocab, size=L).tolist() for L in EDGE_L]], [[0.0] * len(EDGE_L)])


def edge_inputs(sid):
    """One utterance of L = 1, 63, 70 (T = 3, 65, 72): the lengths ``inputs`` does not hold."""
    return _edge_inputs(SHAPES[sid].vocab)


@functools.lru_cache(maxsize=None)
def _train_inputs(vocab):
    return D.synthetic_nbest(3, 6, seed=3, vocab=vocab, len_lo=1, len_hi=40)


def train_inputs(sid):
    """The trainer batch of a shape: (NBest, sequences, target, am, cer), 3 utterances of 6."""
    nb = _train_inputs(SHAPES[sid].vocab)
    rng = np.random.default_rng(3)
    target = rng.normal(-1.0, 1.0, nb.n_hyp).astype(np.float32)
    cer = (rng.integers(0, 5, nb.n_hyp) / 10.0).astype(np.float32)
    return nb, seqs_of(nb), target, nb.am.astype(np.float32), cer


def seqs_of(nb):
    return [nb.tokens[nb.hyp_off[h]:nb.hyp_off[h + 1]].tolist() for h in range(nb.n_hyp)]


def token_rows(nb):
    """Encoder rows of a PLL call: every hypothesis of L words is L masked copies of T = L + 2 tokens."""
    T = np.diff(nb.hyp_off).astype(np.int64)
    return int(((T - 2) * T).sum())


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


def py_sum(vals, off):
    """Python float64 += of vals[off[h]:off[h + 1]] in order (MLM_PLL/main.py:105-107)."""
    out = np.zeros(len(off) - 1, np.float64)
    for h in range(len(out)):
        acc = 0.0
        for x in vals[off[h]:off[h + 1]]:
            acc += float(x)
        out[h] = acc
    return out


@functools.lru_cache(maxsize=None)
def model(sid, dtype):
    """TorchBert on the shape's weights in ``dtype`` ("float32" / "float64")."""
    from oracle.bert_ref import TorchBert, set_cpu_threads
    set_cpu_threads()
    return TorchBert({k: np.asarray(v, dtype) for k, v in weights(sid).items()}, SHAPES[sid])


def _r16(t):
    return t.half().to(t.dtype)


@functools.lru_cache(maxsize=None)
def model_fp16_operands(sid):
    """The yardstick of the fp16 mode where a shape misses the 1e-3 rules: the float64 oracle with the
    operands (input and weight) of every Linear rounded to fp16 (the encoder's projections, the MLM
    transform and tied decoder, the CLS head), everything else in float64."""
    import torch.nn.functional as Fn
    from oracle.bert_ref import TorchBert

    class Fp16OperandBert(TorchBert):
        def _lin(self, x, key):
            return Fn.linear(_r16(x), self.w16[key + ".weight"], self.w[key + ".bias"])

        def mlm_logits(self, hidden):
            c = "cls.predictions."
            t = self._ln(Fn.gelu(self._lin(hidden, c + "transform.dense")), c + "transform.LayerNorm")
            return Fn.linear(_r16(t), self.w16["bert.embeddings.word_embeddings.weight"], self.w[c + "bias"])

        def cls_score(self, hidden):
            return Fn.linear(_r16(hidden[:, 0, :]), self.w16["linear.weight"], self.w["linear.bias"]).squeeze(-1)

    base = model(sid, "float64")
    tb = Fp16OperandBert({}, SHAPES[sid])
    tb.w = base.w
    tb.w16 = {k: _r16(v) for k, v in base.w.items() if k.endswith("weight") and v.dim() == 2}
    return tb


def _row_logprobs(tb, nb):
    """log_softmax (in the model's dtype) of the logits at the masked position of every do_job row:
    [R, vocab], rows hypothesis by hypothesis, position by position."""
    out = []
    with torch.no_grad():
        for h in range(nb.n_hyp):
            seq = torch.from_numpy(nb.tokens[nb.hyp_off[h]:nb.hyp_off[h + 1]].astype(np.int64))
            L = len(seq) - 2
            ids = seq[None, :].repeat(L, 1)
            r = torch.arange(L)
            ids[r, r + 1] = tb.s.mask_id
            hid = tb.encoder(ids, torch.ones_like(ids))
            out.append(tb.mlm_logits(hid[r, r + 1, :]).log_softmax(dim=-1))
    return torch.cat(out)


class Oracle:
    """Both oracles of one scorer shape on its inputs.  rows*: the label's log-prob per masked row
    (the fp32 oracle's in float32, as the reference holds it); pll*: their Python float64 sums;
    lp64: [R, vocab] float64 log-probs of the float64 oracle; cls32 / cls64: CLS scores per hypothesis."""

    def __init__(self, sid, which="main"):
        nb = inputs(sid) if which == "main" else edge_inputs(sid)
        self.sid, self.nb = sid, nb
        L = np.diff(nb.hyp_off) - 2
        self.row_off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
        lab = torch.from_numpy(np.concatenate([nb.tokens[nb.hyp_off[h] + 1:nb.hyp_off[h + 1] - 1]
                                               for h in range(nb.n_hyp)]).astype(np.int64))
        lp32 = _row_logprobs(model(sid, "float32"), nb)
        self.lp64 = _row_logprobs(model(sid, "float64"), nb)
        r = torch.arange(len(lab))
        self.labels = lab.numpy()
        self.rows32 = lp32[r, lab].numpy()
        self.rows64 = self.lp64[r, lab].numpy()
        assert self.rows32.dtype == np.float32 and self.rows64.dtype == np.float64
        self.pll32, self.pll64 = py_sum(self.rows32, self.row_off), py_sum(self.rows64, self.row_off)
        self.e32_rows = float(np.abs(self.rows32.astype(np.float64) - self.rows64).max())
        self.e32_pll = float(np.abs(self.pll32 - self.pll64).max())
        self.cls32, self.cls64 = (self._cls(model(sid, d)) for d in ("float32", "float64"))

    def _cls(self, tb):
        out = []
        with torch.no_grad():
            for s in seqs_of(self.nb):
                ids = torch.tensor([s], dtype=torch.long)
                out.append(float(tb.cls_score(tb.encoder(ids, torch.ones_like(ids)))[0]))
        return np.asarray(out, np.float64)

    @functools.cached_property
    def e16_cls(self):
        """Error of the fp16-operand emulation's CLS scores against the float64 oracle (on first use)."""
        return float(np.abs(self._cls(model_fp16_operands(self.sid)) - self.cls64).max())

    @functools.cached_property
    def e16_lp(self):
        """The same for the log-probs of every masked row, over the whole vocabulary (on first use)."""
        return float((_row_logprobs(model_fp16_operands(self.sid), self.nb) - self.lp64).abs().max())

    def x3_bound(self, what):
        """The fp16x3 rule's bound for "rows" or "pll" (absolute)."""
        e32, ref = (self.e32_rows, self.rows64) if what == "rows" else (self.e32_pll, self.pll64)
        return X3_FACTOR * max(e32, 2.0 ** -23 * float(np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def _oracle(sid, which):
    return Oracle(sid, which)


def oracle(sid, which="main"):
    """The oracles of a shape on ``inputs`` ("main") or ``edge_inputs`` ("edges"), computed once."""
    return _oracle(sid, which)


def padded_rows(nb, mask_id):
    """The do_job rows of an N-best as a padded batch: (input_ids, attention_mask int64 [R, Tmax], mask_pos)."""
    from oracle.bert_ref import _pad, pll_rows
    rows = list(pll_rows(nb.tokens, nb.hyp_off, mask_id))
    return _pad([r[1] for r in rows]), _pad([[1] * len(r[1]) for r in rows]), [r[2] for r in rows]


def sets_plan(nb):
    """Multi-mask rows with two and three masked positions: a hypothesis of L >= 3 words gets the rows
    [1, L] and [1, (L + 1) // 2, L], one of L = 2 the row [1, 2], one of L = 1 none (its PLL is 0.0).
    Returns (row_off, pos_off, pos) as PLLScorer.score_sets takes them."""
    row_off, pos_off, pos = [0], [0], []
    for h in range(nb.n_hyp):
        L = int(nb.hyp_off[h + 1] - nb.hyp_off[h]) - 2
        rows = [[1, L], [1, (L + 1) // 2, L]] if L >= 3 else [[1, 2]] if L == 2 else []
        for r in rows:
            pos += r
            pos_off.append(len(pos))
        row_off.append(len(pos_off) - 1)
    return tuple(np.asarray(x, np.int32) for x in (row_off, pos_off, pos))


def sets_rows(nb, plan, mask_id):
    """One host-masked row per multi-mask row of ``plan``: padded (input_ids, attention_mask, labels)
    int64 [n_rows, Tmax] (labels -100 off the masked positions) and each row's position list."""
    row_off, pos_off, pos = plan
    hyp = np.repeat(np.arange(nb.n_hyp), np.diff(row_off))
    tmax = int(np.diff(nb.hyp_off).max())
    n = len(pos_off) - 1
    ids, am = np.zeros((n, tmax), np.int64), np.zeros((n, tmax), np.int64)
    lab = np.full((n, tmax), -100, np.int64)
    qpos = []
    for r in range(n):
        seg = nb.tokens[nb.hyp_off[hyp[r]]:nb.hyp_off[hyp[r] + 1]]
        p = pos[pos_off[r]:pos_off[r + 1]]
        ids[r, :len(seg)], am[r, :len(seg)] = seg, 1
        lab[r, p] = seg[p]
        ids[r, p] = mask_id
        qpos.append([int(x) for x in p])
    return ids, am, lab, qpos


def sets_logprobs(tb, ids, am, qpos):
    """log_softmax (model dtype) at every masked position of the rows of ``sets_rows``, in list order:
    [n_pos, vocab]."""
    with torch.no_grad():
        hid = tb.encoder(torch.from_numpy(ids), torch.from_numpy(am))
        rows = [r for r, ps in enumerate(qpos) for _ in ps]
        return tb.mlm_logits(hid[rows, [p for ps in qpos for p in ps], :]).log_softmax(dim=-1)
