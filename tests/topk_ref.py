"""Reference and checkers for the decoder's top-k form (a plain module, imported by name):
tests/test_gpu_topk.py, checked on the CPU in tests/test_topk_ref.py.

The operands are tail_ref's decoder families plus ``ties``.  The reference logits are
z = A.W[:V]^T + b[:V] on the values the fp16 operands hold, in float64 (the reference) and float32
(the yardstick): per row e32 = max_c |z32 - z64| and bound = 4 max(e32, 2^-23 max_c |z64|), the
project's rule.  Three checkers, none of which excludes a row:

  check_values    every returned id is distinct and in [0, V), its log-prob is within the log-prob
                  bound of the float64 log-prob OF THAT ID, log-probs are non-increasing;
  check_complete  no column outside the returned set beats the weakest returned one by more than
                  2 bound (float64 logits);
  check_exact     on "clear" rows — every gap between consecutive float64 logits among the top k + 1
                  exceeds 2 bound, so float64 decides the order — the ids equal topk_ref(z64, k).

All three raise AssertionError with the first offending row.
"""
import torch

import tail_ref as R

FAMILIES = R.DECODER_FAMILIES + ("ties",)
EPS32 = 2.0 ** -23


def operands(family, M, V, K, W, seed=0, device="cpu"):
    """tail_ref.decoder_operands, plus the family ``ties``: A = 0 and b[c] = 1 where c % 97 == 3,
    else 0 (pad columns poisoned as usual), so the logits are exactly the bias and the order is
    decided by the tie rule alone: columns 3, 100, 197, ... then the lowest remaining columns."""
    if family != "ties":
        return R.decoder_operands(family, M, V, K, W, seed, device)
    vpad = W.shape[0]
    A = torch.zeros(M, K, dtype=torch.float16, device=device)
    b = torch.where(torch.arange(vpad, device=device) % 97 == 3, 1.0, 0.0).float()
    b[V:] = R.POISON_BIAS
    return A.contiguous(), b.contiguous(), R.decoder_labels(M, V, vpad, seed, device)


def ties_expected(V, k):
    """The ids every row of the ``ties`` family must return."""
    ones = [c for c in range(V) if c % 97 == 3]
    zeros = [c for c in range(V) if c % 97 != 3]
    return (ones + zeros)[:k]


def topk_ref(z, k):
    """ids [M, k] of a stable sort of every row of z by (-logit, column)."""
    return torch.sort(-z, dim=1, stable=True).indices[:, :k]


class Ref:
    """The float64 reference of one operand set and the per-row bounds (computed once, read only)."""

    def __init__(self, A, W, b, V):
        self.V = V
        z64 = A.double() @ W[:V].double().t() + b[:V].double()
        z32 = A.float() @ W[:V].float().t() + b[:V].float()
        self.z = z64
        self.e32 = (z32.double() - z64).abs().max(dim=1).values
        self.bound = 4 * torch.maximum(self.e32, EPS32 * z64.abs().max(dim=1).values)          # logits, per row
        self.lse = torch.logsumexp(z64, dim=1)
        self.lp = z64 - self.lse[:, None]
        lp32 = z32 - torch.logsumexp(z32, dim=1)[:, None]
        self.e32_lp = (lp32.double() - self.lp).abs().max(dim=1).values

    @classmethod
    def from_logprobs(cls, lp64, bound):
        """A reference given as float64 log-probs [M, V] (a model oracle's) with the caller's per-row
        bound [M] on them: the selection is shift-invariant, so the log-probs stand in for the logits."""
        self = object.__new__(cls)
        self.V = lp64.shape[1]
        self.z = self.lp = lp64
        self.bound = bound
        return self

    def lp_bound(self, ids):
        """[m, k]: 4 max(e32 of the row's log-probs, 2^-23 max(|logit of the id|, |lse|))."""
        m = ids.shape[0]
        zi = self.z[:m].gather(1, ids.long())
        return 4 * torch.maximum(self.e32_lp[:m, None], EPS32 * torch.maximum(zi.abs(), self.lse[:m, None].abs()))

    def clear_rows(self, k):
        """Rows whose top min(k + 1, V) float64 logits are pairwise more than 2 bound apart."""
        top = torch.sort(self.z, dim=1, descending=True).values[:, :min(k + 1, self.V)]
        return ((top[:, :-1] - top[:, 1:]) > 2 * self.bound[:, None]).all(dim=1)


def _first(bad):
    return int(torch.nonzero(bad.reshape(bad.shape[0], -1).any(dim=1))[0])


def check_values(ids, lp, ref, lp_bound=None):
    """ids int [m, k], lp float32 [m, k] of rows [0, m) of ref.  lp_bound: another [m, k] / scalar
    bound on the log-probs (the product tests' relative one)."""
    m, k = ids.shape
    ids = ids.long()
    bad = (ids < 0) | (ids >= ref.V)
    assert not bad.any(), f"row {_first(bad)}: id outside [0, {ref.V}): {ids[_first(bad)].tolist()}"
    srt = torch.sort(ids, dim=1).values
    dup = srt[:, 1:] == srt[:, :-1]
    assert not dup.any(), f"row {_first(dup)}: duplicate id: {ids[_first(dup)].tolist()}"
    assert torch.isfinite(lp).all(), "non-finite log-prob"
    inc = lp[:, 1:] > lp[:, :-1]
    assert not inc.any(), f"row {_first(inc)}: log-probs increase: {lp[_first(inc)].tolist()}"
    err = (lp.double() - ref.lp[:m].gather(1, ids)).abs()
    bound = ref.lp_bound(ids) if lp_bound is None else lp_bound
    over = err > bound
    assert not over.any(), (f"row {_first(over)}: log-prob off by {err[_first(over)].max().item():.3e}, "
                            f"bound {torch.as_tensor(bound).min().item():.3e}")
    return float((err / bound).max()) if m else 0.0


def check_complete(ids, ref, margin=None):
    """margin: [m] / scalar in place of 2 bound."""
    m, k = ids.shape
    ids = ids.long()
    z = ref.z[:m]
    weakest = z.gather(1, ids).min(dim=1).values
    rest = z.clone()
    rest.scatter_(1, ids, float("-inf"))
    mg = 2 * ref.bound[:m] if margin is None else margin
    miss = rest > (weakest + mg)[:, None]
    if miss.any():
        r = _first(miss)
        c = int(torch.nonzero(miss[r])[0])
        raise AssertionError(f"row {r}: column {c} (logit {z[r, c].item():.9g}) is missing, weakest returned "
                             f"{weakest[r].item():.9g}")


def check_exact(ids, ref):
    """Returns the share of clear rows (among the m rows given)."""
    m, k = ids.shape
    clear = ref.clear_rows(k)[:m]
    want = topk_ref(ref.z[:m], k)
    bad = (ids.long() != want) & clear[:, None]
    assert not bad.any(), (f"clear row {_first(bad)}: ids {ids[_first(bad)].tolist()} != float64 order "
                           f"{want[_first(bad)].tolist()}")
    return float(clear.double().mean()) if m else 1.0
