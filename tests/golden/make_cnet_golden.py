"""Generate ``cnet_merge.json`` by running the REFERENCE's own functions (needs the reference tree).

Run from the repo root:  ``python tests/golden/make_cnet_golden.py <reference dir>``

``new_merge_alignments`` and ``get_feature`` come unmodified from Nbest_Align/preprocess.py and
``levenshtein_distance_alignment`` from espnet_data/preprocess/align.py; the packages preprocess.py
imports but this image lacks or that would need downloads (sklearn, tqdm, jiwer, transformers) are
stubbed as in make_golden.py: jiwer.cer is ``oracle.rescore_ref.corpus_cer`` on characters and
``BertTokenizer.from_pretrained`` returns ``data.CharTokenizer``.  Only outputs are written.

Fixture: {"cases": [{"h": hypotheses, "t": merged table or null where the reference raises IndexError}],
"features": {"charset", "hyps", "refs", "rows"}}.  A hypothesis / slot of one-character tokens is stored
as a string, anything else as a list (``list(x)`` restores both).
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = sys.argv[1] if len(sys.argv) > 1 else sys.exit(__doc__)
OUT = os.path.join(REPO, "tests", "golden", "cnet_merge.json")
sys.path.insert(0, REPO)

from asr_rescoring_amd import data as D          # noqa: E402
from oracle import rescore_ref                   # noqa: E402

FEATURE_CHARS = "abcd*"


def install_stubs():
    sk, skm = types.ModuleType("sklearn"), types.ModuleType("sklearn.metrics")
    skm.max_error = None
    sk.metrics = skm
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, **kw: x
    jw = types.ModuleType("jiwer")
    enc = lambda s: [ord(c) for c in s.strip()]          # noqa: E731
    jw.cer = lambda r, h: rescore_ref.corpus_cer([enc(r)], [enc(h)])
    tr = types.ModuleType("transformers")
    tr.BertTokenizer = types.SimpleNamespace(from_pretrained=lambda name: D.CharTokenizer(FEATURE_CHARS))
    sys.modules.update({"sklearn": sk, "sklearn.metrics": skm, "tqdm": tq, "jiwer": jw, "transformers": tr})


def load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pack(seq):
    return "".join(seq) if all(isinstance(t, str) and len(t) == 1 for t in seq) else list(seq)


def reference_table(pre, al, hyps):
    try:
        als = []
        for h in hyps[1:]:
            a = al.levenshtein_distance_alignment(list(hyps[0]), list(h))
            als.append([[r, t] for r, t in zip(a[0], a[1])])
        merged = als.pop(0)
        for a in als:
            merged = pre.new_merge_alignments(merged, a)
        return merged
    except IndexError:
        return None


def random_lists(rng):
    alphabets = ["ab", "abc", "".join(chr(0x4e00 + k) for k in range(30))]
    out = []
    for i in range(300):
        alpha = alphabets[i % 3]
        n = int(rng.integers(2, 9))
        top = int(rng.integers(0, 9))
        hyps = []
        for _ in range(n):
            ln = 0 if rng.random() < 0.06 else max(0, top + int(rng.integers(-2, 3)))
            hyps.append([alpha[int(c)] for c in rng.integers(0, len(alpha), ln)])
        out.append(hyps)
    # edits of one sequence, as N-best lists are
    for i in range(60):
        alpha = alphabets[2]
        base = [alpha[int(c)] for c in rng.integers(0, 30, int(rng.integers(3, 11)))]
        hyps = [base]
        for _ in range(int(rng.integers(1, 8))):
            h = list(base)
            for _ in range(int(rng.integers(0, 4))):
                k, pos = int(rng.integers(0, 3)), int(rng.integers(0, len(h) + 1))
                if k == 0 and h:
                    h[min(pos, len(h) - 1)] = alpha[int(rng.integers(0, 30))]
                elif k == 1:
                    h.insert(pos, alpha[int(rng.integers(0, 30))])
                elif h:
                    del h[min(pos, len(h) - 1)]
            hyps.append(h)
        out.append(hyps)
    return out


def main():
    install_stubs()
    sys.path.insert(0, REF)
    al = load("ref_align", "espnet_data/preprocess/align.py")
    sys.modules.setdefault("espnet_data", types.ModuleType("espnet_data"))
    sys.modules.setdefault("espnet_data.preprocess", types.ModuleType("espnet_data.preprocess"))
    sys.modules["espnet_data.preprocess.align"] = al
    pre = load("ref_nbest_align_pre", "Nbest_Align/preprocess.py")
    rng = np.random.default_rng(20)
    lists = [
        [["how", "are", "you"], ["how", "are", "you", "doing"]],          # align.py's docstring answers
        [list("你好嗎"), list("你好不好")],
        [list("1234"), list("123"), list("12345"), list("13")],           # preprocess.py's __main__
    ] + random_lists(rng)
    cases = []
    for hyps in lists:
        t = reference_table(pre, al, hyps)
        cases.append({"h": [pack(h) for h in hyps], "t": None if t is None else [pack(s) for s in t]})
    # feature rows of get_feature itself (tiny lists: its search enumerates every combination)
    f_hyps = {"u0": {"h1": "abca", "h2": "abda", "h3": "aca"}, "u1": {"h1": "ab", "h2": "cab", "h3": "abd", "h4": "b"},
              "u2": {"h1": "dcba", "h2": "dcba"}, "u3": {"h1": "abc", "h2": "abcd", "h3": "bc"}}
    f_refs = {"u0": "abda", "u1": "cabd", "u2": "dcb", "u3": "abcd"}
    with tempfile.TemporaryDirectory() as td:
        paths = [os.path.join(td, "ref_text.json"), os.path.join(td, "hyp_text.json")]
        json.dump(f_refs, open(paths[0], "w"))
        json.dump(f_hyps, open(paths[1], "w"))
        cfg = types.SimpleNamespace(model=types.SimpleNamespace(bert="char"), max_utt=100, n_best=10)
        rows = pre.get_feature(cfg, paths, ["ref_text", "hyp_text"])
    json.dump({"cases": cases, "features": {"charset": FEATURE_CHARS, "hyps": f_hyps, "refs": f_refs, "rows": rows}},
              open(OUT, "w", encoding="utf-8"), ensure_ascii=False, separators=(",", ":"))
    print(len(cases), "cases,", sum(c["t"] is None for c in cases), "IndexError;", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
