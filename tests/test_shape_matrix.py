"""CPU: the shape matrix of tests/shape_matrix.py: its inputs are what the GPU tests' docstrings
say they are, and its two oracles (TorchBert in fp32 and on float64 weights) agree within the measured
e32 figures on the two smallest shapes."""
import numpy as np
import pytest

import shape_matrix as SM


def test_inputs_are_as_documented():
    for vocab in (1000, 1100):
        sid = "h512" if vocab == 1100 else "l1"
        nb = SM.inputs(sid)
        T = np.diff(nb.hyp_off)
        assert nb.n_hyp == 24 and int((T - 2).sum()) == 1042 and SM.token_rows(nb) == 49762
        assert T.min() == 31 and T.max() == 63
        assert (T <= 48).any() and (T > 48).any()
        assert int(nb.tokens.max()) < vocab
        edges = SM.edge_inputs(sid)
        assert np.diff(edges.hyp_off).tolist() == [3, 65, 72] and 72 <= SM.MAX_POS and int(edges.tokens.max()) < vocab
    for sid in SM.TRAINER_IDS:
        s = SM.SHAPES[sid]
        nb = SM.train_inputs(sid)[0]
        assert nb.n_hyp == 18 and int(np.diff(nb.hyp_off).max()) <= SM.MAX_POS
        assert s.intermediate % 4 == 0 and s.vocab % 4 == 0
    for sid in SM.SCORER_IDS:
        s = SM.SHAPES[sid]
        assert s.hidden == 64 * s.heads and s.intermediate % 128 == 0


def test_sets_plan_has_two_and_three_positions():
    nb = SM.inputs("l1")
    row_off, pos_off, pos = SM.sets_plan(nb)
    n = np.diff(pos_off)
    assert set(n.tolist()) == {2, 3} and len(row_off) == nb.n_hyp + 1
    ids, am, lab, qpos = SM.sets_rows(nb, (row_off, pos_off, pos), 103)
    assert ((ids == 103).sum(1) == n).all() and ((lab != -100).sum(1) == n).all()
    assert all(p == sorted(set(p)) for p in qpos)


@pytest.mark.parametrize("sid", ["f640", "l1"])
def test_oracles_agree(sid):
    o = SM.oracle(sid)
    e_pll = SM.rel_err(o.pll32, o.pll64).max()
    print(f"SHAPES {sid} oracle: e32 rows {o.e32_rows:.3e} pll {o.e32_pll:.3e} (rel {e_pll:.3e}) "
          f"min |row| {np.abs(o.rows64).min():.3f} cls e32 {np.abs(o.cls32 - o.cls64).max():.3e}")
    assert o.rows64.shape == (1042,) and o.lp64.shape == (1042, SM.SHAPES[sid].vocab)
    assert o.e32_rows <= 5.7e-6 and e_pll <= 7.9e-8
    assert np.abs(o.rows64).min() >= 3.09
    assert np.abs(o.cls32 - o.cls64).max() <= 1e-5
