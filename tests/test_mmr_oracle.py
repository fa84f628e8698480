"""CPU: the numpy oracle of hrec_mmr_rerank (tests/mmr_oracle.py) against an
np.longdouble evaluation of the same definition, the gap of the seeded inputs
the GPU tests compare exactly, and the consequences of the definition on
hand-made pools."""
import numpy as np
import pytest

import mmr_oracle as mo


def _id(case):
    return "d%d-p%d-t%d-r%d-l%s-%s" % (case.d, case.pool, case.top_n, case.rows, case.lam, "f64" if case.f64 else "f32")


@pytest.mark.parametrize("case", mo.EXACT_CASES, ids=_id)
def test_gap_of_the_exact_cases(case):
    """The seeded inputs compared exactly on the GPU have a smallest gap between
    the best and the second-best value above 1e3 * tol at every step."""
    res = mo.case_oracle(case)
    print(_id(case), "min gap", res.gap.min(), "1e3 tol", 1e3 * mo.tol(case.d))
    assert res.gap.min() > 1e3 * mo.tol(case.d)


@pytest.mark.parametrize("case", mo.EXACT_CASES, ids=_id)
def test_oracle_against_longdouble_exact_cases(case):
    pool, s, vectors = mo.case_inputs(case)
    res = mo.case_oracle(case)
    inv = mo.inv_norms(vectors)
    sl = slice(0, min(case.rows, 5))  # the first rows are enough for the oracle's own check
    ext = mo.mmr(pool[sl], s[sl], vectors, inv, case.lam, case.top_n, dtype=np.longdouble)
    assert np.array_equal(ext.pos, res.pos[sl]) and np.array_equal(ext.len, res.len[sl])
    err = np.abs(ext.value.astype(np.float64) - res.value[sl]).max()
    print(_id(case), "max |f64 - longdouble|", err, "tol", mo.tol(case.d))
    assert err <= mo.tol(case.d)


@pytest.mark.parametrize("case", [c for c in mo.CASES if c not in mo.EXACT_CASES], ids=_id)
def test_oracle_against_longdouble_replayed(case):
    """Where ties are possible (d = 1, lambda 0 or 1) the f64 picks are
    replayed in extended precision: each is within tol of the best there."""
    pool, s, vectors = mo.case_inputs(case)
    res = mo.case_oracle(case)
    sl = slice(0, min(case.rows, 5))
    ext = mo.mmr(pool[sl], s[sl], vectors, mo.inv_norms(vectors), case.lam, case.top_n, forced=res.pos[sl],
                 dtype=np.longdouble)
    assert ext.deficit.max() <= mo.tol(case.d)
    live = res.pos[sl] >= 0
    assert np.abs(ext.value.astype(np.float64) - res.value[sl])[live].max() <= mo.tol(case.d)


def _unit(*rows):
    return np.asarray(rows, np.float32)


def test_hand_made_pool():
    """Items 0 and 1 point the same way, item 2 is orthogonal. Scores 3, 2, 1:
    rel 1, 0.5, 0. lambda 0.5: step 0 values 0.5, 0.25, 0 -> 0; step 1:
    0.25 - 0.5 * 1 = -0.25 against 0 - 0 = 0 -> 2; then 1."""
    v = _unit([2, 0], [3, 0], [0, 1])
    pool = np.array([[0, 1, 2]])
    s = np.array([[3.0, 2.0, 1.0]])
    res = mo.mmr(pool, s, v, mo.inv_norms(v), 0.5, 3)
    assert res.pos.tolist() == [[0, 2, 1]] and res.len.tolist() == [3]
    assert res.value.tolist() == [[0.5, 0.0, -0.25]]
    assert res.gap[0] == 0.25


def test_lambda_one_keeps_pool_order_and_first_pick_is_the_best():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((30, 4)).astype(np.float32)
    pool = np.stack([rng.permutation(30)[:12] for _ in range(4)])
    s = -np.sort(-rng.standard_normal((4, 12)), axis=1)
    s[1, 3] = s[1, 4]  # equal scores keep their order
    res = mo.mmr(pool, s, v, mo.inv_norms(v), 1.0, 12)
    assert np.array_equal(res.pos, np.tile(np.arange(12), (4, 1)))
    s2 = s.copy()
    s2[0, 0], s2[0, 1] = np.nan, np.inf  # the best finite-scored entry is position 2
    for lam in (0.0, 0.3, 1.0):
        assert mo.mmr(pool, s2, v, mo.inv_norms(v), lam, 3).pos[0, 0] == 2


def test_invalid_entries_and_lengths():
    v = _unit([1, 0], [0, 1], [1, 1], [0, 0])
    inv = mo.inv_norms(v)
    assert inv[3] == 0.0
    pool = np.array([[0, -1, 7, 1, 2, 3], [-1, 9, 4, -5, 4, 4], [2, 3, 0, 1, 0, 0]])
    s = np.array([[6.0, 5.0, 4.0, 3.0, 2.0, 1.0]] * 3)
    res = mo.mmr(pool, s, v, inv, 0.5, 4, pool_len=[6, 6, 2])
    assert res.len.tolist() == [4, 0, 2]
    assert set(res.pos[0].tolist()) == {0, 3, 4, 5} and res.pos[0, 0] == 0
    assert res.pos[1].tolist() == [-1] * 4 and np.isnan(res.value[1]).all()
    # the zero vector (position 1 of row 2) has cosine 0 with everything
    assert res.pos[2].tolist() == [0, 1, -1, -1] and res.value[2, 1] == 0.0
    # non-finite scores: never the first pick while a finite one exists, selected last, value -inf
    s3 = np.array([[np.nan, 5.0, -np.inf, 3.0, np.inf, 1.0]])
    pool3 = np.array([[0, 1, 2, 0, 1, 2]])
    r3 = mo.mmr(pool3, s3, v, inv, 0.5, 6)
    assert sorted(r3.pos[0, :3].tolist()) == [1, 3, 5] and r3.pos[0, 3:].tolist() == [0, 2, 4]
    assert np.isneginf(r3.value[0, 3:]).all()


def test_forced_replay_reports_the_deficit():
    v = _unit([2, 0], [3, 0], [0, 1])
    pool, s = np.array([[0, 1, 2]]), np.array([[3.0, 2.0, 1.0]])
    res = mo.mmr(pool, s, v, mo.inv_norms(v), 0.5, 3, forced=np.array([[0, 1, 2]]))
    assert res.deficit.tolist() == [[0.0, 0.25, 0.0]]
    with pytest.raises(AssertionError):
        mo.mmr(pool, s, v, mo.inv_norms(v), 0.5, 3, forced=np.array([[0, 0, 2]]))
