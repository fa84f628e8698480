"""CPU: the numpy oracle of hrec_als_explain (tests/explain_oracle.py). Its two
precisions agree, its contributions add up to the prediction y_i . (A^-1 b),
and EVERY generated call of the GPU test satisfies the gap condition under
which positions are compared exactly (so no GPU case is ever left out)."""
import numpy as np
import pytest

import explain_oracle as eo


def _problem(seed, k, n, implicit, alpha, special=False):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((60, k)).astype(np.float32)
    cols = rng.integers(0, 60, n).astype(np.int32)  # duplicates stay separate terms
    vals = rng.uniform(-5, 5, n).astype(np.float32)
    if special:
        vals[::4] = 0.0  # zero and negative ratings
        vals[1::4] = -np.abs(vals[1::4])
        vals[2] = abs(vals[2]) + 0.5
    entries = rng.integers(0, 60, 7)
    return Y, cols, vals, entries


CASES = [(1, 8, 20, 0, 0.0, False), (2, 8, 20, 1, 0.5, False), (3, 20, 5, 0, 0.0, True), (4, 20, 5, 1, 2.0, True),
         (5, 33, 100, 1, 0.0, True), (6, 64, 150, 0, 0.0, True), (7, 10, 1, 0, 0.0, False), (8, 10, 3, 1, 40.0, True)]


@pytest.mark.parametrize("seed,k,n,implicit,alpha,special", CASES)
def test_paths_agree_and_sum_to_the_prediction(seed, k, n, implicit, alpha, special):
    Y, cols, vals, entries = _problem(seed, k, n, implicit, alpha, special)
    r64 = eo.explain_row(Y, k, cols, vals, entries, 0.1, implicit, alpha, dt=eo.F64)
    rld = eo.explain_row(Y, k, cols, vals, entries, 0.1, implicit, alpha, dt=eo.LD)
    assert r64.ok and rld.ok and r64.c.dtype == np.float64 and rld.c.dtype == np.longdouble
    scale = np.abs(rld.c).sum(axis=1, keepdims=True)
    assert (np.abs(r64.c - rld.c) <= 1e-11 * scale).all()
    assert np.array_equal(r64.elig, rld.elig)
    # sum_j c_ij = y_i . (A^-1 b), longdouble
    pred = Y[entries, :k].astype(eo.LD) @ rld.x
    assert (np.abs(rld.total() - pred) <= 1e-15 * scale[:, 0]).all()
    if implicit:
        assert np.array_equal(rld.elig, vals > 0)
        assert (rld.c[:, ~rld.elig] == 0).all()  # beta = 0: no share
    p64, v64, l64 = eo.top_lists(r64, 5)
    pld, vld, lld = eo.top_lists(rld, 5)
    assert np.array_equal(l64, lld) and (l64 == min(5, int(rld.elig.sum()))).all()


def test_blank_rows_and_invalid_entries():
    Y, cols, vals, entries = _problem(11, 8, 10, 1, 1.0)
    for dt in (eo.F64, eo.LD):
        assert not eo.explain_row(Y, 8, cols[:0], vals[:0], entries, 0.1, 0, 0.0, dt=dt).ok
        assert not eo.explain_row(Y, 8, cols, -np.abs(vals), entries, 0.1, 1, 1.0, dt=dt).ok  # no rating > 0
        # a zero matrix (no regularisation, alpha 0, YtY 0) has no usable factorisation
        assert not eo.explain_row(Y, 8, cols, np.abs(vals), entries, 0.0, 1, 0.0, yty=np.zeros((8, 8)), dt=dt).ok
        e = np.array([3, -1, 60, 5])
        row = eo.explain_row(Y, 8, cols, np.abs(vals), e, 0.1, 1, 1.0, dt=dt)
        assert np.isnan(row.c[1]).all() and np.isnan(row.c[2]).all() and np.isfinite(row.c[[0, 3]]).all()
        pos, val, ln = eo.top_lists(row, 4)
        assert list(ln) == [4, 0, 0, 4] and (pos[1] == -1).all() and np.isnan(val[2]).all()


def test_ties_put_the_earlier_position_first():
    Y, _, _, entries = _problem(12, 8, 10, 0, 0.0)
    cols = np.array([5, 9, 5, 30, 9], np.int32)
    vals = np.array([2.0, 3.0, 2.0, 1.0, 3.0], np.float32)
    row = eo.explain_row(Y, 8, cols, vals, entries, 0.1, 0, 0.0, dt=eo.LD)
    assert (row.c[:, 0] == row.c[:, 2]).all() and (row.c[:, 1] == row.c[:, 4]).all()
    pos, val, ln = eo.top_lists(row, 5)
    for i in range(len(entries)):
        p = list(pos[i])
        assert p.index(0) < p.index(2) and p.index(1) < p.index(4)
    assert not eo.gaps_ok(row, 5)


def test_every_generated_call_meets_the_gap_condition():
    """The share of GPU cases left out of the exact position check is zero."""
    assert len(eo.CALLS) >= 30
    names = [c.name for c in eo.CALLS]
    assert len(set(names)) == len(names)
    for call in eo.CALLS:
        seen = {}
        for r in range(len(call.hist_rows)):
            key = (int(call.hist_rows[r]), call.row_entries(r).tobytes())
            if key in seen:
                continue
            seen[key] = True
            row = call.oracle_row(r, eo.LD)
            assert eo.gaps_ok(row, call.top_m), (call.name, r)
