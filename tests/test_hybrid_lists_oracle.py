"""CPU: tests/hybrid_lists_oracle.py against oracle.fusion (adaptive_fusion +
top_k, the restated reference) on tie-free rows, and against hand-written
cases: ties, NaN rows, everything excluded, out-of-range and duplicate
columns, the substitution, and the list-overflow predicate."""
import numpy as np
from hybrid_lists_oracle import DBL_MAX, excluded_set, fuse_row, lists, ranking, row_overflows, substitute

from oracle import fusion as ofus


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def test_matches_reference_fusion_on_tie_free_rows():
    rng = np.random.default_rng(3)
    for n, als_wins in ((1, True), (7, False), (300, True), (301, False)):
        als = rng.normal(size=(4, n)).astype(np.float32)
        tt = rng.normal(size=(4, n)).astype(np.float32)
        got, lens, _ = lists(als, tt, n, als_wins)
        f1 = (0.5, 0.1) if als_wins else (0.1, 0.5)
        for r in range(4):
            ref = ofus.top_k(ofus.adaptive_fusion(list(zip(range(n), [float(x) for x in als[r]])),
                                                  list(zip(range(n), tt[r])), *f1, legacy=True), n)
            assert len(set(s for _, s in ref)) == n  # tie-free
            idx, val = got[r]
            assert idx.tolist() == [i for i, _ in ref]
            np.testing.assert_array_equal(_bits(val), _bits([s for _, s in ref]))
            assert lens[r] == n


def test_substitution_is_f64_and_per_entry():
    fb = np.array([0.1, 1 / 3, 2 / 3, 0.7])  # not f32-representable
    a = substitute(np.array([1.5, np.nan, np.nan, -2.0], np.float32), fb)
    np.testing.assert_array_equal(_bits(a), _bits([1.5, 1 / 3, 2 / 3, -2.0]))
    a = substitute(np.array([np.nan, 2.0], np.float32))
    assert np.isnan(a[0]) and a[1] == 2.0
    # the reference fusion over the substituted f64 row
    tt = np.array([0.3, 0.1, 0.9, 0.5], np.float32)
    als = np.array([1.5, np.nan, np.nan, -2.0], np.float32)
    got, _, mm = lists(als[None], tt[None], 4, True, fallback=fb)
    ref = ofus.top_k(ofus.adaptive_fusion(list(zip(range(4), substitute(als, fb).tolist())), list(zip(range(4), tt)),
                                          1.0, 0.0), 4)
    assert got[0][0].tolist() == [i for i, _ in ref]
    np.testing.assert_array_equal(_bits(got[0][1]), _bits([s for _, s in ref]))
    np.testing.assert_array_equal(mm[0], [-2.0, 1.5, np.float64(np.float32(0.1)), np.float64(np.float32(0.9))])


def test_ties_keep_column_order_and_nan_ranks_last():
    assert ranking(np.array([1.0, 2.0, 1.0, 2.0, 0.0, -0.0])).tolist() == [1, 3, 0, 2, 4, 5]
    assert ranking(np.array([np.nan, 1.0, np.nan, -np.inf])).tolist() == [1, 3, 0, 2]
    als = np.array([[0.0, 1.0, 0.0, 1.0, np.nan]], np.float32)
    tt = np.array([[1.0, 0.0, 1.0, 0.0, 0.5]], np.float32)
    got, lens, _ = lists(als, tt, 5, True)
    assert got[0][0].tolist() == [1, 3, 0, 2, 4]  # 0.8, 0.8, 0.2, 0.2, NaN
    np.testing.assert_array_equal(got[0][1][:4], [0.8, 0.8, 0.2, 0.2])
    assert np.isnan(got[0][1][4]) and lens[0] == 5


def test_all_nan_and_constant_rows():
    fused, mm = fuse_row(np.full(3, np.nan), np.array([1, 2, 3], np.float32), False)
    assert np.isnan(fused).all()
    np.testing.assert_array_equal(mm, [DBL_MAX, -DBL_MAX, 1.0, 3.0])
    fused, mm = fuse_row(np.array([1.0, 2.0]), np.full(2, np.nan, np.float32), True)
    assert np.isnan(fused).all()
    np.testing.assert_array_equal(mm, [1.0, 2.0, DBL_MAX, -DBL_MAX])
    # constant rows: range 0 -> scale 1, x * 1 + (0 - x) = 0
    fused, _ = fuse_row(np.full(4, 2.5), np.full(4, -1.25, np.float32), True)
    np.testing.assert_array_equal(fused, np.zeros(4))
    got, _, _ = lists(np.full((1, 4), 2.5, np.float32), np.full((1, 4), -1.25, np.float32), 3, True)
    assert got[0][0].tolist() == [0, 1, 2]


def test_exclusion_and_lengths():
    als = np.array([[4, 3, 2, 1, 0]] * 4, np.float32)
    tt = np.array([[4, 3, 2, 1, 0]] * 4, np.float32)
    rows = np.array([0, 1, -1, 2])
    indptr = np.array([0, 7, 12, 12])
    cols = np.array([-3, 0, 0, 2, 2, 5, 9, 0, 1, 2, 3, 4], np.int32)  # out of range, duplicates; everything; empty
    excl = (rows, indptr, cols)
    assert excluded_set(excl, 0, 5).tolist() == [0, 2]
    assert excluded_set(excl, 1, 5).tolist() == [0, 1, 2, 3, 4]
    assert excluded_set(excl, 2, 5).size == 0 and excluded_set(excl, 3, 5).size == 0
    got, lens, mm = lists(als, tt, 4, True, excl=excl)
    assert got[0][0].tolist() == [1, 3, 4] and got[1][0].tolist() == []
    assert got[2][0].tolist() == [0, 1, 2, 3] and got[3][0].tolist() == [0, 1, 2, 3]
    assert lens.tolist() == [3, 0, 4, 4]
    # the scalers see the excluded columns: column 1 keeps the score it has in the full row
    full, _, _ = lists(als, tt, 5, True)
    assert got[0][1][0] == full[0][1][1] == 0.8 * 0.75 + 0.2 * 0.75
    np.testing.assert_array_equal(mm, np.array([[0.0, 4.0, 0.0, 4.0]] * 4))
    # an excluded column never displaces a NaN entry
    als[0, 1] = np.nan
    got, lens, _ = lists(als, tt, 5, True, excl=excl)
    assert got[0][0].tolist() == [3, 4, 1] and lens[0] == 3 and np.isnan(got[0][1][2])


def test_row_overflow_predicate():
    fused = np.zeros(50)
    assert not row_overflows(fused, [], 3, sample=50, cap=10)           # the row is the sample
    assert row_overflows(fused, [], 3, sample=20, cap=10)               # 50 equal values reach the bound
    assert not row_overflows(fused, np.arange(40), 3, sample=20, cap=10)  # no live sample column: all 10 pass
    assert row_overflows(fused, np.arange(39), 3, sample=20, cap=10)
    v = np.arange(50, dtype=np.float64)
    assert not row_overflows(v, [], 3, sample=20, cap=40)  # bound 17: 33 values reach it
    assert row_overflows(v, [], 3, sample=20, cap=32)
    v[:20] = np.nan
    assert row_overflows(v, [], 3, sample=20, cap=49)      # a NaN bound admits everything
