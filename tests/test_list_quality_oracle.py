"""CPU: the list-quality oracle (tests/list_quality_oracle.py) against closed
forms, and the sum identity the device kernel uses against the pairwise
definition, both in extended precision."""
import numpy as np
import pytest

import list_quality_oracle as lq


def test_gini_closed_forms():
    assert lq.gini(np.full(7, 3)) == 0.0
    for n in (2, 5, 100):
        c = np.zeros(n, np.int64)
        c[n // 2] = 11
        assert lq.gini(c) == (n - 1) / n


def test_entropy_of_uniform_exposure():
    for m in (1, 2, 8, 37):
        c = np.zeros(50, np.int64)
        c[:m] = 4
        assert abs(lq.distributional_coverage(c) - np.log2(m)) <= 4 * m * lq.U53 * max(1.0, np.log2(m))
    assert lq.catalog_coverage(np.array([0, 2, 0, 1])) == 0.5


def test_personalization_closed_forms():
    same = np.tile(np.arange(5), (4, 1))
    assert lq.personalization(same, None, 30, 5) == 0.0
    disjoint = np.arange(20).reshape(4, 5)
    assert lq.personalization(disjoint, None, 30, 5) == 1.0
    assert np.isnan(lq.personalization(same[:1], None, 30, 5))
    # rows without an entry do not count as users
    assert lq.personalization(np.vstack([same, np.full((1, 5), -1)]), None, 30, 5) == 0.0


def test_diversity_closed_forms():
    v = np.tile(np.array([[3.0, 4.0, 0.0]], np.float32), (6, 1))
    vals, cnt, exposure = lq.per_row(np.arange(6)[None, :], None, v)
    assert abs(vals[0, 0]) <= 8 * (3 + 6) * lq.U53
    eye = np.eye(6, dtype=np.float32) * 2.5
    vals, cnt, exposure = lq.per_row(np.arange(6)[None, :], None, eye)
    assert vals[0, 0] == 1.0
    assert cnt[0, 0] == 6 and exposure.tolist() == [1] * 6
    # fewer than two valid entries: undefined
    assert np.isnan(lq.per_row(np.array([[2, -1, 9]]), None, eye)[0][0, 0])


def test_invalid_entries_and_zero_vectors_are_ignored():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((9, 5)).astype(np.float32)
    v[4] = 0
    v[5, 2] = np.inf
    x = lq.unit_rows(v)
    assert not x[4].any() and not x[5].any()
    lists = np.array([[0, -1, 4, 9, 5, 2, 7]])
    vals, cnt, exposure = lq.per_row(lists, [6], v, history=[np.array([-1, 1, 30, 3])],
                                     tables=np.array([[1.0, 2, 3, 4, np.nan, 6, 7, 8, 9]]))
    assert cnt[0].tolist() == [4, 2, 3]  # 0, 4, 5, 2 | 1, 3 | 0, 5, 2
    assert exposure.tolist() == [1, 0, 1, 0, 1, 1, 0, 0, 0]
    assert vals[0, 2] == (1.0 + 6.0 + 3.0) / 3
    pairs = x[0] @ x[2]  # every pair with item 4 or 5 is 0
    assert abs(vals[0, 0] - (1 - pairs / 6)) <= 8 * (5 + 4) * lq.U53


@pytest.mark.parametrize("d,m,g", [(1, 2, 1), (50, 10, 30), (64, 70, 5), (200, 40, 600), (256, 300, 0)])
def test_sum_identity_agrees_with_pairs_in_extended_precision(d, m, g):
    """The f64 oracle (pairwise) against both formulations in np.longdouble: a
    quarter of the device tolerance 8 (d + m + g) 2^-53."""
    rng = np.random.default_rng(d * 1000 + m)
    n = m + g + 3
    v = (rng.standard_normal((n, d)) + 0.3).astype(np.float32)  # a common offset: cosines well away from 0
    cols = rng.permutation(n)[:m]
    hist = rng.permutation(n)[:g]
    x64, xl = lq.unit_rows(v), lq.unit_rows(v, dtype=np.longdouble)
    tol = 0.25 * 8 * (d + m + g) * lq.U53
    ref = lq.diversity_pairwise(x64, cols)
    assert abs(float(lq.diversity_pairwise(xl, cols)) - ref) <= tol
    assert abs(float(lq.diversity_identity(xl, cols)) - ref) <= tol
    assert abs(float(lq.diversity_identity(x64, cols)) - ref) <= 4 * tol  # the kernel's route in f64: the full bound
    if g:
        ref = lq.unexpectedness_pairwise(x64, cols, hist)
        assert abs(float(lq.unexpectedness_pairwise(xl, cols, hist)) - ref) <= tol
        s, h = xl[cols].sum(axis=0), xl[hist].sum(axis=0)
        assert abs(float(1 - np.dot(s, h) / (m * g)) - ref) <= tol


def test_history_tables():
    nov, pop = lq.history_tables([1, 1, 2, 2, 2, 1], [0, 0, 0, 3, 3, 2], 5)
    # distinct pairs: (1,0) (1,2) (2,0) (2,3): h = 2, 0, 1, 1, 0
    assert pop.tolist() == [1.0, 0.0, 0.5, 0.5, 0.0]
    assert nov[0] == 1.0 and nov[2] == 2.0 and np.isnan(nov[1]) and np.isnan(nov[4])
