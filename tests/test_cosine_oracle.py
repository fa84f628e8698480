"""CPU: the numpy oracle of hrec_cosine_topk (tests/cosine_oracle.py) against
sklearn's cosine_similarity, on the tie rule and on the zero-row rule."""
import numpy as np
import pytest

import cosine_oracle as co


@pytest.mark.parametrize("d", [1, 3, 50, 64, 200, 256])
def test_sims_match_sklearn(d):
    """Generic rows: both are f64 cosines of the same f32 values, each within
    (d + 4) 2^-53 of the real one for unit-size terms, so 1e-12 is a bound on
    f64 rounding at d <= 256, not a tuned number."""
    from sklearn.metrics.pairwise import cosine_similarity

    rng = np.random.default_rng(100 + d)
    v = rng.standard_normal((300, d)).astype(np.float32)
    q = np.arange(0, 300, 7)
    got = co.sims(v, d, co.inv_norms(v), q)
    want = cosine_similarity(v[q].astype(np.float64), v.astype(np.float64))
    assert np.abs(got - want).max() <= 1e-12


def test_chain_is_sequential():
    """np.add.accumulate is the left-to-right chain: a Python loop over the
    components gives the same bits."""
    rng = np.random.default_rng(7)
    v = rng.standard_normal((40, 65)).astype(np.float32)
    inv = co.inv_norms(v)
    got = co.sims(v, 65, inv, [3, 17])
    for b, r in enumerate((3, 17)):
        for j in range(40):
            acc = 0.0
            for c in range(65):
                acc = acc + float(v[r, c]) * float(v[j, c])
            assert got[b, j] == (acc * inv[r]) * inv[j]


def test_padding_columns_are_ignored():
    rng = np.random.default_rng(8)
    v = rng.standard_normal((30, 12)).astype(np.float32)
    w = v.copy()
    w[:, 9:] = np.nan
    a = co.topk(v[:, :9].copy(), 9, co.inv_norms(v, 9), np.arange(30), 5)
    b = co.topk(w, 9, co.inv_norms(w, 9), np.arange(30), 5)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_tie_rule_smaller_column_first_and_self_skipped():
    base = np.random.default_rng(9).standard_normal((5, 8)).astype(np.float32)
    v = np.concatenate([base, base, base])  # every row three times
    inv = co.inv_norms(v)
    idx, val, ln = co.topk(v, 8, inv, np.arange(15), 4)
    assert (ln == 4).all()
    for r in range(15):
        twins = [j for j in (r % 5, r % 5 + 5, r % 5 + 10) if j != r]
        assert idx[r, :2].tolist() == twins  # ascending columns among equal sims
        assert val[r, 0] == val[r, 1]
        assert r not in idx[r]
    idx0, val0, _ = co.topk(v, 8, inv, np.arange(15), 3, skip_self=False)
    assert (idx0 == np.stack([np.arange(15) % 5, np.arange(15) % 5 + 5, np.arange(15) % 5 + 10], 1)).all()


def test_zero_rows_and_non_finite_rows_have_similarity_zero():
    rng = np.random.default_rng(10)
    v = rng.standard_normal((12, 6)).astype(np.float32)
    v[2] = 0.0
    v[5, 1] = np.nan
    v[7, 0] = np.inf
    inv = co.inv_norms(v)
    assert inv[2] == 0 and inv[5] == 0 and inv[7] == 0
    s = co.sims(v, 6, inv, np.arange(12))
    assert np.isfinite(s).all()
    for z in (2, 5, 7):
        assert (s[z] == 0).all() and (s[:, z] == 0).all()
        assert not np.signbit(s[z]).any()
    idx, val, ln = co.topk(v, 6, inv, [2], 11)
    assert ln[0] == 11 and (val[0] == 0).all() and idx[0].tolist() == [j for j in range(12) if j != 2]
    # a strict cut at 0 removes them all
    assert co.topk(v, 6, inv, [2], 11, min_sim=0.0)[2][0] == 0


def test_lengths_unknown_queries_and_min_sim():
    rng = np.random.default_rng(11)
    v = rng.standard_normal((9, 4)).astype(np.float32)
    inv = co.inv_norms(v)
    idx, val, ln = co.topk(v, 4, inv, [0, -1, 9, 8, 0], 20)
    assert ln.tolist() == [8, 0, 0, 8, 8]
    assert (idx[1] == -1).all() and np.isnan(val[1]).all()
    assert (idx[0, 8:] == -1).all() and np.isnan(val[0, 8:]).all()
    assert np.array_equal(idx[0], idx[4])
    assert (np.diff(val[0, :8]) <= 0).all()
    cut = val[0, 2]
    idx2, val2, ln2 = co.topk(v, 4, inv, [0], 20, min_sim=cut)
    assert ln2[0] == int((val[0, :8] > cut).sum()) and ln2[0] <= 2
    assert co.topk(v, 4, inv, [0], 20, skip_self=False)[2][0] == 9
    one = co.topk(v[:1], 4, inv[:1], [0], 3)
    assert one[2][0] == 0
