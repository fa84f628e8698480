"""GPU: hrec_mmr_rerank against the numpy oracle (tests/mmr_oracle.py).

(a) Validity on every case of mmr_oracle.CASES: the kernel's own selections
are replayed in the oracle; at every step the selected entry's oracle value is
within tol of the oracle's maximum over the unselected entries, and out_value
is within tol of it. tol = 8 (d + 4) 2^-53 absolute (mmr_oracle.tol has the
derivation). (b) Exact equality of out_pos on the gap-checked seeded inputs
(mmr_oracle.EXACT_CASES; tests/test_mmr_oracle.py checks their gaps). (c)
lambda = 1, (d) lambda = 0 on clusters, (e) duplicates, (f) invalid entries,
(g) equal bits on a second call. Both sides take the SAME inv_norm: the
kernel's hrec_row_inv_norms, read back.

One kernel run and one oracle replay per case, shared by (a), (b) and (g)."""
import numpy as np
import pytest

import mmr_oracle as mo

pytestmark = pytest.mark.gpu


def _id(case):
    return "d%d-p%d-t%d-r%d-l%s-%s" % (case.d, case.pool, case.top_n, case.rows, case.lam, "f64" if case.f64 else "f32")


def run(pool, scores, vectors, lam, top_n, pool_len=None, inv=None):
    """(pos, len, value, inv_norm) numpy of one kernel call on host arrays."""
    import torch
    from src import _hrec

    v = torch.as_tensor(np.ascontiguousarray(vectors), device="cuda")
    inv_d = _hrec.row_inv_norms(v) if inv is None else torch.as_tensor(inv, device="cuda")
    pl = None if pool_len is None else torch.as_tensor(np.asarray(pool_len, np.int32), device="cuda")
    pos, ln, val = _hrec.mmr_rerank(torch.as_tensor(np.ascontiguousarray(pool), device="cuda"),
                                    torch.as_tensor(np.ascontiguousarray(scores), device="cuda"), v, inv_d, lam, top_n,
                                    pool_len=pl, want_value=True)
    torch.cuda.synchronize()
    return pos.cpu().numpy(), ln.cpu().numpy(), val.cpu().numpy(), inv_d.cpu().numpy()


def check_valid(got, pool, scores, vectors, lam, top_n, d, pool_len=None):
    """(a) for one call; returns the oracle's own Result on the same inputs."""
    pos, ln, val, inv = got
    want = mo.mmr(pool, scores, vectors, inv, lam, top_n, pool_len=pool_len)
    assert np.array_equal(ln, want.len)
    live = np.arange(top_n)[None, :] < ln[:, None]
    assert (pos[~live] == -1).all() and np.isnan(val[~live]).all()
    rep = mo.mmr(pool, scores, vectors, inv, lam, top_n, pool_len=pool_len, forced=pos)  # asserts each pick is open
    tol = mo.tol(d)
    with np.errstate(invalid="ignore"):
        verr = np.where(rep.value == val, 0.0, np.abs(rep.value - val))[live]
    print("max deficit", rep.deficit.max(), "max |out_value - oracle|", verr.max() if verr.size else 0.0, "tol", tol)
    assert rep.deficit.max() <= tol
    assert not verr.size or verr.max() <= tol
    return want


_RUNS = {}


def case_run(case):
    if case not in _RUNS:
        pool, s, vectors = mo.case_inputs(case)
        _RUNS[case] = run(pool, s, vectors, case.lam, case.top_n)
    return _RUNS[case]


_WANT = {}


@pytest.mark.parametrize("case", mo.CASES, ids=_id)
def test_valid(device, case):
    pool, s, vectors = mo.case_inputs(case)
    _WANT[case] = check_valid(case_run(case), pool, s, vectors, case.lam, case.top_n, case.d)


@pytest.mark.parametrize("case", mo.EXACT_CASES, ids=_id)
def test_exact(device, case):
    pool, s, vectors = mo.case_inputs(case)
    pos, ln, val, inv = case_run(case)
    want = _WANT.get(case) or mo.mmr(pool, s, vectors, inv, case.lam, case.top_n)
    assert want.gap.min() > 1e3 * mo.tol(case.d)  # with the kernel's inv_norm too
    assert np.array_equal(pos, want.pos) and np.array_equal(ln, want.len)
    assert (pos[:, 0] == 0).all()  # the first pick is the best-scored entry


@pytest.mark.parametrize("case", [c for c in mo.CASES if c.rows > 1 or c.pool >= 600], ids=_id)
def test_same_bits_on_a_second_call(device, case):
    pool, s, vectors = mo.case_inputs(case)
    a = case_run(case)
    b = run(pool, s, vectors, case.lam, case.top_n)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("d,pool,rows,f64", [(8, 63, 5, False), (65, 100, 5, True), (50, 257, 3, False),
                                             (8, 1024, 2, True), (64, 1024, 2, False)])
def test_lambda_one_returns_pool_order(device, d, pool, rows, f64):
    """(c): 0 .. len - 1 exactly, equal scores, short rows and skipped entries included."""
    rng = np.random.default_rng(d + pool)
    n = 2 * pool
    vectors = rng.standard_normal((n, d)).astype(np.float32)
    cols = np.stack([rng.permutation(n)[:pool] for _ in range(rows)]).astype(np.int64)
    s = -np.sort(-rng.standard_normal((rows, pool)), axis=1)
    s[0, : pool // 2] = s[0, 0]  # equal scores
    s[-1, :] = 1.5               # all equal: hi == lo
    s = s if f64 else s.astype(np.float32)
    pos, ln, val, _ = run(cols, s, vectors, 1.0, pool)
    assert (ln == pool).all() and np.array_equal(pos, np.tile(np.arange(pool, dtype=np.int32), (rows, 1)))
    assert (val[-1] == 1.0).all()
    if pool >= 4:  # a short row, and invalid entries in it: the valid positions in pool order
        cols2 = cols.copy()
        cols2[0, 1], cols2[0, 2] = -1, n
        plen = np.full(rows, pool, np.int32)
        plen[0] = pool - 1
        pos, ln, _, _ = run(cols2, s, vectors, 1.0, pool, pool_len=plen)
        keep = [p for p in range(pool - 1) if p not in (1, 2)]
        assert ln[0] == len(keep) and pos[0, : ln[0]].tolist() == keep and (pos[0, ln[0]:] == -1).all()
        assert np.array_equal(pos[1:], np.tile(np.arange(pool, dtype=np.int32), (rows - 1, 1)))


@pytest.mark.parametrize("d,c,per,f64", [(8, 5, 4, False), (64, 7, 9, True), (200, 3, 100, False), (64, 40, 20, True)])
def test_lambda_zero_on_clusters(device, d, c, per, f64):
    """(d): c clusters of identical vectors, mutually orthogonal (cosine 1
    inside a cluster, 0 across, exactly: one non-zero component, a power of
    two). lambda = 0: every value is -maxsim. The first pick is position 0 (all
    values 0), the next c - 1 picks are the first position of every other
    cluster in pool order (value 0 against -1), then every entry has value -1
    and the rest follows in pool order."""
    rng = np.random.default_rng(c * per)
    pool = c * per
    cluster = rng.permutation(np.repeat(np.arange(c), per))  # the cluster of each position
    vectors = np.zeros((pool, d), np.float32)
    vectors[np.arange(pool), cluster % d] = 2.0 ** rng.integers(-3, 4, pool)
    assert c <= d
    cols = np.arange(pool, dtype=np.int64)[None, :]
    s = -np.sort(-rng.standard_normal((1, pool)))
    s = s if f64 else s.astype(np.float32)
    pos, ln, val, inv = run(cols, s, vectors, 0.0, pool)
    first = sorted(int(np.flatnonzero(cluster == k)[0]) for k in range(c))
    assert first[0] == 0
    rest = [p for p in range(pool) if p not in first]
    assert pos[0].tolist() == first + rest and ln[0] == pool
    assert (val[0, :c] == 0.0).all() and (val[0, c:] == -1.0).all()
    check_valid((pos, ln, val, inv), cols, s, vectors, 0.0, pool, d)


@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_duplicates_with_equal_scores_take_the_smaller_position(device, lam):
    """(e): positions 2 k and 2 k + 1 hold two items with the same vector and
    the same score: equal values at every step, so the even one is always
    picked before its twin, in every wave and across waves (pool 300: five
    waves' worth of positions, two per thread)."""
    rng = np.random.default_rng(17)
    half, d = 150, 24
    base = rng.standard_normal((half, d)).astype(np.float32)
    vectors = np.repeat(base, 2, axis=0)
    cols = rng.permutation(half)[:, None] * 2 + np.array([0, 1])[None, :]
    cols = cols.reshape(1, -1).astype(np.int64)
    s = np.repeat(-np.sort(-rng.standard_normal(half)).astype(np.float32), 2)[None, :]
    got = run(cols, s, vectors, lam, 2 * half)
    pos = got[0][0].tolist()
    rank = {p: t for t, p in enumerate(pos)}
    assert sorted(pos) == list(range(2 * half))
    assert all(rank[2 * k] < rank[2 * k + 1] for k in range(half))
    check_valid(got, cols, s, vectors, lam, 2 * half, d)


def _invalid_inputs(f64):
    rng = np.random.default_rng(23)
    n, d, pool = 90, 20, 70
    vectors = rng.standard_normal((n, d)).astype(np.float32)
    vectors[5] = 0.0                      # zero norm
    vectors[6, 3], vectors[7, 0] = np.inf, np.nan  # inv_norm 0 whatever the components are
    cols = np.stack([rng.permutation(n)[:pool] for _ in range(8)]).astype(np.int64)
    s = -np.sort(-rng.standard_normal((8, pool)), axis=1)
    cols[0, [0, 9, 69]] = -1                       # -1 columns, the best entry among them
    cols[1, [1, 64, 65]] = [n, n + 1000, 2 ** 40]  # columns >= n
    cols[2, :10] = [5, 6, 7, 5, 6, 7, 10, 11, 12, 13]  # zero-norm rows and rows with inf / NaN components
    s[3, [0, 4, 20, 21, 60]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]  # non-finite scores
    cols[4] = -1                                   # no valid entry
    cols[5, 3:] = -7                               # three valid entries: fewer than top_n
    s[6, :] = np.nan                               # no finite score at all
    plen = np.array([70, 70, 70, 70, 70, 70, 70, 33], np.int32)  # a short row
    plen[1] = 66
    return vectors, cols, (s if f64 else s.astype(np.float32)), plen, d


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("lam", [0.0, 0.4, 1.0])
def test_invalid_entries(device, lam, f64):
    """(f): each row one kind of invalid input, all against the oracle."""
    vectors, cols, s, plen, d = _invalid_inputs(f64)
    for pool_len in (plen, None, np.array([0, -3, 1, 1000, 70, 2, 5, 70], np.int32)):
        got = run(cols, s, vectors, lam, 12, pool_len=pool_len)
        want = check_valid(got, cols, s, vectors, lam, 12, d, pool_len=pool_len)
        assert got[3][5] == 0.0 and got[3][6] == 0.0 and got[3][7] == 0.0
        if pool_len is plen:
            assert got[1].tolist() == [12, 12, 12, 12, 0, 3, 12, 12]
            assert (got[0][4] == -1).all()
            assert np.isneginf(got[2][6]).all() and got[0][6].tolist() == list(range(12))
        if 0.0 < lam < 1.0 and want.gap[[0, 1, 7]].min() > 1e3 * mo.tol(d):
            assert np.array_equal(got[0][[0, 1, 7]], want.pos[[0, 1, 7]])


def test_strided_views_and_wrapper_errors(device):
    """pool and scores as column slices of wider matrices (pool_ld, scores_ld
    > pool_n) and vectors as a slice of wider rows (ld > d)."""
    import torch
    from src import _hrec

    case = mo.Case(50, 100, 10, 5, 0.7, False)
    pool, s, vectors = mo.case_inputs(case)
    want = case_run(case)
    wide_v = torch.zeros((vectors.shape[0], 64), device="cuda")
    wide_v[:, :50] = torch.as_tensor(vectors, device="cuda")
    wide_p = torch.full((5, 130), -1, dtype=torch.int64, device="cuda")
    wide_p[:, :100] = torch.as_tensor(pool, device="cuda")
    wide_s = torch.full((5, 120), float("nan"), device="cuda")
    wide_s[:, :100] = torch.as_tensor(s, device="cuda")
    inv = _hrec.row_inv_norms(wide_v, 50)
    pos, ln, val = _hrec.mmr_rerank(wide_p[:, :100], wide_s[:, :100], wide_v, inv, 0.7, 10, d=50, want_value=True)
    assert np.array_equal(pos.cpu().numpy(), want[0]) and np.array_equal(val.cpu().numpy(), want[2])
    with pytest.raises(_hrec.HrecError):
        _hrec.mmr_rerank(wide_p[:, :100], wide_s[:, :99], wide_v, inv, 0.7, 10, d=50)
    with pytest.raises(_hrec.HrecError):
        _hrec.mmr_rerank(wide_p[:, :100], wide_s[:, :100], wide_v, inv, 0.7, 101, d=50)
    with pytest.raises(_hrec.HrecError):
        _hrec.mmr_rerank(wide_p[:, :100], wide_s[:, :100], wide_v, inv, 1.5, 10, d=50)
