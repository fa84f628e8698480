"""GPU: hrec_cosine_topk against the numpy oracle (tests/cosine_oracle.py):
np.array_equal on out_idx, on the bits of out_val and on out_len, in every
mode. Both sides take the SAME inv_norm: the kernel's hrec_row_inv_norms, read
back. The oracle's sims of a case are computed once and shared by its top_k,
skip_self and mode variants."""
import numpy as np
import pytest

import cosine_oracle as co

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)


class Case:
    """One matrix on the device with its inv_norm, its prepared operand and
    the oracle's sims for one query list."""

    def __init__(self, vectors, d, queries):
        import torch
        from src import _hrec

        self.host = np.ascontiguousarray(vectors, np.float32)
        self.d = d
        self.q = np.asarray(queries, np.int64)
        self.v = torch.as_tensor(self.host, device="cuda")
        self.inv_d = _hrec.row_inv_norms(self.v, d)
        self.items = _hrec.cosine_items(self.v, self.inv_d, d)
        self.q_d = torch.as_tensor(self.q, device="cuda")
        self.inv = self.inv_d.cpu().numpy()
        self.sims = co.sims(self.host, d, self.inv, self.q)

    def run(self, top_k, skip_self=True, min_sim=float("-inf"), mode=0):
        """(idx, val, len numpy, whether the first attempt raised *overflow)."""
        import torch
        from src import _hrec

        idx, val, ln, raised = _hrec.cosine_topk(self.v, self.inv_d, self.q_d, top_k, skip_self=skip_self,
                                                 min_sim=min_sim, mode=mode, items=self.items, d=self.d,
                                                 want_overflow=True)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), val.cpu().numpy(), ln.cpu().numpy(), raised

    def want(self, top_k, skip_self=True, min_sim=float("-inf")):
        return co.topk(self.host, self.d, self.inv, self.q, top_k, skip_self, min_sim, s=self.sims)

    def check(self, top_k, skip_self=True, min_sim=float("-inf"), modes=MODES):
        want = self.want(top_k, skip_self, min_sim)
        raised = {}
        for mode in modes:
            idx, val, ln, raised[mode] = self.run(top_k, skip_self, min_sim, mode)
            where = "top_k %d skip_self %d mode %d" % (top_k, skip_self, mode)
            assert np.array_equal(ln, want[2]), where
            assert np.array_equal(idx, want[0]), where
            assert np.array_equal(val.view(np.int64), want[1].view(np.int64)), where  # the bits, NaN padding included
        return raised


def padded(rng, n, d, pad):
    """[n, d + pad] with NaN in the padding columns (never read)."""
    v = np.full((n, d + pad), np.nan, np.float32)
    v[:, :d] = rng.standard_normal((n, d)).astype(np.float32)
    return v


# ld - d per d: 16-B row loads with and without padding (ld % 4 == 0), a tail of d % 4 components, scalar loads
PAD = {1: 0, 3: 3, 50: 3, 64: 4, 65: 3, 200: 0, 256: 3}


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
@pytest.mark.parametrize("d", [1, 3, 50, 64, 65, 200, 256])
def test_small_every_row_a_query(device, d, n):
    rng = np.random.default_rng(1000 * d + n)
    case = Case(padded(rng, n, d, PAD[d]), d, np.arange(n))
    for top_k in sorted({1, 10, 64, 65, max(n - 1, 1), n, 1024}):
        for skip_self in (1, 0):
            case.check(top_k, skip_self)


QUERIES = 64


def pruned_queries(rng, n):
    """64 queries: rows 0 and n - 1, a repeated row, a -1, the rest random."""
    q = rng.integers(0, n, QUERIES)
    q[:5] = (0, n - 1, 5, 5, -1)
    return q


_LARGE = {}


def large_case(n, d):
    if (n, d) not in _LARGE:
        rng = np.random.default_rng(n + d)
        _LARGE[(n, d)] = Case(rng.standard_normal((n, d)).astype(np.float32), d, pruned_queries(rng, n))
    return _LARGE[(n, d)]


@pytest.mark.parametrize("top_k", [10, 65, 1024])
@pytest.mark.parametrize("d", [50, 64, 256])
@pytest.mark.parametrize("n", [20011, 40000])
def test_pruned_forced(device, n, d, top_k):
    """Above the auto cut and no multiple of a tile. On random rows the kept
    lists stay far below their capacity for top_k 10 and 65 (about top_k n / S
    rows beat the sample bound, and the margin's band adds a few hundred), so
    the pruned arm answers these itself."""
    from src import _hrec

    assert n >= _hrec.COSINE_AUTO_CUT
    case = large_case(n, d)
    raised = case.check(top_k)
    print("overflow raised per mode", raised)
    assert not raised[1]
    if top_k <= 65:
        assert not raised[2] and not raised[0]
    lens = case.want(top_k)[2]
    assert lens[4] == 0 and (np.delete(lens, 4) == top_k).all()
    # the filter kept at least the answer (and the query's own row)
    import torch

    ws = torch.empty(_hrec.cosine_topk_workspace_bytes(QUERIES, n, top_k, d, 2), dtype=torch.uint8, device="cuda")
    _hrec.cosine_topk(case.v, case.inv_d, case.q_d, top_k, mode=2, items=case.items, d=d, ws=ws)
    kept = _hrec.cosine_topk_counts(ws, QUERIES, n, top_k, d).cpu().numpy()
    print("rows kept per query: mean %.1f max %d" % (np.delete(kept, 4).mean(), kept.max()))
    assert kept[4] == 0 and (np.delete(kept, 4) >= top_k).all()


def test_pruned_on_clustered_rows_beyond_the_sample(device):
    """Low-spread input at n = 20,011, where the sample (the first 8192 rows, or
    32768 for top_k > 64) is not the whole matrix for top_k 10: 200 clusters
    (rows = centre + 0.3 noise, so cosines inside a cluster lie near 0.92 and
    their ordering is decided far below the margin), exact duplicates and zero
    rows placed beyond the sample. A query's kept list is its cluster of about
    100 rows and the few that come within the band: far below the capacity, so
    the pruned arm must answer top_k 10 itself."""
    n, d = 20011, 64
    rng = np.random.default_rng(31)
    centres = rng.standard_normal((200, d))
    member = rng.integers(0, 200, n)
    v = (centres[member] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    v[15000:15040] = v[9000:9040]      # ties: the smaller column first
    v[[8500, 12000, n - 2]] = 0.0      # zero rows as candidates and as a query
    q = rng.integers(0, n, QUERIES)
    q[:8] = (0, n - 1, 9000, 15000, 9001, 12000, -1, 15039)
    case = Case(v, d, q)
    raised = case.check(10)
    print("clustered: overflow raised per mode", raised)
    assert raised == {0: False, 1: False, 2: False}
    case.check(10, skip_self=0)
    case.check(150, min_sim=0.5)
    case.check(1024)
    idx = case.want(10)[0]
    assert idx[2, 0] == 15000 and idx[3, 0] == 9000  # a row's duplicate is its nearest neighbour


def test_ties_every_row_three_times(device):
    rng = np.random.default_rng(21)
    base = rng.standard_normal((400, 16)).astype(np.float32)
    case = Case(np.concatenate([base, base, base]), 16, np.arange(1200))
    for top_k in (2, 10):
        case.check(top_k)
        case.check(top_k, skip_self=0)
    idx = case.want(2)[0]
    r = np.arange(1200)
    twins = np.sort(np.stack([(r + 400) % 1200, (r + 800) % 1200], 1), 1)
    assert np.array_equal(idx, twins)  # equal sims: the smaller column first


def test_zero_and_non_finite_rows(device):
    rng = np.random.default_rng(22)
    v = rng.standard_normal((500, 20)).astype(np.float32)
    v[[3, 100, 499]] = 0.0
    v[7, 2] = np.nan
    v[8, 19] = np.inf
    v[9, 0] = -np.inf
    v[10] = np.nan
    case = Case(v, 20, np.arange(500))
    assert (case.inv[[3, 100, 499, 7, 8, 9, 10]] == 0).all()
    for top_k in (10, 499):
        case.check(top_k)
    case.check(10, min_sim=0.0)
    case.check(10, skip_self=0, min_sim=-0.5)
    idx, val, ln, _ = case.run(10, mode=2)
    assert (val[3] == 0).all() and not np.signbit(val[3]).any() and idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10]
    assert (case.run(10, min_sim=0.0, mode=2)[2][[3, 7, 8, 9, 10]] == 0).all()


def test_tight_clusters_with_min_sim(device):
    rng = np.random.default_rng(23)
    centres = rng.standard_normal((8, 32))
    v = (np.repeat(centres, 100, 0) + 1e-3 * rng.standard_normal((800, 32))).astype(np.float32)
    v = v[rng.permutation(800)]
    case = Case(v, 32, np.arange(800))
    for top_k in (10, 150):
        case.check(top_k, min_sim=0.5)
    lens = case.want(150, min_sim=0.5)[2]
    assert (lens >= 99).all() and (lens < 150).any()  # a list ends where the similarities fall to 0.5


def test_identical_rows_overflow_and_the_redone_batch(device):
    """Every sim ties, so every kept list overflows whatever its capacity: the
    pruned arm raises *overflow (mode 2, and mode 0 from the cut on), and the
    wrapper's redone result is the oracle's: the first kk columns other than
    the query."""
    from src import _hrec

    # above the auto cut, and more rows than a list can hold (the cut lies below that capacity)
    n = max(_hrec.COSINE_AUTO_CUT, _hrec.COSINE_CAP) + 5
    row = np.random.default_rng(24).standard_normal(8).astype(np.float32)
    q = np.array([0, 1, 9, n - 1, -1, 7, 7, n // 2], np.int64)
    case = Case(np.tile(row, (n, 1)), 8, q)
    raised = case.check(10)
    assert raised[2] and raised[0] and not raised[1]
    idx = case.want(10)[0]
    assert idx[0].tolist() == list(range(1, 11)) and idx[2].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert idx[3].tolist() == list(range(10)) and (idx[4] == -1).all()
    # the driver: under auto the first flagged batch sends the rest to the exhaustive arm (one wasted pruned pass);
    # an explicit pruned mode is kept, and every batch is flagged and redone
    import torch
    from src import ranked_lists

    old = ranked_lists.SIMILAR_BATCH
    ranked_lists.SIMILAR_BATCH = 2
    try:
        for mode, flagged in ((0, 1), (2, 4), (1, 0)):
            stats = {}
            got = ranked_lists.similar(case.v, 8, q, 10, mode=mode, stats=stats)
            torch.cuda.synchronize()
            assert stats == {"batches": 4, "flagged": flagged}, (mode, stats)
            for g, w in zip(got, case.want(10)):
                assert np.array_equal(g.cpu().numpy(), w, equal_nan=True)
    finally:
        ranked_lists.SIMILAR_BATCH = old
    # just above the cut every row may still fit a list: right either way
    mid = Case(np.tile(row, (_hrec.COSINE_AUTO_CUT + 5, 1)), 8, np.array([0, 3, _hrec.COSINE_AUTO_CUT + 4, -1]))
    print("identical rows just above the cut: overflow raised per mode", mid.check(10))
    # below the cut auto takes the exhaustive arm: nothing to raise
    small = Case(np.tile(row, (_hrec.COSINE_AUTO_CUT - 1, 1)), 8, q[:3])
    assert small.check(10, modes=(0,)) == {0: False}


@pytest.mark.parametrize("mode", MODES)
def test_same_bits_on_a_second_call(device, mode):
    case = large_case(20011, 64)
    a, b = case.run(65, mode=mode), case.run(65, mode=mode)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                              y.view(np.int64) if y.dtype == np.float64 else y)


def test_similar_driver_batches_and_flags(device):
    """ranked_lists.similar over several sub-batches equals one oracle call."""
    import torch
    from src import ranked_lists

    case = large_case(20011, 64)
    q = np.concatenate([case.q, case.q[::-1]])
    old = ranked_lists.SIMILAR_BATCH
    ranked_lists.SIMILAR_BATCH = 50
    try:
        stats = {}
        cols, sims, lens = ranked_lists.similar(case.v, 64, q, 10, stats=stats)
    finally:
        ranked_lists.SIMILAR_BATCH = old
    torch.cuda.synchronize()
    assert stats == {"batches": 3, "flagged": 0}
    want = case.want(10)
    for got, w in zip((cols, sims, lens), want):
        g = got.cpu().numpy()
        assert np.array_equal(g[:QUERIES], w, equal_nan=True) and np.array_equal(g[QUERIES:], w[::-1], equal_nan=True)
