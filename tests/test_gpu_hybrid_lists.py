"""GPU: hrec_hybrid_lists (through _hrec.hybrid_lists) against the numpy oracle
of its contract (tests/hybrid_lists_oracle.py) and, per row, against
_hrec.fuse_topk(a_r, t_r, als_wins, n, minmax=...) with the excluded entries
deleted: indices, the f64 bits of the values (NaN compared as NaN), out_len,
out_minmax and the overflow flag. Entries past a row's length are not looked
at. In mode 0 a row the oracle's predicate (row_overflows: the sample bound
admits more live columns than HYBRID_LISTS_CAP) says is cut must raise the
flag and is not compared; every other row must be right and the flag must be
0 when no row is cut.

The overflow case: a row of n = HYBRID_LISTS_CAP + 100 identical scores with
a quarter of its columns excluded keeps only 3/4 of them, fewer than the list
holds (the list must hold the sample, so CAP >= SAMPLE >= 1024), so no flag
can be due there. Both shapes are tested: that one (complete answer, flag 0)
and a row with CAP + 100 identical scores LEFT after a quarter is excluded
(flag 1, the other rows right, mode 1 complete)."""
import numpy as np
import pytest
import torch
from hybrid_lists_oracle import excluded_set, fuse_row, ranking, row_overflows, substitute

pytestmark = pytest.mark.gpu

TOP_KS = (1, 8, 9, 64, 65, 1024)


def _consts():
    from src import _hrec

    return _hrec.HYBRID_LISTS_SAMPLE, _hrec.HYBRID_LISTS_CAP


def _dev_mat(x, pad, dev, fill):
    """x on the device as an [n_rows, n] view of an [n_rows, ld] buffer whose
    padding holds `fill` (ld = n, or n rounded up to 8 plus 8)."""
    n_rows, n = x.shape
    ld = n if not pad else (n + 7) // 8 * 8 + 8
    buf = torch.full((n_rows, ld), fill, dtype=torch.float32, device=dev)
    buf[:, :n] = torch.as_tensor(x, device=dev)
    return buf[:, :n]


def _csr(sets, rng=None):
    """(excl_rows, excl_indptr, excl_cols) of per-row column lists (None: a
    negative row id). The CSR rows are stored in a shuffled order when rng is
    given, so excl_rows is a real indirection."""
    live = [r for r, s in enumerate(sets) if s is not None]
    order = list(rng.permutation(len(live))) if rng is not None else list(range(len(live)))
    rows = np.full(len(sets), -1, np.int64)
    indptr, cols = [0], []
    for q, k in enumerate(order):
        r = live[k]
        rows[r] = q
        cols += list(sets[r])
        indptr.append(len(cols))
    if any(s is None for s in sets):
        rows[[r for r, s in enumerate(sets) if s is None]] = -np.arange(1, 1 + sum(s is None for s in sets))
    return rows, np.asarray(indptr, np.int64), np.asarray(cols, np.int32)


def _excl_dev(excl, dev):
    return None if excl is None else tuple(torch.as_tensor(x, device=dev) for x in excl)


def _same_values(got, exp, msg):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=msg)
    ok = ~np.isnan(exp)
    np.testing.assert_array_equal(got[ok].view(np.int64), exp[ok].view(np.int64), err_msg=msg)


class Ref:
    """The expected full ranking of every row (computed once per input):
    the oracle's, asserted equal to hrec_fuse_topk's for that row."""

    def __init__(self, dev, als, tt, als_wins, fb=None, excl=None):
        from src import _hrec

        self.n_rows, self.n = als.shape
        self.rows = []
        for r in range(self.n_rows):
            a = substitute(als[r], fb)
            fused, mm = fuse_row(a, tt[r], als_wins)
            order = ranking(fused)
            m = torch.empty(4, dtype=torch.float64, device=dev)
            i, s, _ = _hrec.fuse_topk(torch.as_tensor(a, device=dev), torch.as_tensor(tt[r], device=dev), als_wins,
                                      self.n, want_fused=False, minmax=m)
            np.testing.assert_array_equal(i.cpu().numpy(), order, err_msg=f"fuse_topk row {r}")
            _same_values(s.cpu().numpy(), fused[order], f"fuse_topk row {r}")
            np.testing.assert_array_equal(m.cpu().numpy(), mm, err_msg=f"fuse_topk minmax row {r}")
            gone = excluded_set(excl, r, self.n)
            mask = np.zeros(self.n, bool)
            mask[gone] = True
            self.rows.append((order[~mask[order]], fused, mm, gone))

    def check(self, res, top_k, mode, expect_overflow=None):
        sample, cap = _consts()
        idx, val, lens, over, mm = (x.cpu().numpy() for x in res)
        kk = min(top_k, self.n)
        assert idx.shape == val.shape == (self.n_rows, kk)
        cut = []
        for r, (kept, fused, m, gone) in enumerate(self.rows):
            msg = f"row {r} top_k {top_k} mode {mode}"
            L = min(kk, len(kept))
            assert lens[r] == L, msg
            np.testing.assert_array_equal(mm[r], m, err_msg=msg)
            if mode == 0 and row_overflows(fused, gone, kk, sample, cap):
                cut.append(r)
                continue
            np.testing.assert_array_equal(idx[r, :L], kept[:L], err_msg=msg)
            _same_values(val[r, :L], fused[kept[:L]], msg)
        assert int(over[0]) == (1 if cut else 0), (top_k, mode, cut)
        if expect_overflow is not None:
            assert bool(cut) == expect_overflow
        return cut


def _run(dev, als, tt, top_k, als_wins, fb=None, excl=None, mode=0, pad=False):
    from src import _hrec

    return _hrec.hybrid_lists(_dev_mat(als, pad, dev, float("nan")), _dev_mat(tt, pad, dev, 3e38), top_k, als_wins,
                              fallback=None if fb is None else torch.as_tensor(fb, device=dev),
                              excl=_excl_dev(excl, dev), mode=mode, want_minmax=True)


def _shape_ns():
    sample, _ = _consts()
    return (1, 63, 64, 65, 1025, sample - 1, sample, sample + 37, 20011)


@pytest.mark.parametrize("n_pos", range(9))
def test_shapes(device, n_pos):
    """Every n with n_rows 1 / 3 / 65, both leading dimensions, both weight
    choices, every top_k (top_k > n included) and both modes; half of the
    inputs carry a random exclusion (about a tenth of each row)."""
    n = _shape_ns()[n_pos]
    rng = np.random.default_rng(100 + n_pos)
    for n_rows, pad, als_wins, with_excl in ((1, False, True, False), (3, True, False, True), (65, True, True, True),
                                             (65, False, False, False)):
        als = rng.normal(size=(n_rows, n)).astype(np.float32)
        tt = rng.normal(size=(n_rows, n)).astype(np.float32)
        excl = None
        if with_excl:
            excl = _csr([np.flatnonzero(rng.random(n) < 0.1) for _ in range(n_rows)], rng)
        ref = Ref(device, als, tt, als_wins, excl=excl)
        for top_k in TOP_KS:
            cut = ref.check(_run(device, als, tt, top_k, als_wins, excl=excl, mode=0, pad=pad), top_k, 0)
            ref.check(_run(device, als, tt, top_k, als_wins, excl=excl, mode=1, pad=pad), top_k, 1)
            if n <= _consts()[0]:
                assert not cut  # the row is the sample: never an overflow


def _exclusion_sets(rng, als, tt, n, sample):
    fused, _ = fuse_row(substitute(als[5]), tt[5], True)
    return [
        None,                                                   # 0: a negative excl_rows entry
        [],                                                     # 1: an empty row
        list(range(n)),                                         # 2: everything
        sorted(set(range(n)) - {7, sample + 5, n - 1}),         # 3: all but 3
        sorted(rng.choice(n, 500, replace=False).tolist()),     # 4: 500 random columns
        sorted(ranking(fused)[:500].tolist()),                  # 5: the row's own top 500
        [-9, -1, 3, 3, 3, 17, 17, sample + 1, sample + 1, n, n + 5, 2 ** 31 - 1],  # 6: < 0, >= n, duplicates
        sorted(rng.choice(sample, 300, replace=False).tolist()),              # 7: only inside the sample
        sorted((sample + rng.choice(n - sample, 300, replace=False)).tolist()),  # 8: only outside it
    ]


@pytest.mark.parametrize("als_wins", [True, False])
def test_exclusion_cases(device, als_wins):
    sample, _ = _consts()
    n = sample + 900
    rng = np.random.default_rng(7)
    als = rng.normal(size=(9, n)).astype(np.float32)
    tt = rng.normal(size=(9, n)).astype(np.float32)
    tt[6, [3, 40, sample + 1]] = np.nan  # NaN entries next to excluded ones
    sets = _exclusion_sets(rng, als, tt, n, sample)
    excl = _csr(sets, rng)
    ref = Ref(device, als, tt, als_wins, excl=excl)
    assert [len(k) for k, *_ in ref.rows] == [n, n, 0, 3, n - 500, n - 500, n - 3, n - 300, n - 300]
    for top_k in (8, 64, 1024):
        for mode in (0, 1):
            res = _run(device, als, tt, top_k, als_wins, excl=excl, mode=mode, pad=True)
            ref.check(res, top_k, mode)
            lens = res[2].cpu().numpy()
            assert lens[2] == 0 and lens[3] == 3
    # all three pointers null: nothing excluded
    ref0 = Ref(device, als, tt, als_wins)
    for mode in (0, 1):
        res = _run(device, als, tt, 8, als_wins, mode=mode)
        ref0.check(res, 8, mode)
        assert res[2].cpu().numpy().tolist() == [8] * 9


@pytest.mark.parametrize("with_fb", [True, False])
def test_values(device, with_fb):
    """NaN ALS rows and entries with and without the fallback vector, NaN
    two-tower entries (last, in index order, never displacing a deleted
    column), +-0.0 and a constant row."""
    sample, _ = _consts()
    n = sample + 404
    rng = np.random.default_rng(11)
    als = rng.normal(size=(6, n)).astype(np.float32)
    tt = rng.normal(size=(6, n)).astype(np.float32)
    fb = rng.random(n) * 5 + 1 / 3  # f64 values that are not f32-representable
    assert np.any(fb.astype(np.float32).astype(np.float64) != fb)
    als[0] = np.nan                                    # a cold user
    als[1, rng.choice(n, 60, replace=False)] = np.nan  # unknown items
    tt[2, rng.choice(n, n - 5, replace=False)] = np.nan   # five numbers, the rest NaN
    tt[3] = np.nan                                     # nothing but NaN on the two-tower side
    als[4] = rng.choice(np.array([0.0, -0.0], np.float32), n)
    tt[4] = rng.choice(np.array([0.0, -0.0, 1.0], np.float32), n)
    als[5], tt[5] = 2.5, -1.25                         # constant
    sets = [None, [], sorted(rng.choice(n, 200, replace=False).tolist()),
            sorted(rng.choice(n, n - 4, replace=False).tolist()), [], [0, 1, 2]]
    excl = _csr(sets, rng)
    ref = Ref(device, als, tt, True, fb=fb if with_fb else None, excl=excl)
    if with_fb:
        assert not np.isnan(ref.rows[0][1]).any()
    else:
        assert np.isnan(ref.rows[0][1]).all() and ref.rows[0][0][:3].tolist() == [0, 1, 2]
    assert np.isnan(ref.rows[3][1]).all() and len(ref.rows[3][0]) == 4
    for top_k in (8, 1024):
        for mode in (0, 1):
            ref.check(_run(device, als, tt, top_k, True, fb=fb if with_fb else None, excl=excl, mode=mode), top_k,
                      mode)


def test_ties_keep_frame_order(device):
    """Quantised scores: a handful of distinct fused values over thousands of
    columns. Inside the sample size mode 0 ranks everything; above it the
    ties at the bound fill the list (flag) and mode 1 answers."""
    sample, cap = _consts()
    rng = np.random.default_rng(13)
    for n, expect in ((sample - 96, False), (10 * cap, True)):  # ~ n / 7.5 live columns share the best value
        als = rng.integers(0, 3, (3, n)).astype(np.float32)
        tt = rng.integers(0, 2, (3, n)).astype(np.float32)
        excl = _csr([np.flatnonzero(rng.random(n) < 0.2) for _ in range(3)])
        ref = Ref(device, als, tt, False, excl=excl)
        kept, fused = ref.rows[0][:2]
        assert len(np.unique(fused)) <= 6 and np.all(np.diff(kept[fused[kept] == fused[kept[0]]]) > 0)
        for top_k in (9, 1024):
            ref.check(_run(device, als, tt, top_k, False, excl=excl, mode=0), top_k, 0, expect_overflow=expect)
            ref.check(_run(device, als, tt, top_k, False, excl=excl, mode=1), top_k, 1)


def test_overflow(device):
    sample, cap = _consts()
    rng = np.random.default_rng(17)
    for n, expect in ((cap + 100, False), ((cap + 100) * 4 // 3 + 4, True)):
        als = rng.normal(size=(3, n)).astype(np.float32)
        tt = rng.normal(size=(3, n)).astype(np.float32)
        als[1], tt[1] = 0.5, 0.25                          # identical scores
        gone = np.arange(0, n, 4)                          # a quarter of the columns
        excl = _csr([[], gone.tolist(), gone[:50].tolist()])
        ref = Ref(device, als, tt, True, excl=excl)
        assert (n - len(gone) > cap) == expect
        for top_k in (8, 65):
            cut = ref.check(_run(device, als, tt, top_k, True, excl=excl, mode=0), top_k, 0, expect_overflow=expect)
            assert cut == ([1] if expect else [])          # rows 0 and 2 were compared and are right
            res = _run(device, als, tt, top_k, True, excl=excl, mode=1)
            ref.check(res, top_k, 1)
            first = np.setdiff1d(np.arange(n), gone)[:top_k]
            np.testing.assert_array_equal(res[0][1].cpu().numpy(), first)  # the first kk non-excluded indices
            assert int(res[3].item()) == 0


def test_modes_agree(device):
    """A served shape in small: 65 rows, 20011 columns, each row's own top
    500 excluded, top 10: mode 0 does not overflow and equals mode 1."""
    rng = np.random.default_rng(19)
    n = 20011
    als = rng.normal(size=(65, n)).astype(np.float32)
    tt = rng.normal(size=(65, n)).astype(np.float32)
    sets = [sorted(ranking(fuse_row(substitute(als[r]), tt[r], True)[0])[:500].tolist()) for r in range(65)]
    excl = _csr(sets, rng)
    a = _run(device, als, tt, 10, True, excl=excl, mode=0, pad=True)
    b = _run(device, als, tt, 10, True, excl=excl, mode=1, pad=True)
    assert int(a[3].item()) == 0 and int(b[3].item()) == 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert a[2].cpu().numpy().tolist() == [10] * 65
    for r in (0, 64):
        assert not set(a[0][r].cpu().numpy().tolist()) & set(sets[r])
