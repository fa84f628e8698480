"""GPU: hrec_row_inv_norms and hrec_list_quality against the numpy oracle
(tests/list_quality_oracle.py) at the smallest shapes where the kernel can go
wrong: every components-per-lane count (d 1..64, 65..128, 129..192, 193..256)
with ld > d, lists of 1, 2, 10, 70 (two strides of 64) and 1024 columns, one
block, two blocks and more blocks than the reducer has lanes.

Tolerances: diversity and unexpectedness 8 (d + m + g) 2^-53
absolute per row; a table mean 2 m 2^-53 max|table|. Counts, exposure and the
defined / undefined pattern are exact."""
import functools

import numpy as np
import pytest

import list_quality_oracle as lq

pytestmark = pytest.mark.gpu

ZERO, INF, NANV, HOT = 0, 1, 2, 3  # items: zero vector, an infinite component, a NaN component, in every list


@functools.lru_cache(maxsize=None)
def make_case(d, list_n, n_rows, n, n_tab, with_hist, seed=0):
    """Host arrays of one call and the oracle's answer (computed once)."""
    rng = np.random.default_rng([seed, d, list_n, n_rows, n])
    ld = d + 3
    vec = (rng.standard_normal((n, ld)) + 0.25).astype(np.float32)
    vec[:, d:] = 7.0  # padding: must not be read as components
    vec[ZERO, :d] = 0.0
    vec[INF, 0] = np.inf
    vec[NANV, d - 1] = np.nan
    others = np.arange(4, n)  # the special items are placed by hand: the entries of a list are distinct
    lists = np.empty((n_rows, list_n + 2), np.int64)  # lists_ld > list_n
    lists[:, list_n:] = n - 1  # past the list: must not be read as entries
    for r in range(n_rows):
        row = rng.permutation(others)[:list_n]
        if list_n >= 10:
            row[1], row[2], row[4] = ZERO, INF, NANV
        row[-1] = HOT  # one item in every list
        if list_n >= 2 and r % 3 == 1:
            row[0] = -1
        if list_n >= 10 and r % 3 == 2:
            row[3], row[list_n // 2] = n, n + 5
        lists[r, :list_n] = row
    pattern = [list_n, 0, 1, max(1, list_n // 2), list_n + 5, -2, list_n]
    lens = np.array([pattern[r % len(pattern)] for r in range(n_rows)], np.int32)
    hist_rows = indptr = hcols = history = None
    if with_hist:
        long_seg = np.sort(rng.integers(-1, n + 2, 600))  # duplicates, -1 and >= n inside
        segs = [np.zeros(0, np.int64), long_seg, np.sort(rng.permutation(n)[:3]), np.array([-1]),
                np.sort(rng.permutation(n)[:70])]
        indptr = np.r_[0, np.cumsum([s.size for s in segs])].astype(np.int64)
        hcols = np.concatenate(segs).astype(np.int32)
        hist_rows = np.array([[1, -1, 0, 2, 3, 4][r % 6] for r in range(n_rows)], np.int64)
        history = [None if q < 0 else segs[q] for q in hist_rows]
    tables = None
    if n_tab:
        tables = rng.standard_normal((n_tab, n)) * 10.0
        tables[rng.random((n_tab, n)) < 0.2] = np.nan
        tables[n_tab - 1, HOT] = np.nan
        if n_tab == 4:
            tables[2] = np.nan  # a table without a value: NaN everywhere, counted nowhere
    vals, cnt, exposure = lq.per_row(lists[:, :list_n], lens, vec, d, history, tables)
    for a in (vec, lists, lens, vals, cnt, exposure):
        a.setflags(write=False)
    return dict(d=d, ld=ld, n=n, list_n=list_n, n_rows=n_rows, vec=vec, lists=lists, lens=lens,
                hist=(hist_rows, indptr, hcols) if with_hist else None, tables=tables, vals=vals, cnt=cnt,
                exposure=exposure)


def run(device, case, rows=slice(None), exposure=None, sums=None, inv=None):
    import torch
    from src import _hrec

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    vec = dev(case["vec"])
    if inv is None:
        inv = _hrec.row_inv_norms(vec, case["d"])
    hist = None
    if case["hist"] is not None:
        hist = (dev(case["hist"][0][rows]), dev(case["hist"][1]), dev(case["hist"][2]))
    tables = None if case["tables"] is None else dev(case["tables"])
    lists = dev(case["lists"])[rows, : case["list_n"]]  # a view: row stride list_n + 2
    return _hrec.list_quality(lists, vec, inv, list_len=dev(case["lens"][rows]), history=hist, tables=tables,
                              exposure=exposure, sums=sums, d=case["d"])


def tolerances(case, cnt):
    """[n_rows, 2 + n_tab] absolute bounds for the rows of cnt."""
    tol = np.empty(cnt.shape)
    m, g = cnt[:, 0].astype(np.float64), cnt[:, 1].astype(np.float64)
    tol[:, 0] = 8 * (case["d"] + m) * lq.U53
    tol[:, 1] = 8 * (case["d"] + m + g) * lq.U53
    if case["tables"] is not None:
        for t in range(case["tables"].shape[0]):
            tmax = np.nanmax(np.abs(case["tables"][t])) if not np.isnan(case["tables"][t]).all() else 0.0
            tol[:, 2 + t] = 2 * m * lq.U53 * tmax
    return tol


def check_rows(case, per_row, row_n, rows=slice(None)):
    vals, cnt = case["vals"][rows], case["cnt"][rows]
    got = per_row.cpu().numpy()
    assert (row_n.cpu().numpy() == cnt).all()
    assert (np.isnan(got) == np.isnan(vals)).all(), (np.argwhere(np.isnan(got) != np.isnan(vals)))
    err = np.abs(np.where(np.isnan(vals), 0.0, got - vals))
    tol = tolerances(case, cnt)
    print("max error / bound per column:", (err / np.maximum(tol, 1e-300)).max(axis=0), "max error:", err.max(axis=0))
    assert (err <= tol).all(), (err.max(axis=0), tol.max(axis=0))


def check_sums(case, sums, rows=slice(None)):
    """The sums over rows: each row within its bound, plus the two summations'
    own error (R - 1) 2^-53 sum |v| each; the counts exactly."""
    vals, cnt = case["vals"][rows], case["cnt"][rows]
    want = lq.column_sums(vals)
    got = sums.cpu().numpy()
    ncol = vals.shape[1]
    assert (got[ncol:] == want[ncol:]).all()
    tol = np.where(np.isnan(vals), 0.0, tolerances(case, cnt)).sum(axis=0)
    tol += 2 * vals.shape[0] * lq.U53 * np.abs(np.nan_to_num(vals)).sum(axis=0)
    assert (np.abs(got[:ncol] - want[:ncol]) <= tol).all(), (got[:ncol] - want[:ncol], tol)


@pytest.mark.parametrize("d", [1, 50, 64, 65, 200, 256])
def test_inv_norms(device, d):
    import torch
    from src import _hrec

    case = make_case(d, 10, 5, 300, 1, True)
    got = _hrec.row_inv_norms(torch.as_tensor(case["vec"], device=device), d).cpu().numpy()
    want = lq.inv_norms(case["vec"], d)
    assert (got[[ZERO, INF, NANV]] == 0.0).all() and ((got == 0.0) == (want == 0.0)).all()
    # d squares and d - 1 additions, a square root (halves it), a division: (d / 2 + 2) 2^-53 on each side
    assert (np.abs(got - want) <= (d + 4) * lq.U53 * want).all()


@pytest.mark.parametrize("d", [1, 50, 64, 65, 200, 256])
def test_every_width(device, d):
    """Lengths 0, 1, short, full, beyond and negative; -1 and >= n inside lists
    and histories; zero, infinite and NaN vectors; history rows -1, empty, 600
    entries, invalid only; one table with NaN entries."""
    case = make_case(d, 10, 7, 300, 1, True)
    per_row, row_n, exposure, sums = run(device, case)
    check_rows(case, per_row, row_n)
    assert (exposure.cpu().numpy() == case["exposure"]).all()
    check_sums(case, sums)


@pytest.mark.parametrize("list_n,n", [(1, 40), (2, 40), (70, 300), (1024, 3000)])
def test_every_list_length(device, list_n, n):
    case = make_case(50, list_n, 5, n, 4, True)
    per_row, row_n, exposure, sums = run(device, case)
    check_rows(case, per_row, row_n)
    assert (exposure.cpu().numpy() == case["exposure"]).all()
    check_sums(case, sums)


@pytest.mark.parametrize("n_rows", [1, 5, 261])
def test_row_counts_and_contended_exposure(device, n_rows):
    """One block, two blocks, and 66 blocks: lane 0 and lane 1 of the second
    launch add two partials each. Item HOT stands in every list."""
    case = make_case(65, 10, n_rows, 120, 0, False)
    per_row, row_n, exposure, sums = run(device, case)
    check_rows(case, per_row, row_n)
    got = exposure.cpu().numpy()
    assert (got == case["exposure"]).all()
    want_hot = int(sum(HOT in lq.valid_entries(case["lists"][r, :10], 120, case["lens"][r]) for r in range(n_rows)))
    assert got[HOT] == want_hot
    check_sums(case, sums)
    assert np.isnan(per_row.cpu().numpy()[:, 1]).all()  # no history CSR: unexpectedness undefined everywhere


def test_no_tables_no_history_full_lists(device):
    """list_len NULL: every list is full."""
    import torch
    from src import _hrec

    case = make_case(64, 10, 5, 80, 0, False)
    vec = torch.as_tensor(case["vec"], device=device)
    lists = torch.as_tensor(np.ascontiguousarray(case["lists"][:, :10]), device=device)
    per_row, row_n, exposure, sums = _hrec.list_quality(lists, vec, _hrec.row_inv_norms(vec, 64), d=64)
    vals, cnt, expo = lq.per_row(case["lists"][:, :10], None, case["vec"], 64)
    full = dict(case, vals=vals, cnt=cnt)
    check_rows(full, per_row, row_n)
    assert (exposure.cpu().numpy() == expo).all()
    assert tuple(per_row.shape) == (5, 2) and sums.numel() == 4


def test_two_calls_accumulate(device):
    """Rows 0..99 then 100..260 into one exposure vector and one set of sums."""
    case = make_case(200, 10, 261, 150, 4, True)
    a = run(device, case, slice(0, 100))
    b = run(device, case, slice(100, 261), exposure=a[2], sums=a[3])
    check_rows(case, a[0], a[1], slice(0, 100))
    check_rows(case, b[0], b[1], slice(100, 261))
    assert b[2].data_ptr() == a[2].data_ptr() and b[3].data_ptr() == a[3].data_ptr()
    assert (b[2].cpu().numpy() == case["exposure"]).all()
    check_sums(case, b[3])


def test_equal_inputs_give_equal_bits(device):
    case = make_case(256, 70, 261, 300, 4, True)
    a, b = run(device, case), run(device, case)
    check_rows(case, a[0], a[1])
    for x, y in ((a[0], b[0]), (a[3], b[3])):
        assert (x.cpu().numpy().view(np.int64) == y.cpu().numpy().view(np.int64)).all()
    assert (a[2] == b[2]).all() and (a[1] == b[1]).all()
