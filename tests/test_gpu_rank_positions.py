"""GPU: hrec_rank_positions through _hrec.rank_positions against the numpy
oracle of its contract (tests/rank_positions_oracle.py). Ranks, live / ranked /
unranked, AUC and the reciprocal rank exactly; sum_w_pr and sum_w within rtol
(m + 8) 2^-52, m the row's ranked labels; the totals within (n_rows + 8) 2^-52.
"""
import math
import warnings

import numpy as np
import pytest
import torch

import rank_positions_oracle as rpo

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ROWS = {1: 1, 63: 3, 64: 5, 65: 7, 1000: 37, 4097: 6}


def _chunk():
    from src import _hrec

    return _hrec.RP_CHUNK


def _label_counts():
    c = _chunk()
    return (3, 0, 1, c - 1, 17, c, c + 1, 2 * c + 3)


def _scores(rng, n_rows, n, dtype):
    s = rng.normal(3.0, 1.0, (n_rows, n))
    s[:, ::3] = np.round(s[:, ::3])  # ties
    return s.astype(dtype)


def _fused(als, tt, fb, wins):
    """The fused matrix in hrec_hybrid_lists' arithmetic (fb None: NaN ALS entries stay) and its minmax rows."""
    a = als.astype(np.float64) if fb is None else np.where(np.isnan(als), fb[None, :], als.astype(np.float64))
    amin, amax = np.nanmin(a, axis=1), np.nanmax(a, axis=1)
    tmin, tmax = np.nanmin(tt, axis=1), np.nanmax(tt, axis=1)
    ra, rt = amax - amin, tmax - tmin
    ascale = 1.0 / np.where(ra < 10 * np.finfo(np.float64).eps, 1.0, ra)
    tscale = (np.float32(1.0) / np.where(rt < 10 * np.finfo(np.float32).eps, np.float32(1.0), rt)).astype(np.float32)
    amin_ = 0.0 - amin * ascale
    tmin_ = (np.float32(0.0) - tmin * tscale).astype(np.float32)
    an = a * ascale[:, None] + amin_[:, None]
    tn = (tt * tscale[:, None]).astype(np.float32) + tmin_[:, None]
    w0 = np.where(wins != 0, 0.8, 0.2)[:, None]
    w1 = np.where(wins != 0, 0.2, 0.8)[:, None]
    return w0 * an + w1 * tn.astype(np.float64), np.stack([amin, amax, tmin.astype(np.float64),
                                                          tmax.astype(np.float64)], axis=1)


def _strided(a, device, pad=3):
    """The matrix as a device view whose row stride is its width + pad."""
    t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=torch.as_tensor(a).dtype, device=device)
    t[:, : a.shape[1]] = torch.as_tensor(a, device=device)
    return t[:, : a.shape[1]]


def _source_inputs(rng, source, n_rows, n, device, with_fallback=True, pad=3):
    """(the matrix the oracle ranks, the kernel's scores, extra keyword arguments)."""
    if source in ("f64", "f32"):
        s = _scores(rng, n_rows, n, np.float64 if source == "f64" else np.float32)
        return s, _strided(s, device, pad), {}
    als = _scores(rng, n_rows, n, np.float32)
    als[rng.random((n_rows, n)) < 0.1] = np.nan
    if n_rows > 1:
        als[-1, :] = np.nan  # a cold user
    fb = rng.normal(3.0, 1.0, n) if with_fallback else None
    kw = {} if fb is None else {"fallback": torch.as_tensor(fb, device=device)}
    if source == "als":
        seen = als.astype(np.float64) if fb is None else np.where(np.isnan(als), fb[None, :], als.astype(np.float64))
        return seen, _strided(als, device, pad), kw
    tt = _scores(rng, n_rows, n, np.float32)
    wins = (np.arange(n_rows) % 2).astype(np.int32)
    with warnings.catch_warnings():  # an all-NaN row without fallback: nanmin / nanmax say so
        warnings.simplefilter("ignore", RuntimeWarning)
        fused, mm = _fused(als, tt, fb, wins)
    mm = np.nan_to_num(mm, nan=0.0)  # an all-NaN row without fallback: every fused score is NaN whatever these are
    kw.update(tt=_strided(tt, device, pad), minmax=torch.as_tensor(mm, device=device),
              row_wins=torch.as_tensor(wins, device=device))
    return fused, _strided(als, device, pad), kw


def _labels(rng, n_rows, n, counts):
    """A label CSR with one more row than the call reads, read in a shuffled order; rows with count 0 are
    label_rows -1. Columns unsorted, with duplicates and some -1."""
    q_of = rng.permutation(n_rows + 1)[:n_rows]
    per = {}
    for i in range(n_rows):
        m = counts[i % len(counts)]
        c = rng.integers(0, n, m)
        if m > 2:
            c[rng.integers(0, m, max(1, m // 8))] = -1
            c[1] = c[0]  # a duplicate for sure
        per[int(q_of[i])] = c
    spare = [q for q in range(n_rows + 1) if q not in per]
    for q in spare:
        per[q] = rng.integers(0, n, 5)  # a CSR row no row of the call reads
    indptr, cols = [0], []
    for q in range(n_rows + 1):
        cols += per[q].tolist()
        indptr.append(len(cols))
    rows = np.array([int(q_of[i]) if counts[i % len(counts)] else -1 for i in range(n_rows)], np.int64)
    read = np.zeros(len(cols), bool)
    for r in rows[rows >= 0]:
        read[indptr[r]: indptr[r + 1]] = True
    return rows, np.array(indptr, np.int64), np.array(cols, np.int64), read


def _exclusion(rng, n_rows, n, lab):
    """Per row in turn: no exclusion row (-1), an empty list, a list overlapping the labels (with repeats), every column."""
    rows_l, indptr_l, cols_l, _ = lab
    rows, indptr, cols = [], [0], []
    for i in range(n_rows):
        kind = i % 4
        if kind == 0:
            rows.append(-1)
            continue
        if kind == 1:
            c = np.zeros(0, np.int64)
        elif kind == 2:
            own = cols_l[indptr_l[rows_l[i]]: indptr_l[rows_l[i] + 1]] if rows_l[i] >= 0 else np.zeros(0, np.int64)
            own = own[own >= 0]
            c = np.sort(np.concatenate([own[::2], own[:2], rng.integers(0, n, min(n, 9))]))
        else:
            c = np.arange(n)
        rows.append(len(indptr) - 1)
        cols += c.tolist()
        indptr.append(len(cols))
    return np.array(rows, np.int64), np.array(indptr, np.int64), np.array(cols, np.int64)


def _dev(lab, device):
    return (torch.as_tensor(lab[0], device=device), torch.as_tensor(lab[1], device=device),
            torch.as_tensor(lab[2].astype(np.int32), device=device))


def _check(got, exp, read, n_rows, weighted=False):
    from src import _hrec

    rank, row, row_n, sums = (x.cpu().numpy() for x in got)
    e_rank, e_row, e_row_n, e_sums = exp
    assert np.array_equal(rank[read], e_rank[read])
    assert np.array_equal(row_n, e_row_n)
    assert np.array_equal(row[:, :2], e_row[:, :2], equal_nan=True)  # AUC and reciprocal rank: exact
    for i in range(n_rows):
        tol = (int(e_row_n[i, 1]) + 8) * EPS
        for j in (2, 3):
            assert abs(row[i, j] - e_row[i, j]) <= tol * abs(e_row[i, j]), (i, j, row[i, j], e_row[i, j])
        if not weighted:
            assert row[i, 3] == e_row_n[i, 1]
    for name, g in zip(_hrec.RP_SUMS, sums.tolist()):
        e = e_sums[name]
        assert abs(g - e) <= (n_rows + 8) * EPS * abs(e), (name, g, e)


def _run(device, seen, s, lab, kw, excl=None, weight=None):
    from src import _hrec

    got = _hrec.rank_positions(s, _dev(lab, device), excl=None if excl is None else _dev(excl, device),
                               weight=None if weight is None else torch.as_tensor(weight, device=device), **kw)
    exp = rpo.batch_positions(seen, lab[0], lab[1], lab[2], weight, excl)
    return got, exp


@pytest.mark.parametrize("source", ["f64", "f32", "als", "fused"])
@pytest.mark.parametrize("n", sorted(ROWS))
def test_shapes_and_sources(device, n, source):
    n_rows = ROWS[n]
    rng = np.random.default_rng(100 * n + len(source))
    seen, s, kw = _source_inputs(rng, source, n_rows, n, device)
    counts = _label_counts()
    counts = counts[n % len(counts):] + counts[: n % len(counts)]
    lab = _labels(rng, n_rows, n, counts)
    excl = _exclusion(rng, n_rows, n, lab)
    weight = rng.integers(0, 4, lab[2].size).astype(np.float64) + rng.random(lab[2].size)
    got, exp = _run(device, seen, s, lab, dict(kw, source=source), excl, weight)
    _check(got, exp, lab[3], n_rows, weighted=True)
    got, exp = _run(device, seen, s, lab, dict(kw, source=source))
    _check(got, exp, lab[3], n_rows)


@pytest.mark.parametrize("count", [0, 1, 2, 3, 4, 5, 6, 7])
def test_every_label_count_alone(device, count):
    """One row whose labels fill a chunk exactly, fall one short, run over, or span three chunks."""
    m = _label_counts()[count]
    n = 700
    rng = np.random.default_rng(count)
    seen = _scores(rng, 2, n, np.float32)
    lab = _labels(rng, 2, n, (m, 5))
    got, exp = _run(device, seen, torch.as_tensor(seen, device=device), lab, {})
    _check(got, exp, lab[3], 2)
    excl = (np.array([0, 0], np.int64), np.array([0, 60], np.int64), np.arange(0, 120, 2, dtype=np.int64))
    got, exp = _run(device, seen, torch.as_tensor(seen, device=device), lab, {}, excl)
    _check(got, exp, lab[3], 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_ties_and_special_values(device, dtype):
    n, n_rows = 1000, 6
    rng = np.random.default_rng(17)
    s = rng.normal(0.0, 1.0, (n_rows, n))
    s[0, :] = 2.5                               # all equal: the list is column order
    s[1, :] = np.floor(rng.random(n) * 8) / 8   # eight levels
    s[2, rng.random(n) < 0.3] = np.nan
    s[3, :] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    s[4, ::5] = np.inf
    s[4, 1::5] = -np.inf
    s[4, 2::5] = np.nan
    s[5, :] = np.nan                            # all NaN: column order again
    s = s.astype(dtype)
    c = _chunk()
    lab = _labels(rng, n_rows, n, (40, c + 9, 200, 64, 300, 33))
    excl = _exclusion(rng, n_rows, n, lab)
    for x in (None, excl):
        got, exp = _run(device, s, _strided(s, device, 1), lab, {}, x)
        _check(got, exp, lab[3], n_rows)
    rank = got[0].cpu().numpy()
    lo, hi = lab[1][lab[0][0]], lab[1][lab[0][0] + 1]
    cols0 = lab[2][lo:hi]
    assert np.array_equal(rank[lo:hi][cols0 >= 0], cols0[cols0 >= 0])  # no exclusion row for row 0


@pytest.mark.parametrize("with_fallback", [True, False])
def test_fused_source_with_nan_als(device, with_fallback):
    n, n_rows = 1000, 5
    rng = np.random.default_rng(23 + with_fallback)
    seen, s, kw = _source_inputs(rng, "fused", n_rows, n, device, with_fallback=with_fallback, pad=4)
    lab = _labels(rng, n_rows, n, (30, 7, _chunk() + 1, 100, 12))
    excl = _exclusion(rng, n_rows, n, lab)
    got, exp = _run(device, seen, s, lab, dict(kw, source="fused"), excl)
    _check(got, exp, lab[3], n_rows)
    # the recomputed fused keys are the oracle matrix's: the f64 source over it gives the same bits
    got64, _ = _run(device, seen, torch.as_tensor(seen, device=device), lab, {}, excl)
    assert got[0].cpu().numpy()[lab[3]].tobytes() == got64[0].cpu().numpy()[lab[3]].tobytes()
    for a, b in zip(got[1:], got64[1:]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_two_calls_give_identical_bits(device):
    n, n_rows = 4097, 9
    rng = np.random.default_rng(31)
    seen, s, kw = _source_inputs(rng, "als", n_rows, n, device)
    lab = _labels(rng, n_rows, n, _label_counts())
    excl = _exclusion(rng, n_rows, n, lab)
    weight = rng.random(lab[2].size)
    runs = [_run(device, seen, s, lab, dict(kw, source="als"), excl, weight)[0] for _ in range(2)]
    assert runs[0][0].cpu().numpy()[lab[3]].tobytes() == runs[1][0].cpu().numpy()[lab[3]].tobytes()
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_no_labels_at_all_and_want_rank(device):
    from src import _hrec

    n, n_rows = 65, 3
    s = torch.as_tensor(_scores(np.random.default_rng(1), n_rows, n, np.float32), device=device)
    lab = (torch.full((n_rows,), -1, dtype=torch.int64, device=device), torch.zeros(1, dtype=torch.int64, device=device),
           torch.zeros(0, dtype=torch.int32, device=device))
    rank, row, row_n, sums = _hrec.rank_positions(s, lab, want_rank=False)
    assert rank is None
    assert np.isnan(row.cpu().numpy()[:, :2]).all() and (row.cpu().numpy()[:, 2:] == 0).all()
    assert row_n.cpu().numpy().tolist() == [[n, 0, 0]] * n_rows
    assert sums.cpu().numpy().tolist() == [0.0] * len(_hrec.RP_SUMS)
    assert math.isnan(rpo.metrics(dict(zip(_hrec.RP_SUMS, sums.tolist())))["auc"])
