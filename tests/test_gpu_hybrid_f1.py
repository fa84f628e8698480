"""GPU: hrec_hybrid_model_f1 (through _hrec.hybrid_model_f1) against the oracle
of its contract (tests/hybrid_f1_oracle.py): out_top ids, the f64 bits of
out_f1 (NaN compared as NaN), out_wins and the overflow flag, in both modes;
and hrec_hybrid_lists_rowwise against hrec_hybrid_lists (constant row_wins,
bit for bit up to each row's length) and against hybrid_lists_oracle.lists
applied row by row (mixed row_wins).

All comparisons are exact. In mode 0 the flag must equal the oracle's
predicate (list_overflows: a model's sample bound admits more columns than
HYBRID_LISTS_CAP); only the overflow case is built to raise it."""
import numpy as np
import pytest
import torch
from hybrid_f1_oracle import keys, list_overflows, model_f1, orders
from hybrid_lists_oracle import lists
from test_gpu_hybrid_lists import _csr, _dev_mat, _excl_dev, _same_values

pytestmark = pytest.mark.gpu

N_ROWS = (1, 3, 70)
NS = (1, 7, 64, 65, 1000, 4096, 4097, 9000)
KS = (1, 5, 10, 64, 1024)


def _consts():
    from src import _hrec

    return _hrec.HYBRID_LISTS_SAMPLE, _hrec.HYBRID_LISTS_CAP


def _label_inputs(sets, totals, rng):
    """(label_rows, label_indptr, label_cols, label_total) of per-row column
    lists (None: label_rows = -1) and per-row totals, the CSR rows shuffled."""
    rows, indptr, cols = _csr([None if s is None else sorted(set(s)) for s in sets], rng)
    total = np.zeros(len(indptr) - 1, np.int32)
    for r, q in enumerate(rows):
        if q >= 0:
            total[q] = totals[r]
    return rows, indptr, cols, total


def _labels_for(full, n, rng):
    """Rows cycle through six kinds: labels from the ALS side's own top,
    from the two-tower side's own top, random ones with a larger total, no
    label row, label_total 0, and labels none of which is a candidate."""
    sets, totals = [], []
    for r in range(full.shape[0]):
        kind = r % 6
        if kind == 0:
            s = full[r, 0, :3].tolist()
            sets.append(s), totals.append(len(set(s)))
        elif kind == 1:
            s = full[r, 1, :4].tolist() + rng.integers(0, n, 2).tolist()
            sets.append(s), totals.append(len(set(s)) + 1)
        elif kind == 2:
            s = rng.integers(0, n, 12).tolist() + full[r, 0, :1].tolist()
            sets.append(s), totals.append(len(set(s)) + 7)
        elif kind == 3:
            sets.append(None), totals.append(0)
        elif kind == 4:
            sets.append(rng.integers(0, n, 3).tolist()), totals.append(0)
        else:
            sets.append([]), totals.append(5)
    return _label_inputs(sets, totals, rng)


def _run(dev, als, tt, k, labels, default_wins, fb=None, mode=0, pad=False):
    from src import _hrec

    return _hrec.hybrid_model_f1(_dev_mat(als, pad, dev, float("nan")), _dev_mat(tt, pad, dev, 3e38), k,
                                 labels=tuple(torch.as_tensor(x, device=dev) for x in labels),
                                 default_wins=default_wins,
                                 fallback=None if fb is None else torch.as_tensor(fb, device=dev), mode=mode,
                                 want_top=True)


def _check(res, exp, msg):
    f1, wins, over, top = (x.cpu().numpy() for x in res)
    e_f1, e_wins, e_top = exp
    assert top.shape == e_top.shape, msg
    np.testing.assert_array_equal(top, e_top, err_msg=msg)
    _same_values(f1, e_f1, msg)
    np.testing.assert_array_equal(wins, e_wins, err_msg=msg)
    return int(over[0])


def _cut(kmat, kk):
    sample, cap = _consts()
    return any(list_overflows(kmat[r, m], kk, sample, cap) for r in range(kmat.shape[0]) for m in range(2))


def _inputs(rng, n_rows, n):
    """n_rows 1: plain; 3: a cold ALS row and unknown items, with the f64
    fallback, ld > n, default_wins 1; 70: scores quantised to 8 levels (ties
    decide the selection) with NaN entries and no fallback, ld > n."""
    als = rng.normal(size=(n_rows, n)).astype(np.float32)
    tt = rng.normal(size=(n_rows, n)).astype(np.float32)
    fb, pad, dw = None, False, 0
    if n_rows == 3:
        fb = rng.random(n) * 5 + 1 / 3  # f64 values that are not f32-representable
        als[0] = np.nan
        als[1, rng.random(n) < 0.2] = np.nan
        pad, dw = True, 1
    elif n_rows == 70:
        als = rng.integers(0, 8, (n_rows, n)).astype(np.float32) / 3
        tt = rng.integers(0, 8, (n_rows, n)).astype(np.float32) / 7
        als[rng.random((n_rows, n)) < 0.02] = np.nan
        tt[5, rng.random(n) < 0.5] = np.nan
        pad = True
    return als, tt, fb, pad, dw


@pytest.mark.parametrize("n", NS)
def test_shapes(device, n):
    rng = np.random.default_rng(1000 + n)
    for n_rows in N_ROWS:
        als, tt, fb, pad, dw = _inputs(rng, n_rows, n)
        full, kmat = orders(als, tt, fb), keys(als, tt, fb)
        labels = _labels_for(full, n, rng)
        for k in KS:
            exp = model_f1(als, tt, k, labels, dw, fb, full=full)
            msg = f"n_rows {n_rows} n {n} k {k}"
            assert not _cut(kmat, min(k, n)), msg  # the inputs are not meant to overflow
            for mode in (0, 1):
                assert _check(_run(device, als, tt, k, labels, dw, fb, mode, pad), exp, f"{msg} mode {mode}") == 0
            if n_rows == 70 and n >= 1000 and k in (5, 10):  # both choices, the default and both F1 = 0 occur
                f1, wins, _ = exp
                assert set(wins[0::6]) == {1} and set(wins[1::6]) == {0} and np.isnan(f1[3::6]).all()
                assert np.isnan(f1[4::6]).all() and (f1[5::6] == 0).all() and (f1[2::6, 0] > 0).all()


@pytest.mark.parametrize("with_fb", [True, False])
@pytest.mark.parametrize("default_wins", [0, 1])
def test_nans_ties_and_default(device, with_fb, default_wins):
    """ALS NaNs with and without a fallback next to quantised scores; both
    default_wins; ld > n; n just past the sample."""
    sample, _ = _consts()
    n = sample + 1
    rng = np.random.default_rng(31 + with_fb)
    als = (rng.integers(0, 8, (12, n)) / 3).astype(np.float32)
    tt = (rng.integers(0, 8, (12, n)) / 7).astype(np.float32)
    als[0] = np.nan
    als[1, rng.random(n) < 0.3] = np.nan
    als[2, : sample] = np.nan                 # the whole sample is NaN on the ALS side
    tt[3, 30:] = np.nan                       # 30 numbers: the bound of k = 1024 is NaN
    tt[4, rng.random(n) < 0.9] = np.nan
    fb = (rng.integers(0, 8, n) / 5 + 1e-9) if with_fb else None
    full, kmat = orders(als, tt, fb), keys(als, tt, fb)
    labels = _labels_for(full, n, rng)
    cuts = []
    for k in (1, 10, 1024):
        exp = model_f1(als, tt, k, labels, default_wins, fb, full=full)
        cut = _cut(kmat, k)  # a NaN bound (fewer than k numbers in the sample) admits all n > CAP columns
        cuts.append(cut)
        assert _check(_run(device, als, tt, k, labels, default_wins, fb, 1, True), exp, f"k {k} mode 1") == 0
        res = _run(device, als, tt, k, labels, default_wins, fb, 0, True)
        if cut:
            assert int(res[2].item()) == 1
        else:
            assert _check(res, exp, f"k {k} mode 0") == 0
        assert set(exp[1][3::6]) == {default_wins} and set(exp[1][4::6]) == {default_wins}
    assert cuts == [not with_fb, not with_fb, True]


def test_overflow(device):
    """n = 9000 with each model's scores ascending by column: the sample
    holds the worst columns, so more than CAP reach its bound. Mode 0 raises
    the flag; mode 1 equals the oracle."""
    sample, cap = _consts()
    n = 9000
    rng = np.random.default_rng(41)
    als = np.tile(np.arange(n, dtype=np.float32), (3, 1))
    tt = np.tile(np.arange(n, dtype=np.float32) / 2, (3, 1))
    full, kmat = orders(als, tt), keys(als, tt)
    labels = _labels_for(full, n, rng)
    for k in (10, 1024):
        assert n - sample + k > cap and _cut(kmat, k)
        exp = model_f1(als, tt, k, labels, 0, full=full)
        assert exp[2][0, 0, 0] == n - 1
        res = _run(device, als, tt, k, labels, 0, mode=0)
        assert int(res[2].item()) == 1
        assert _check(_run(device, als, tt, k, labels, 0, mode=1), exp, f"k {k} mode 1") == 0
    # one model alone overflowing raises the flag too
    tt2 = rng.normal(size=(3, n)).astype(np.float32)
    assert _cut(keys(als, tt2), 10) and not _cut(keys(tt2, tt2), 10)
    assert int(_run(device, als, tt2, 10, labels, 0, mode=0)[2].item()) == 1
    assert int(_run(device, tt2, als, 10, labels, 0, mode=0)[2].item()) == 1
    assert int(_run(device, tt2, tt2, 10, labels, 0, mode=0)[2].item()) == 0


def test_no_labels_at_all(device):
    from src import _hrec

    rng = np.random.default_rng(43)
    als = torch.as_tensor(rng.normal(size=(5, 300)).astype(np.float32), device=device)
    tt = torch.as_tensor(rng.normal(size=(5, 300)).astype(np.float32), device=device)
    for dw in (0, 1):
        f1, wins, over = _hrec.hybrid_model_f1(als, tt, 10, labels=None, default_wins=dw)
        assert torch.isnan(f1).all() and wins.tolist() == [dw] * 5 and int(over.item()) == 0


# ------------------------------------------------------------ rowwise lists
def _lists_inputs(rng, n_rows, n):
    als = rng.normal(size=(n_rows, n)).astype(np.float32)
    tt = rng.normal(size=(n_rows, n)).astype(np.float32)
    als[0, rng.random(n) < 0.1] = np.nan
    fb = rng.random(n) * 5 + 1 / 3
    excl = _csr([None if r % 5 == 4 else np.flatnonzero(rng.random(n) < (0.1 if r % 5 else 0.999)).tolist()
                 for r in range(n_rows)], rng)
    return als, tt, fb, excl


def _call(dev, entry, als, tt, top_k, wins, fb, excl, mode):
    return entry(_dev_mat(als, True, dev, float("nan")), _dev_mat(tt, True, dev, 3e38), top_k, wins,
                 fallback=torch.as_tensor(fb, device=dev), excl=_excl_dev(excl, dev), mode=mode, want_minmax=True)


@pytest.mark.parametrize("n", [65, 4097 + 900])
def test_rowwise_constant_equals_hybrid_lists(device, n):
    from src import _hrec

    rng = np.random.default_rng(51 + n)
    n_rows = 11
    als, tt, fb, excl = _lists_inputs(rng, n_rows, n)
    for const in (0, 1):
        wins = torch.full((n_rows,), const * 7, dtype=torch.int32, device=device)  # any non-zero value means ALS wins
        for with_excl in (excl, None):
            for mode in (0, 1):
                for top_k in (10, 1024):
                    a = _call(device, _hrec.hybrid_lists, als, tt, top_k, bool(const), fb, with_excl, mode)
                    b = _call(device, _hrec.hybrid_lists_rowwise, als, tt, top_k, wins, fb, with_excl, mode)
                    msg = f"wins {const} excl {with_excl is not None} mode {mode} top_k {top_k}"
                    for x, y in zip(a[2:], b[2:]):  # lens, overflow, minmax
                        assert torch.equal(x, y), msg
                    assert int(a[3].item()) == 0, msg
                    live = torch.arange(a[0].shape[1], device=device).unsqueeze(0) < a[2].unsqueeze(1)
                    assert torch.equal(a[0][live], b[0][live]), msg
                    assert torch.equal(a[1].view(torch.int64)[live], b[1].view(torch.int64)[live]), msg


@pytest.mark.parametrize("n", [65, 4097 + 900])
def test_rowwise_mixed_equals_oracle_rows(device, n):
    from src import _hrec

    rng = np.random.default_rng(61 + n)
    n_rows = 11
    als, tt, fb, excl = _lists_inputs(rng, n_rows, n)
    wins = rng.integers(0, 2, n_rows).astype(np.int32)
    assert 0 < wins.sum() < n_rows
    for with_excl in (excl, None):
        for top_k in (10, 1024):
            exp = [lists(als[r: r + 1], tt[r: r + 1], top_k, bool(wins[r]), fb,
                         None if with_excl is None else (with_excl[0][r: r + 1], *with_excl[1:]))
                   for r in range(n_rows)]
            for mode in (0, 1):
                idx, val, lens, over, mm = (x.cpu().numpy() for x in _call(
                    device, _hrec.hybrid_lists_rowwise, als, tt, top_k, torch.as_tensor(wins, device=device), fb,
                    with_excl, mode))
                assert int(over[0]) == 0
                for r, (rows, e_len, e_mm) in enumerate(exp):
                    msg = f"row {r} excl {with_excl is not None} top_k {top_k} mode {mode}"
                    L = int(e_len[0])
                    assert lens[r] == L, msg
                    np.testing.assert_array_equal(idx[r, :L], rows[0][0][:L], err_msg=msg)
                    _same_values(val[r, :L], rows[0][1][:L], msg)
                    np.testing.assert_array_equal(mm[r], e_mm[0], err_msg=msg)
