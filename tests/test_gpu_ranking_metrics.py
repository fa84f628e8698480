"""GPU: hrec_ranking_metrics (Spark's RankingMetrics over ranked id lists on
the device) against the plain-Python oracle of tests/ranking_oracle.py.

Per-row values are compared bit for bit (uint64 views): each is one IEEE
division of integers, or of sums added in ascending position from the gain
table the wrapper makes on the host (_hrec.rank_tables, handed to the oracle
too). The three counts are exact. Each of the five sums is within rtol 1e-12
of math.fsum over the oracle's per-row values: a sum of n <= 4097 non-negative
f64 terms in any order carries at most n 2^-53 = 4.5e-13 relative error.

Cases: label rows of 0, 1, 63, 64, 65 and 1500 entries (in turn), drawn with
duplicates from a range of about 0.7 of their length; lists drawn without
replacement from a range twice their length, so hits are common."""
import math

import numpy as np
import pytest
import torch
from ranking_oracle import mean_metrics, row_metrics

pytestmark = pytest.mark.gpu

LABEL_SIZES = (0, 1, 63, 64, 65, 1500)
# raw ids that are no array index: the extremes, both sides of +-2^31 and of 2^32
SPECIAL = np.array([-2 ** 63, -2 ** 40, -2 ** 32 - 1, -2 ** 31 - 1, -2 ** 31, -1, 0, 1, 2 ** 31 - 1, 2 ** 31,
                    2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40, 2 ** 63 - 1], dtype=np.int64)


def _hrec():
    from src import _hrec

    return _hrec


def _case(seed, n_rows, len_max, with_len=False, ld=None, id_map=None):
    """(pred [n_rows, ld], pred_len or None, indptr, labels) on the host."""
    rng = np.random.default_rng(seed)
    ld = len_max if ld is None else ld
    rows, pred = [], np.zeros((n_rows, ld), np.int64)
    pred_len = np.full(n_rows, len_max, np.int32)
    for r in range(n_rows):
        s = LABEL_SIZES[(r + seed) % len(LABEL_SIZES)]
        lab = np.sort(rng.integers(0, max(3, int(0.7 * s) + 1), s)).astype(np.int64)
        pool = max(2 * len_max, 8) if id_map is None else len(id_map)
        lst = np.resize(rng.permutation(pool), ld).astype(np.int64)
        if id_map is not None:
            lab, lst = id_map[lab % len(id_map)], id_map[lst]
            lab.sort()
        if with_len:
            pred_len[r] = 0 if r % 5 == 1 else rng.integers(0, len_max + 1)
            if s:  # the slots past the list hold the row's own labels: they must not count
                lst[pred_len[r]:] = np.resize(lab, ld - pred_len[r])
        pred[r] = lst
        rows.append(lab)
    indptr = np.zeros(n_rows + 1, np.int64)
    indptr[1:] = np.cumsum([len(x) for x in rows])
    labels = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return pred, (pred_len if with_len else None), indptr, labels


def _run(device, pred, pred_len, indptr, labels, k, len_max):
    h = _hrec()
    t = lambda a: None if a is None else torch.as_tensor(a, device=device)  # noqa: E731
    out = [h.ranking_metrics(t(pred), t(indptr), t(labels), k, pred_len=t(pred_len), pred_len_max=len_max,
                             want_per_row=True) for _ in range(2)]
    torch.cuda.synchronize()
    (sums, unsorted, per_row), (sums2, unsorted2, per_row2) = out
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)), "two calls must give the same bits"
    assert torch.equal(per_row.view(torch.int64), per_row2.view(torch.int64)) and torch.equal(unsorted, unsorted2)
    return dict(zip(h.RANK_SUMS, sums.tolist())), int(unsorted.item()), per_row.cpu().numpy()


def _check(device, pred, pred_len, indptr, labels, k, len_max):
    gain = _hrec().rank_tables(k)[0]
    n_rows = len(indptr) - 1
    exp, hits, empty = [], 0, 0
    for r in range(n_rows):
        lab = labels[indptr[r]: indptr[r + 1]]
        lst = pred[r, : (len_max if pred_len is None else pred_len[r])]
        exp.append(row_metrics(lst, lab, k, gain))
        members = set(lab.tolist())
        hits += sum(1 for x in lst[:k].tolist() if x in members)
        empty += len(lab) == 0
    exp = np.array(exp, np.float64).reshape(n_rows, 5)
    got, unsorted, per_row = _run(device, pred, pred_len, indptr, labels, k, len_max)
    print("sums:", got, "expected column sums:", [math.fsum(exp[:, j]) for j in range(5)])
    assert unsorted == 0
    assert per_row.shape == exp.shape and np.array_equal(per_row.view(np.uint64), exp.view(np.uint64))
    assert got["n_rows"] == n_rows and got["n_empty"] == empty and got["hits"] == hits
    for j, name in enumerate(("sum_precision", "sum_recall", "sum_ap", "sum_ap_k", "sum_ndcg")):
        np.testing.assert_allclose(got[name], math.fsum(exp[:, j]), rtol=1e-12, atol=0)
    return exp


@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 257, 4097])
def test_row_counts(device, n_rows, with_len):
    pred, pred_len, indptr, labels = _case(n_rows, n_rows, 10, with_len)
    exp = _check(device, pred, pred_len, indptr, labels, 10, 10)
    if n_rows >= 257 and not with_len:
        assert (exp[:, 0] > 0).sum() > n_rows // 2, "hits must be common"


def _ks(len_max):
    return sorted({1, max(1, len_max // 2), len_max, min(1024, len_max + 7), 1024})


@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("len_max,k", [(n, k) for n in (1, 10, 64, 65, 1024) for k in _ks(n)])
def test_list_lengths_and_cuts(device, len_max, k, with_len):
    pred, pred_len, indptr, labels = _case(100 + len_max, 37, len_max, with_len, ld=len_max + (3 if with_len else 0))
    _check(device, pred, pred_len, indptr, labels, k, len_max)


@pytest.mark.parametrize("with_len", [False, True])
def test_ids_are_raw_keys(device, with_len):
    """-1, the int64 extremes, +-2^31 and values beyond 2^32 are ids like any other."""
    pred, pred_len, indptr, labels = _case(7, 30, 12, with_len, id_map=SPECIAL)
    assert {-1, -2 ** 31, 2 ** 31, 2 ** 32 + 5} <= set(pred.ravel().tolist())
    exp = _check(device, pred, pred_len, indptr, labels, 12, 12)
    assert (exp[:, 1] > 0).any()


def test_no_rows_gives_zeros(device):
    got, unsorted, per_row = _run(device, np.zeros((0, 4), np.int64), None, np.zeros(1, np.int64),
                                  np.zeros(0, np.int64), 3, 4)
    assert unsorted == 0 and per_row.shape == (0, 5) and all(v == 0.0 for v in got.values())


def test_rows_without_labels_and_without_lists(device):
    """Every label row empty (no label entry at all), and lists of length 0."""
    pred = np.arange(12, dtype=np.int64).reshape(3, 4)
    got, unsorted, per_row = _run(device, pred, None, np.zeros(4, np.int64), np.zeros(0, np.int64), 2, 4)
    assert unsorted == 0 and got["n_rows"] == 3 and got["n_empty"] == 3 and not per_row.any()
    _check(device, pred, np.zeros(3, np.int32), np.array([0, 2, 2, 5]), np.array([0, 1, 4, 8, 9]), 2, 4)


@pytest.mark.parametrize("row_len", [2, 65, 1500])
def test_a_descending_label_row_is_reported(device, row_len):
    pred, _, indptr, labels = _case(3, 8, 10)
    rows = [labels[indptr[r]: indptr[r + 1]] for r in range(8)]
    bad = np.arange(row_len, dtype=np.int64)
    bad[[-2, -1]] = bad[[-1, -2]]  # one descending neighbour pair, in the last row
    rows.append(bad)
    indptr = np.r_[0, np.cumsum([len(x) for x in rows])].astype(np.int64)
    pred = np.vstack([pred, pred[:1]])
    _, unsorted, _ = _run(device, pred, None, indptr, np.concatenate(rows), 10, 10)
    assert unsorted == 1
    rows[-1] = np.sort(bad)
    _, unsorted, _ = _run(device, pred, None, indptr, np.concatenate(rows), 10, 10)
    assert unsorted == 0


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 10, 15])
def test_spark_suite_example(device, k):
    lists = [[1, 6, 2, 7, 8, 3, 9, 10, 4, 5], [4, 1, 5, 6, 2, 7, 3, 8, 9, 10], [1, 2, 3, 4, 5]]
    labs = [[1, 2, 3, 4, 5], [1, 2, 3], []]
    pred = np.zeros((3, 10), np.int64)
    for r, lst in enumerate(lists):
        pred[r, : len(lst)] = lst
    indptr, labels = np.array([0, 5, 8, 8]), np.array(labs[0] + labs[1], np.int64)
    exp = _check(device, pred, np.array([10, 10, 5], np.int32), indptr, labels, k, 10)
    # the wrapper's numpy gain table against the oracle's math.log one: the same to the last bits
    np.testing.assert_allclose(exp.mean(axis=0), mean_metrics(lists, labs, k), rtol=1e-14, atol=0)
    table = {1: (1 / 3, 1 / 15), 2: (1 / 3, 8 / 45), 3: (1 / 3, 11 / 45), 4: (0.25, 11 / 45), 5: (4 / 15, 16 / 45),
             10: (4 / 15, 2 / 3), 15: (8 / 45, 2 / 3)}
    got, _, _ = _run(device, pred, np.array([10, 10, 5], np.int32), indptr, labels, k, 10)
    assert got["sum_precision"] / 3 == pytest.approx(table[k][0], rel=0, abs=1e-15)
    assert got["sum_recall"] / 3 == pytest.approx(table[k][1], rel=0, abs=1e-15)
    assert got["sum_ap"] / 3 == pytest.approx(0.355026, rel=0, abs=1e-5)
    if k == 10:
        assert got["sum_ndcg"] / 3 == pytest.approx(0.487913, rel=0, abs=1e-5)
