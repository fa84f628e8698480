"""CPU: the numpy oracle of hrec_rank_positions (tests/rank_positions_oracle.py)
on cases worked by hand."""
import math

import numpy as np

import rank_positions_oracle as rpo


def test_two_positives_among_four():
    # the list is columns 2, 0, 3, 1; the labels stand at positions 0 and 2
    pred = np.array([0.5, 0.1, 0.9, 0.3])
    rank, (auc, rr, swpr, sw), (live, ranked, unranked) = rpo.row_positions(pred, [3, 2])
    assert rank.tolist() == [2, 0]
    assert (live, ranked, unranked) == (4, 2, 0)
    # pairs (positive, negative): (2,0) (2,1) (3,1) in order, (3,0) not: 3 of 4
    assert auc == 0.75 and rr == 1.0
    assert sw == 2.0 and swpr == 2.0 / 3.0 + 0.0


def test_tie_broken_by_column_and_weights():
    pred = np.array([1.0, 2.0, 2.0, 2.0], dtype=np.float32)
    rank, (auc, rr, swpr, sw), _ = rpo.row_positions(pred, [3, 1, 0], weights=[2.0, 0.5, 1.0])
    assert rank.tolist() == [2, 0, 3]  # equal values: the smaller column first
    assert rr == 1.0
    assert auc == 1.0 - (5 - 3) / (3.0 * 1.0)  # S = 5, h = 3, L = 4
    assert sw == 3.5 and swpr == (2.0 * (2.0 / 3.0) + 0.5 * 0.0) + 1.0 * 1.0


def test_nan_last_and_signed_zero_and_infinities():
    pred = np.array([math.nan, -0.0, 0.0, -math.inf, math.inf, math.nan])
    rank, _, (live, _, _) = rpo.row_positions(pred, [0, 1, 2, 3, 4, 5])
    # +inf, then -0.0 and 0.0 (equal: by column), -inf, the NaNs by column
    assert rank.tolist() == [4, 1, 2, 3, 0, 5] and live == 6


def test_excluded_label_and_missing_label_are_unranked():
    pred = np.array([4.0, 3.0, 2.0, 1.0])
    rank, (auc, rr, swpr, sw), cnt = rpo.row_positions(pred, [1, -1, 2, 7], excluded=[0, 1, 1, 9])
    assert rank.tolist() == [-1, -1, 0, -1]  # column 2 leads the list without 0 and 1
    assert cnt == (2, 1, 3)
    assert auc == 1.0 and rr == 1.0 and swpr == 0.0 and sw == 1.0


def test_duplicates_are_answered_and_collapse():
    pred = np.array([4.0, 3.0, 2.0, 1.0])
    rank, (auc, rr, swpr, sw), cnt = rpo.row_positions(pred, [2, 2, 0])
    assert rank.tolist() == [2, 2, 0] and cnt == (4, 3, 0)
    assert auc == 1.0 - (2 - 1) / (2.0 * 2.0)  # h = 2, S = 2
    assert sw == 3.0 and swpr == (2.0 / 3.0 + 2.0 / 3.0) + 0.0


def test_every_live_column_is_a_label():
    pred = np.array([1.0, 2.0, 3.0])
    _, (auc, rr, _, _), cnt = rpo.row_positions(pred, [0, 1], excluded=[2])
    assert math.isnan(auc) and rr == 1.0 and cnt == (2, 2, 0)


def test_one_live_column():
    _, (auc, rr, swpr, sw), cnt = rpo.row_positions(np.array([0.25]), [0])
    assert math.isnan(auc) and rr == 1.0 and swpr == 0.0 and sw == 1.0 and cnt == (1, 1, 0)
    rank, (auc, rr, swpr, sw), cnt = rpo.row_positions(np.array([3.0, 1.0]), [1], excluded=[0])
    assert rank.tolist() == [0] and swpr == 0.0 and cnt == (1, 1, 0)


def test_no_labels_and_batch_sums():
    scores = np.array([[0.5, 0.1, 0.9, 0.3], [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0]])
    indptr = np.array([0, 2, 3])
    cols = np.array([3, 2, 0])
    rank, row, row_n, sums = rpo.batch_positions(scores, [0, -1, 1], indptr, cols)
    assert rank.tolist() == [2, 0, 0]
    assert math.isnan(row[1, 0]) and math.isnan(row[1, 1]) and row[1, 2] == row[1, 3] == 0.0
    assert row_n.tolist() == [[4, 2, 0], [4, 0, 0], [4, 1, 0]]
    assert sums["n_auc"] == 2.0 and sums["sum_auc"] == 0.75 + 1.0
    assert sums["ranked"] == 3.0 and sums["unranked"] == 0.0 and sums["n_w"] == 2.0
    m = rpo.metrics(sums)
    assert m["auc"] == 0.875 and m["meanReciprocalRank"] == 1.0
    assert m["meanPercentileRank"] == (2.0 / 3.0) / 3.0
    assert all(math.isnan(v) for v in rpo.metrics(dict.fromkeys(rpo.SUMS, 0.0)).values())
