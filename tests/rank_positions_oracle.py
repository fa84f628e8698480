"""A numpy oracle of hrec_rank_positions' contract (include/hrec.h): the 0-based
position of every label among a row's live candidates in the list order, and
the row's AUC, reciprocal rank and percentile-rank sums, one row at a time.
Nothing here calls the package.

A row is (pred: its score row over the candidates, f64 or f32; label_cols: the
candidate column of each label entry, any order, duplicates allowed, -1 for an
item outside the candidates; weights aligned with them or None; excluded: the
row's excluded columns or None).
"""
import math

import numpy as np

from user_metrics_oracle import ranking

SUMS = ("sum_auc", "sum_reciprocal_rank", "sum_w_pr", "sum_w", "n_auc", "n_reciprocal_rank", "n_w_pr", "n_w",
        "ranked", "unranked")


def row_positions(pred, label_cols, weights=None, excluded=None):
    """(rank int64 per label entry (-1: unranked), values (auc, reciprocal_rank, sum_w_pr, sum_w),
    counts (live, ranked, unranked))."""
    pred = np.asarray(pred)
    n = pred.size
    cols = np.asarray(label_cols, dtype=np.int64).reshape(-1)
    gone = np.zeros(n, bool)
    if excluded is not None:
        ex = np.asarray(excluded, dtype=np.int64).reshape(-1)
        gone[ex[(ex >= 0) & (ex < n)]] = True
    order = ranking(pred)           # stable descending, NaN last
    order = order[~gone[order]]     # the list without the excluded columns
    live = int(order.size)
    pos = np.full(n, -1, np.int64)
    pos[order] = np.arange(live)
    ok = (cols >= 0) & (cols < n)
    rank = np.full(cols.size, -1, np.int64)
    rank[ok] = pos[cols[ok]]
    is_ranked = rank >= 0
    ranked = int(is_ranked.sum())
    w = np.ones(cols.size) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    sum_w_pr, sum_w = np.float64(0.0), np.float64(0.0)
    for r, wt in zip(rank[is_ranked], w[is_ranked]):  # CSR order
        pr = np.float64(0.0) if live == 1 else np.float64(int(r)) / np.float64(live - 1)
        sum_w_pr = sum_w_pr + wt * pr
        sum_w = sum_w + wt
    distinct = np.unique(rank[is_ranked])  # distinct columns have distinct ranks
    h, s = int(distinct.size), int(distinct.sum())
    auc = rr = math.nan
    if h > 0:
        rr = float(np.float64(1.0) / np.float64(1 + int(distinct.min())))
        if live != h:
            auc = float(np.float64(1.0) - np.float64(s - h * (h - 1) // 2) / (np.float64(h) * np.float64(live - h)))
    return rank, (auc, rr, float(sum_w_pr), float(sum_w)), (live, ranked, int(cols.size) - ranked)


def batch_positions(scores, label_rows, indptr, cols, weights=None, excl=None):
    """Every row of a call: (rank int64 aligned with cols (entries of CSR rows no row reads: -1),
    row f64 [n_rows, 4], row_n int64 [n_rows, 3], sums {name: value}). excl: (excl_rows, excl_indptr,
    excl_cols) or None."""
    scores = np.asarray(scores)
    n_rows = scores.shape[0]
    cols = np.asarray(cols, dtype=np.int64)
    rank = np.full(cols.size, -1, np.int64)
    row = np.zeros((n_rows, 4))
    row_n = np.zeros((n_rows, 3), np.int64)
    for r in range(n_rows):
        q = -1 if label_rows is None else int(label_rows[r])
        lo, hi = (0, 0) if q < 0 else (int(indptr[q]), int(indptr[q + 1]))
        ex = None
        if excl is not None and int(excl[0][r]) >= 0:
            x = int(excl[0][r])
            ex = np.asarray(excl[2])[int(excl[1][x]): int(excl[1][x + 1])]
        rk, vals, cnt = row_positions(scores[r], cols[lo:hi], None if weights is None else weights[lo:hi], ex)
        rank[lo:hi] = rk
        row[r], row_n[r] = vals, cnt
    has = row_n[:, 1] > 0
    sums = {
        "sum_auc": float(np.nansum(row[:, 0])), "sum_reciprocal_rank": float(np.nansum(row[:, 1])),
        "sum_w_pr": float(row[has, 2].sum()), "sum_w": float(row[has, 3].sum()),
        "n_auc": float((~np.isnan(row[:, 0])).sum()), "n_reciprocal_rank": float((~np.isnan(row[:, 1])).sum()),
        "n_w_pr": float(has.sum()), "n_w": float(has.sum()),
        "ranked": float(row_n[:, 1].sum()), "unranked": float(row_n[:, 2].sum()),
    }
    return rank, row, row_n, sums


def metrics(sums):
    """The driver's means from the sums (NaN when nothing is ranked)."""
    nan = math.nan
    return {
        "meanPercentileRank": sums["sum_w_pr"] / sums["sum_w"] if sums["ranked"] > 0 and sums["sum_w"] > 0 else nan,
        "auc": sums["sum_auc"] / sums["n_auc"] if sums["n_auc"] > 0 else nan,
        "meanReciprocalRank": (sums["sum_reciprocal_rank"] / sums["n_reciprocal_rank"]
                               if sums["n_reciprocal_rank"] > 0 else nan),
    }
