"""A numpy oracle of hrec_user_metrics' contract (include/hrec.h): the
reference RecommenderEvaluator's per-user metrics, written from the contract's
arithmetic, one user at a time. Nothing here calls sklearn or the package.

A user is (ratings f64 in frame order, cols: the candidate column of each rated
item or -1, pred: the user's score row over the candidates, f64 or f32). The
f32 row follows the two-tower dtype rule (np.float32 dict values on the
per-user path); every other source is f64.
"""
import math

import numpy as np

NDCG_UNDEFINED = 1   # exactly one common item, or an infinite prediction among the common items
ERR_UNDEFINED = 2    # MAE / RMSE: a rescaled value is not finite
NO_COMMON = 4        # no rated item in the candidate frame: NDCG = MAE = RMSE = 0
NO_RELEVANT = 8      # nothing in the band: Recall = 0
NO_RATINGS = 16      # the row has no ratings at all: everything 0, counted nowhere
STATUS_BITS = 5
BAND = 0.1


def pairwise_sum(a):
    """numpy's pairwise summation of a contiguous f64 vector (what np.add.reduce runs)."""
    a = np.asarray(a, dtype=np.float64)
    n = a.size
    if n < 8:
        res = np.float64(0.0)
        for x in a:
            res = res + x
        return res
    if n <= 128:
        r = [np.float64(x) for x in a[:8]]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def threshold(ratings):
    """The bits of np.mean(list(actual.values()))."""
    r = np.asarray(ratings, dtype=np.float64)
    return pairwise_sum(r) / np.float64(r.size)


def ranking(pred):
    """Stable descending order of a score row: equal scores keep frame order, NaN last."""
    p = np.asarray(pred).astype(np.float64)
    nan = np.isnan(p)
    key = np.where(nan, 0.0, -p)
    return np.lexsort((np.arange(p.size), key, nan))


def discount_prefix(ndcg_k):
    """cs[j] = the first min(j, ndcg_k) discounts 1 / log2(i + 2) added in order (sklearn's
    np.cumsum of its discount vector, zeros past k): ndcg_k + 1 entries."""
    d = 1.0 / (np.log(np.arange(int(ndcg_k), dtype=np.float64) + 2.0) / np.log(2.0))
    return np.concatenate([np.zeros(1), np.cumsum(d)])


def _mm_range(r, eps):
    return type(r)(1.0) if r < 10 * eps else r


def _grades(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 2, (x >= 0.33).astype(np.int64) + (x >= 0.66).astype(np.int64))


def ndcg(t, p, ndcg_k, cs=None):
    """(value, undefined, (true grades, predicted grades)) over the common items."""
    m = len(t)
    if m == 0:
        return 0.0, False, None
    t = np.asarray(t, dtype=np.float64)
    f32 = np.asarray(p).dtype == np.float32
    if m == 1 or np.isinf(np.asarray(p, dtype=np.float64)).any():
        return math.nan, True, None
    cs = discount_prefix(ndcg_k) if cs is None else cs
    lo, hi = t.min(), t.max()
    scale = np.float64(1.0) / _mm_range(hi - lo, np.finfo(np.float64).eps)
    min_ = np.float64(0.0) - lo * scale
    tn = t * scale + min_
    if f32:
        pn = (np.asarray(p, np.float32).astype(np.float64) * scale).astype(np.float32)
        pn = (pn.astype(np.float64) + min_).astype(np.float32).astype(np.float64)
    else:
        pn = np.asarray(p, np.float64) * scale + min_
    gt, gp = _grades(tn), _grades(pn)

    def at(j):
        return cs[min(int(j), int(ndcg_k))]

    dcg, end = np.float64(0.0), 0
    for g in (2, 1, 0):
        sel = gp == g
        c = int(sel.sum())
        if c == 0:
            continue
        w = at(end + c) if end == 0 else at(end + c) - at(end)
        dcg = dcg + (np.float64(int(gt[sel].sum())) / np.float64(c)) * w
        end += c
    n2, n1 = int((gt == 2).sum()), int((gt == 1).sum())
    idcg = np.float64(2.0) * at(n2) + (at(n2 + n1) - at(n2))
    return (float(dcg / idcg) if idcg != 0 else 0.0), False, (gt, gp)


def mae_rmse(t, p):
    """(mae, rmse, undefined) over the common items."""
    m = len(t)
    if m == 0:
        return 0.0, 0.0, False
    t = np.asarray(t, dtype=np.float64)
    p = np.asarray(p)
    with np.errstate(all="ignore"):
        t5 = (np.float64(4.0) * (t - t.min())) / (t.max() - t.min()) + np.float64(1.0)
        if p.dtype == np.float32:
            lo, hi = np.nanmin(p) if not np.isnan(p).all() else np.float32(np.nan), \
                np.nanmax(p) if not np.isnan(p).all() else np.float32(np.nan)
            p5 = ((np.float32(4.0) * (p - lo)) / (hi - lo) + np.float32(1.0)).astype(np.float64)
        else:
            p = p.astype(np.float64)
            lo, hi = (np.nanmin(p), np.nanmax(p)) if not np.isnan(p).all() else (np.nan, np.nan)
            p5 = (np.float64(4.0) * (p - lo)) / (hi - lo) + np.float64(1.0)
    if not (np.isfinite(t5).all() and np.isfinite(p5).all()):
        return math.nan, math.nan, True
    d = t5 - p5
    return float(np.sum(np.abs(d)) / m), float(np.sqrt(np.sum(d * d) / m)), False


def user_metrics(ratings, cols, pred, k_values=(5, 10, 15, 20), ndcg_k=10, ranked=None):
    """One user's row: (values [2 * n_k + 3] = Precision per k, Recall per k, NDCG, MAE, RMSE; status).
    ranked: the user's list (candidate columns, best first); None: the oracle's own ranking of pred."""
    k_values = [int(k) for k in k_values]
    nk = len(k_values)
    ratings = np.asarray(ratings, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    out = np.zeros(2 * nk + 3)
    if ratings.size == 0:
        return out, NO_RATINGS | NO_COMMON | NO_RELEVANT
    thr = threshold(ratings)
    lo, hi = thr - BAND, thr + BAND
    rel = (lo <= ratings) & (ratings <= hi)
    n_rel = int(rel.sum())
    rel_cols = set(int(c) for c in cols[rel] if c >= 0)
    order = [int(c) for c in (ranking(pred) if ranked is None else ranked)]
    status = 0 if n_rel else NO_RELEVANT
    for i, k in enumerate(k_values):
        hits = sum(1 for c in order[:k] if c in rel_cols)
        out[i] = hits / k if k > 0 else 0.0
        out[nk + i] = hits / n_rel if n_rel else 0.0
    common = cols >= 0
    t = ratings[common]
    p = np.asarray(pred)[cols[common]]
    if t.size == 0:
        return out, status | NO_COMMON
    v, und, _ = ndcg(t, p, ndcg_k)
    out[2 * nk] = v
    status |= NDCG_UNDEFINED if und else 0
    mae, rmse, und = mae_rmse(t, p)
    out[2 * nk + 1], out[2 * nk + 2] = mae, rmse
    status |= ERR_UNDEFINED if und else 0
    return out, status


def from_dicts(actual, predicted):
    """(ratings, cols, pred row) of the per-user dicts (actual: {item: rating} in frame order,
    predicted: {item: score} in candidate-frame order); f32 when every score is np.float32."""
    items = list(predicted.keys())
    col = {it: j for j, it in enumerate(items)}
    vals = list(predicted.values())
    f32 = len(vals) > 0 and all(isinstance(v, np.float32) for v in vals)
    pred = np.array(vals, dtype=np.float32 if f32 else np.float64)
    ratings = np.array([float(r) for r in actual.values()], dtype=np.float64)
    cols = np.array([col.get(it, -1) for it in actual.keys()], dtype=np.int64)
    return ratings, cols, pred


def rtol(m):
    """The bound of the issue: summation order, divisions and the square root over m common items."""
    return 2.0 * (m + 8) * 2.0 ** -52
