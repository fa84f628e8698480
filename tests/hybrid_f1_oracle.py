"""numpy / Python-float oracle of hrec_hybrid_model_f1's contract
(include/hrec.h): per row each model's own stable descending selection (ALS
keys after the cold-start substitution in f64, two-tower keys in f32, NaN
last, equal keys in column order) and compute_f1_score's arithmetic on Python
floats. Built on hybrid_lists_oracle.substitute / ranking. Test
infrastructure only."""
import numpy as np
from hybrid_lists_oracle import ranking, substitute


def selection(keys, k):
    """The first min(k, n) columns of the stable descending ranking."""
    keys = np.asarray(keys)
    return ranking(keys.astype(np.float64))[: min(int(k), keys.size)].astype(np.int64)  # f32 -> f64 keeps the order


def selections(als_row, tt_row, k, fallback=None):
    """(ALS selection, two-tower selection) of one row."""
    return selection(substitute(als_row, fallback), k), selection(np.asarray(tt_row, np.float32), k)


def f1_value(tp, k, total):
    """compute_f1_score's last three lines on Python numbers (total =
    len(actual_items); 0: recall 0, as there)."""
    precision = tp / k
    recall = tp / total if total else 0
    return 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0


def row_labels(labels, r):
    """(candidate label columns, total) of row r, or None for a row without
    labels (labels = (label_rows, label_indptr, label_cols, label_total) or
    None)."""
    if labels is None:
        return None
    rows, indptr, cols, total = labels
    q = int(rows[r])
    if q < 0 or int(total[q]) == 0:
        return None
    return np.asarray(cols[int(indptr[q]): int(indptr[q + 1])], np.int64), int(total[q])


def keys(als, tt, fallback=None):
    """f64 [n_rows, 2, n]: each model's ranking keys (the f32 two-tower
    scores widened: same order, ties and NaNs)."""
    als, tt = np.asarray(als, np.float32), np.asarray(tt, np.float32)
    return np.stack([np.stack([substitute(a, fallback), t.astype(np.float64)]) for a, t in zip(als, tt)])


def orders(als, tt, fallback=None):
    """int64 [n_rows, 2, n]: each model's full ranking of every row (a
    selection is its first min(k, n) entries), computed once per input."""
    return np.stack([np.stack([ranking(x) for x in row]) for row in keys(als, tt, fallback)]).astype(np.int64)


def list_overflows(key_row, kk, sample, cap):
    """Whether mode 0 cuts the list of one row of one model: with n > sample
    the bound is the kk-th best key of the first `sample` columns (NaN: below
    every number, equal to NaN); the columns reaching it must fit `cap`."""
    key_row = np.asarray(key_row, np.float64)
    if key_row.size <= sample:
        return False
    s = key_row[:sample]
    bound = s[ranking(s)[kk - 1]]
    if np.isnan(bound):
        return key_row.size > cap
    with np.errstate(invalid="ignore"):
        return int((key_row >= bound).sum()) > cap


def model_f1(als, tt, k, labels=None, default_wins=0, fallback=None, full=None):
    """(f1 f64 [n_rows, 2], wins int32 [n_rows], top int64 [n_rows, 2, min(k,
    n)]); full: orders(als, tt, fallback) when the caller has them."""
    als, tt = np.asarray(als, np.float32), np.asarray(tt, np.float32)
    n_rows, n = als.shape
    kk = min(int(k), n)
    f1 = np.full((n_rows, 2), np.nan, np.float64)
    wins = np.full(n_rows, 1 if default_wins else 0, np.int32)
    top = np.zeros((n_rows, 2, kk), np.int64)
    for r in range(n_rows):
        top[r, 0], top[r, 1] = selections(als[r], tt[r], k, fallback) if full is None else full[r, :, :kk]
        lab = row_labels(labels, r)
        if lab is None:
            continue
        cols, total = lab
        for m in range(2):
            f1[r, m] = float(f1_value(len(set(top[r, m].tolist()) & set(cols.tolist())), int(k), total))
        wins[r] = 1 if f1[r, 0] > f1[r, 1] else 0
    return f1, wins, top


def dict_f1(actual, pred, k, as_f32=False):
    """compute_f1_score(actual, pred, k) through the oracle: the dict's items
    are the candidate frame in dict order; as_f32: the scores are a two-tower
    row (np.float32 values), else an ALS row given as its f64 fallback."""
    ids = list(pred.keys())
    col = {item: j for j, item in enumerate(ids)}
    scores = np.array([pred[i] for i in ids], np.float32 if as_f32 else np.float64)
    keys = scores if as_f32 else substitute(np.full(len(ids), np.nan, np.float32), scores)
    sel = selection(keys, k)
    cols = {col[i] for i in actual if i in col}
    return f1_value(len(set(sel.tolist()) & cols), k, len(set(actual)))
