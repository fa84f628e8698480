"""A numpy oracle for the list-quality measures, written from their
definitions and not from the device kernel's shortcut: cosines pair by pair in
f64, exposure by np.bincount, Gini from the sorted counts, personalization
from the overlap of every pair of lists. Shared by the CPU and the GPU tests.

Conventions (include/hrec.h, hrec_list_quality): a list entry is valid when
its position is below the row's length and its column is in [0, n); the same
for history columns; an item whose squared norm is 0 or not finite is a zero
vector (cosine 0 with everything)."""
import numpy as np

U53 = 2.0 ** -53


def inv_norms(vectors, d=None, dtype=np.float64):
    v = np.asarray(vectors)[:, :d].astype(dtype)
    with np.errstate(all="ignore"):
        s = (v * v).sum(axis=1)
        ok = np.isfinite(s) & (s > 0)
        return np.where(ok, 1.0 / np.sqrt(np.where(ok, s, 1.0)), 0.0).astype(dtype)


def unit_rows(vectors, d=None, dtype=np.float64):
    """x_j = v_j / |v_j| in `dtype`, the zero vector where the norm is unusable."""
    v = np.asarray(vectors)[:, :d].astype(dtype)
    inv = inv_norms(vectors, d, dtype)
    x = np.zeros_like(v)
    ok = inv != 0
    x[ok] = v[ok] * inv[ok][:, None]
    return x


def valid_entries(cols, n, length=None):
    cols = np.asarray(cols, np.int64).reshape(-1)
    if length is not None:
        cols = cols[: max(0, min(int(length), cols.size))]
    return cols[(cols >= 0) & (cols < n)]


def diversity_pairwise(x, cols):
    """1 - the mean cosine over the pairs of distinct entries; NaN below two."""
    m = len(cols)
    if m < 2:
        return float("nan")
    cos = x[cols] @ x[cols].T  # cos[a, b]: the cosine of the pair (a, b)
    return 1 - np.triu(cos, 1).sum() / (m * (m - 1) // 2)


def diversity_identity(x, cols):
    """The same through S.S - Q (the kernel's formula), in x's dtype."""
    m = len(cols)
    if m < 2:
        return float("nan")
    s = x[cols].sum(axis=0)
    q = (x[cols] * x[cols]).sum()
    return 1 - (np.dot(s, s) - q) / (m * (m - 1))


def unexpectedness_pairwise(x, cols, hist):
    m, g = len(cols), len(hist)
    if m == 0 or g == 0:
        return float("nan")
    cos = x[cols] @ x[hist].T  # cos[a, h]: list entry a against history entry h
    return 1 - cos.sum() / (m * g)


def per_row(lists, lens, vectors, d=None, history=None, tables=None):
    """(values f64 [n_rows, 2 + n_tab], counts int64 of the same shape,
    exposure int64 [n]). lists: [n_rows, L] columns; lens: None or one length
    per row; history: None or one column array (or None) per row; tables:
    None or [n_tab, n]."""
    lists = np.asarray(lists, np.int64)
    n = int(np.asarray(vectors).shape[0])
    x = unit_rows(vectors, d)
    tables = np.zeros((0, n)) if tables is None else np.asarray(tables, np.float64)
    n_rows, n_tab = lists.shape[0], tables.shape[0]
    vals = np.full((n_rows, 2 + n_tab), np.nan)
    cnt = np.zeros((n_rows, 2 + n_tab), np.int64)
    exposure = np.zeros(n, np.int64)
    for r in range(n_rows):
        cols = valid_entries(lists[r], n, None if lens is None else lens[r])
        hist = valid_entries(history[r], n) if history is not None and history[r] is not None else np.zeros(0, np.int64)
        exposure += np.bincount(cols, minlength=n)
        vals[r, 0] = diversity_pairwise(x, cols)
        vals[r, 1] = unexpectedness_pairwise(x, cols, hist)
        cnt[r, 0], cnt[r, 1] = len(cols), len(hist)
        for t in range(n_tab):
            tv = tables[t][cols]
            tv = tv[~np.isnan(tv)]
            cnt[r, 2 + t] = tv.size
            if tv.size:
                vals[r, 2 + t] = tv.mean()
    return vals, cnt, exposure


def column_sums(vals):
    """hrec_list_quality's sums: per column the sum over the rows where it is
    defined, then per column the count of those rows."""
    ok = ~np.isnan(vals)
    return np.concatenate([np.where(ok, vals, 0.0).sum(axis=0), ok.sum(axis=0).astype(np.float64)])


def catalog_coverage(exposure):
    return int((exposure > 0).sum()) / exposure.size


def distributional_coverage(exposure):
    """The entropy of the exposure distribution, in bits."""
    c = exposure[exposure > 0].astype(np.float64)
    if c.size == 0:
        return float("nan")
    p = c / c.sum()
    return float(-(p * np.log2(p)).sum())


def gini(exposure):
    c = np.sort(np.asarray(exposure, np.int64))
    n, total = c.size, int(c.sum())
    if total == 0:
        return float("nan")
    num = sum((2 * j - n - 1) * int(cj) for j, cj in enumerate(c, start=1))
    return num / (n * total)


def personalization(lists, lens, n, k):
    """1 - the mean over the pairs of lists (with an entry) of |A & B| / k."""
    lists = np.asarray(lists, np.int64)
    inc = np.zeros((lists.shape[0], n), np.int64)
    for r in range(lists.shape[0]):
        inc[r, valid_entries(lists[r], n, None if lens is None else lens[r])] = 1
    inc = inc[inc.sum(axis=1) > 0]
    u = inc.shape[0]
    if u < 2:
        return float("nan")
    common = inc @ inc.T
    overlap = int(np.triu(common, 1).sum())
    return 1.0 - overlap / (u * (u - 1) / 2 * k)


def history_tables(hist_users, hist_cols, n):
    """(novelty table, popularity table) f64 [n] from the distinct (user,
    candidate column) history pairs: log2(Hsum / h_i) (NaN where h_i = 0) and
    h_i / distinct users."""
    hist_users, hist_cols = np.asarray(hist_users, np.int64), np.asarray(hist_cols, np.int64)
    pairs = np.unique(np.stack([hist_users, hist_cols], 1), axis=0) if hist_users.size else np.zeros((0, 2), np.int64)
    h = np.bincount(pairs[:, 1], minlength=n).astype(np.float64)
    n_users = np.unique(hist_users).size
    with np.errstate(all="ignore"):
        nov = np.where(h > 0, np.log2(h.sum() / np.where(h > 0, h, 1.0)), np.nan)
    return nov, h / max(n_users, 1)


def summary(lists, lens, vectors, k, d=None, history=None, tables=None):
    """Every finished quantity of ranked_lists.list_quality from the
    definitions. tables: (novelty, popularity) or None."""
    n = int(np.asarray(vectors).shape[0])
    vals, cnt, exposure = per_row(lists, lens, vectors, d, history, None if tables is None else np.stack(tables))
    means = [float(np.nanmean(vals[:, c])) if (~np.isnan(vals[:, c])).any() else float("nan")
             for c in range(vals.shape[1])]
    users = int((cnt[:, 0] > 0).sum())
    res = {"catalogCoverage": catalog_coverage(exposure) if users else float("nan"),
           "distributionalCoverage": distributional_coverage(exposure),
           "gini": gini(exposure),
           "personalization": personalization(lists, lens, n, k),
           "intraListDiversity": means[0], "unexpectedness": means[1],
           "novelty": means[2] if tables is not None else float("nan"),
           "averagePopularity": means[3] if tables is not None else float("nan"),
           "count": users}
    if tables is not None:
        res["novelty_unseen"] = int((cnt[:, 0] - cnt[:, 2]).sum())
    else:
        res["novelty_unseen"] = 0
    return res, vals, cnt, exposure
