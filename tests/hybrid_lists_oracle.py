"""numpy oracle of hrec_hybrid_lists' contract (include/hrec.h): per row the
cold-start substitution, sklearn MinMaxScaler arithmetic (ALS side in f64,
two-tower side in f32, NaN ignored, over ALL columns), the f64 fusion with the
f32 norm widened before the multiply, the stable descending ranking with NaN
last, the deletion of the row's excluded columns and out_len. Test
infrastructure only."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def substitute(als_row, fallback=None):
    """a_rj: (double)als[r][j], or fallback[j] where als[r][j] is NaN."""
    a = np.asarray(als_row, np.float32)
    out = a.astype(np.float64)
    if fallback is not None:
        out = np.where(np.isnan(a), np.asarray(fallback, np.float64), out)
    return out


def extremes(x):
    """(min, max) with NaN ignored, in x's dtype. No number at all: the f64
    side keeps hrec_fuse_topk's starting values (+-DBL_MAX), the f32 side
    +-inf (which is what (float)DBL_MAX rounds to)."""
    vals = x[~np.isnan(x)]
    if x.dtype == np.float64:
        return (min(DBL_MAX, vals.min()) if vals.size else DBL_MAX,
                max(-DBL_MAX, vals.max()) if vals.size else -DBL_MAX)
    return (vals.min() if vals.size else np.float32(np.inf), vals.max() if vals.size else np.float32(-np.inf))


def scaler(lo, hi, dt):
    """MinMaxScaler's (scale_, min_) in dtype dt: a range below 10 eps scales by 1."""
    with np.errstate(all="ignore"):
        rng = dt(dt(hi) - dt(lo))
        if rng < dt(10) * np.finfo(dt).eps:
            rng = dt(1)
        scale = dt(dt(1) / rng)
        return scale, dt(dt(0) - dt(lo) * scale)


def fuse_row(a, t, als_wins):
    """(fused f64 [n], minmax f64 [4]) of a (f64, substituted) and t (f32)."""
    a, t = np.asarray(a, np.float64), np.asarray(t, np.float32)
    alo, ahi = extremes(a)
    tlo, thi = extremes(t)
    ascale, amin_ = scaler(alo, ahi, np.float64)
    tscale, tmin_ = scaler(tlo, thi, np.float32)
    w0, w1 = (0.8, 0.2) if als_wins else (0.2, 0.8)
    with np.errstate(all="ignore"):
        an = a * ascale + amin_
        tn = (t * tscale + tmin_).astype(np.float32)
        fused = w0 * an + w1 * tn.astype(np.float64)
    mm = np.array([alo, ahi, min(DBL_MAX, np.float64(tlo)), max(-DBL_MAX, np.float64(thi))], np.float64)
    return fused, mm


def ranking(fused):
    """Column indices, best first: descending, equal values in column order,
    NaN last in column order."""
    return np.argsort(-np.asarray(fused, np.float64), kind="stable")  # NaN sorts to the end, stably


def excluded_set(excl, r, n):
    """Row r's distinct in-range excluded columns (excl = (excl_rows,
    excl_indptr, excl_cols) or None)."""
    if excl is None:
        return np.zeros(0, np.int64)
    rows, indptr, cols = (np.asarray(x, np.int64) for x in excl)
    q = int(rows[r])
    if q < 0:
        return np.zeros(0, np.int64)
    c = cols[indptr[q]: indptr[q + 1]]
    return np.unique(c[(c >= 0) & (c < n)])


def lists(als, tt, top_k, als_wins, fallback=None, excl=None):
    """[(idx int64 [len], val f64 [len])] per row, lens int32 [n_rows],
    minmax f64 [n_rows, 4]."""
    als, tt = np.asarray(als, np.float32), np.asarray(tt, np.float32)
    n_rows, n = als.shape
    kk = min(int(top_k), n)
    out, lens, mms = [], np.zeros(n_rows, np.int32), np.zeros((n_rows, 4), np.float64)
    for r in range(n_rows):
        fused, mms[r] = fuse_row(substitute(als[r], fallback), tt[r], als_wins)
        order = ranking(fused)
        gone = excluded_set(excl, r, n)
        if gone.size:
            mask = np.zeros(n, bool)
            mask[gone] = True
            order = order[~mask[order]]
        lens[r] = min(kk, n - gone.size)
        idx = order[:kk].astype(np.int64)
        out.append((idx, fused[idx]))
    return out, lens, mms


def row_overflows(fused, gone, kk, sample, cap):
    """Whether mode 0 cuts this row's list: with n > sample, the bound is the
    kk-th best fused value of the first `sample` columns without the excluded
    ones (fewer than kk of them: everything passes); the live columns whose
    value reaches it (NaN: below every number, equal to NaN) must fit `cap`."""
    fused = np.asarray(fused, np.float64)
    n = fused.size
    if n <= sample:
        return False
    live = np.ones(n, bool)
    live[np.asarray(gone, np.int64)] = False
    s = fused[:sample][live[:sample]]
    if s.size < kk:
        return int(live.sum()) > cap
    bound = s[ranking(s)[kk - 1]]
    if np.isnan(bound):
        return int(live.sum()) > cap
    with np.errstate(invalid="ignore"):
        return int((live & (fused >= bound)).sum()) > cap
