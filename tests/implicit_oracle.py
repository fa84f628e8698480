"""f64 numpy restatement of Spark 3.5 ALS.computeFactors, implicit branch (the
checker of the implicit-feedback tests): YtY = S^T S, then per destination
row, one rating at a time,
  c1 = alpha |r|,  A += c1 v v^T,  b += (1 + c1) v if r > 0,  n_pos += r > 0,
  A[d][d] += reg n_pos,  solve A x = b in f64, round to f32."""
import numpy as np


def gramian(src):
    s = np.asarray(src, np.float64)
    return s.T @ s


def half_sweep(indptr, indices, values, src, k, reg, alpha, yty=None):
    """src [n_src, >= k] f32 -> [n_rows, k] f32."""
    s = np.asarray(src, np.float64)[:, :k]
    yty = gramian(s) if yty is None else np.asarray(yty, np.float64)[:k, :k]
    n_rows = len(indptr) - 1
    out = np.zeros((n_rows, k), np.float32)
    for r in range(n_rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            continue
        A = yty.copy()
        b = np.zeros(k)
        n_pos = 0
        for j in range(lo, hi):
            v = s[indices[j]]
            rating = float(values[j])
            c1 = alpha * abs(rating)
            A += c1 * np.outer(v, v)
            if rating > 0:
                b += (1.0 + c1) * v
                n_pos += 1
        if n_pos == 0:
            continue  # b = 0: the factor is exactly zero
        A[np.diag_indices(k)] += reg * n_pos
        out[r] = np.linalg.solve(A, b).astype(np.float32)
    return out


def fit(user_csr, item_csc, U0, k, reg, alpha, iters):
    """Items from users, then users from items; (U, V) f32."""
    U = np.asarray(U0, np.float32)[:, :k].copy()
    V = None
    for _ in range(iters):
        V = half_sweep(*item_csc, U, k, reg, alpha)
        U = half_sweep(*user_csr, V, k, reg, alpha)
    return U, V


def coo_to_csr(rows, cols, vals, n_rows):
    """Rows ascending, a row's entries in input order (duplicates kept)."""
    rows = np.asarray(rows)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n_rows + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n_rows))
    return indptr, np.asarray(cols)[order].astype(np.int32), np.asarray(vals, np.float32)[order]
