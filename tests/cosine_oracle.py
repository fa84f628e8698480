"""The numpy oracle of hrec_cosine_topk (include/hrec.h has the contract).

dot(q, j) is the f64 chain acc = acc + (double)v_q[c] * (double)v_j[c], c
ascending from 0.0. The product of two f32 values is exact in f64, so
np.add.accumulate over the f64 products (a strictly sequential sum along the
axis) reproduces it bit for bit, fused or not on the device.
sim = (dot * inv_norm[q]) * inv_norm[j], +0.0 where either inv_norm is 0. The
ranking is a stable sort on (-sim, column); with skip_self the query's own
column leaves first; the list is cut to kk = min(top_k, n - skip_self), then
to the prefix with sim > min_sim."""
import numpy as np


def inv_norms(vectors, d=None):
    """hrec_row_inv_norms up to the order of its sum (tests of the kernel take
    the kernel's own values, read back)."""
    v = np.asarray(vectors, np.float32)[:, :d].astype(np.float64)
    s = (v * v).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((s > 0) & np.isfinite(s), 1.0 / np.sqrt(s), 0.0)


def sims(vectors, d, inv_norm, query_rows, chunk=None):
    """f64 [n_q, n]: the contract's sim for every (query, column); NaN rows
    for unknown queries (a row outside [0, n)). chunk: queries per block of
    products (None: about 2^26 products)."""
    v = np.ascontiguousarray(np.asarray(vectors, np.float32)[:, :d]).astype(np.float64)
    inv = np.asarray(inv_norm, np.float64)
    q = np.asarray(query_rows, np.int64).reshape(-1)
    n = v.shape[0]
    out = np.full((q.size, n), np.nan, np.float64)
    known = np.flatnonzero((q >= 0) & (q < n))
    chunk = chunk or max(1, (1 << 26) // max(n * v.shape[1], 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, known.size, chunk):
            b = known[lo: lo + chunk]
            prod = v[q[b]][:, None, :] * v[None, :, :]            # exact products [b, n, d]
            dot = np.add.accumulate(prod, axis=2)[:, :, -1]       # the sequential chain
            s = (dot * inv[q[b]][:, None]) * inv[None, :]
            zero = (inv[q[b]][:, None] == 0.0) | (inv[None, :] == 0.0)
            out[b] = np.where(zero, 0.0, s)
    return out


def topk(vectors, d, inv_norm, query_rows, top_k, skip_self=True, min_sim=-np.inf, s=None):
    """(out_idx int64 [n_q, top_k], out_val f64, out_len int32): -1 / NaN past
    out_len, out_len 0 for an unknown query. s (optional): sims() of the same
    inputs, computed once for several calls."""
    q = np.asarray(query_rows, np.int64).reshape(-1)
    n = int(np.asarray(vectors).shape[0])
    s = sims(vectors, d, inv_norm, q) if s is None else s
    kk = min(int(top_k), n - int(bool(skip_self)))
    idx = np.full((q.size, top_k), -1, np.int64)
    val = np.full((q.size, top_k), np.nan, np.float64)
    ln = np.zeros(q.size, np.int32)
    for b, r in enumerate(q):
        if not 0 <= r < n:
            continue
        row = s[b]
        assert np.isfinite(row).all()  # every sim is finite
        order = np.argsort(-row, kind="stable")  # larger first, equal sims: the smaller column
        if skip_self:
            order = order[order != r]
        order = order[:kk]
        keep = row[order] > min_sim
        m = int(keep.sum())
        assert keep[:m].all()  # a prefix
        idx[b, :m], val[b, :m], ln[b] = order[:m], row[order[:m]], m
    return idx, val, ln
