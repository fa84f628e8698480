"""Greedy Maximal Marginal Relevance as include/hrec.h defines it for
hrec_mmr_rerank, in numpy (f64 by default, np.longdouble for the check of the
oracle itself), and the seeded inputs the CPU and GPU tests share.

Per row: the valid entries are the positions below the row's length whose
column is in [0, n). x_p = v_col(p) * inv_norm[col(p)] (zero where inv_norm is
0), lo / hi the extremes of the finite scores, rel_p = (s_p - lo) / (hi - lo)
(1 when hi == lo), value_p = lambda * rel_p - (1 - lambda) * max_{q in S} x_p .
x_q (lambda * rel_p while S is empty; -inf for a non-finite score). Each step
takes the unselected valid position with the largest value, the smaller
position among equals."""
import functools
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "pos len value gap deficit")

U = 2.0 ** -53


def tol(d):
    """8 (d + 4) u absolute: one normalised cosine is within (2 d + 5) u of the
    exact one on each side, lambda * rel - (1 - lambda) * maxsim
    adds at most four roundings a side: (4 d + 18) u <= 8 (d + 4) u."""
    return 8.0 * (d + 4) * U


def mmr(pool, scores, vectors, inv_norm, lam, top_n, pool_len=None, forced=None, dtype=np.float64):
    """pos int32 [R, top_n] (-1 past len), len int32 [R], value [R, top_n]
    (NaN past len), gap [R]: the smallest difference between the best and the
    second-best value over the row's steps (inf when no step had two
    candidates; 0 when two -inf values tie), deficit [R, top_n]: best value -
    selected value (0 for the oracle's own picks). forced (optional): int [R,
    >= top_n] positions to select instead of the arg-max (a kernel's output
    replayed); a forced position that is not an unselected valid entry raises
    AssertionError."""
    pool = np.asarray(pool, np.int64)
    R, P = pool.shape
    n = vectors.shape[0]
    lam = dtype(lam)
    pos = np.full((R, top_n), -1, np.int32)
    lens = np.zeros(R, np.int32)
    value = np.full((R, top_n), np.nan, dtype)
    gap = np.full(R, np.inf)
    deficit = np.zeros((R, top_n))
    for r in range(R):
        L = P if pool_len is None else min(max(int(pool_len[r]), 0), P)
        col = pool[r]
        idx = np.flatnonzero((np.arange(P) < L) & (col >= 0) & (col < n))
        m = min(top_n, idx.size)
        lens[r] = m
        if m == 0:
            continue
        c = col[idx]
        inv = np.asarray(inv_norm)[c].astype(dtype)
        with np.errstate(all="ignore"):
            x = np.asarray(vectors)[c].astype(dtype) * inv[:, None]
        x[inv == 0] = 0
        s = np.asarray(scores)[r, idx].astype(dtype)
        fin = np.isfinite(s)
        rel = np.full(idx.size, -np.inf, dtype)
        if fin.any():
            lo, hi = s[fin].min(), s[fin].max()
            with np.errstate(all="ignore"):
                rel[fin] = dtype(1.0) if hi == lo else ((s - lo) / (hi - lo))[fin]
        is_open = np.ones(idx.size, bool)
        maxsim = None
        for t in range(m):
            with np.errstate(all="ignore"):
                val = lam * rel if t == 0 else lam * rel - (dtype(1.0) - lam) * maxsim
            val = np.where(fin, val, -np.inf)
            oi = np.flatnonzero(is_open)
            v = val[oi]
            best = oi[int(np.argmax(v))]  # the first of equals: the smaller position
            if v.size >= 2:
                top2 = np.partition(v, -2)[-2:]
                g = 0.0 if top2[1] == top2[0] else float(top2[1] - top2[0])
                gap[r] = min(gap[r], g)
            sel = best
            if forced is not None:
                k = int(np.searchsorted(idx, int(forced[r][t])))
                assert k < idx.size and idx[k] == int(forced[r][t]) and is_open[k], \
                    f"row {r} step {t}: position {int(forced[r][t])} is not an unselected valid entry"
                sel = k
                deficit[r, t] = 0.0 if val[best] == val[sel] else float(val[best] - val[sel])
            pos[r, t] = idx[sel]
            value[r, t] = val[sel]
            is_open[sel] = False
            sim = x @ x[sel]
            maxsim = sim if t == 0 else np.maximum(maxsim, sim)
    return Result(pos, lens, value, gap, deficit)


def inv_norms(vectors):
    """hrec_row_inv_norms in f64: 1 / |row|, 0 where the squared norm is 0 or
    not finite. (The kernel's own sum order differs in the last bits; tests
    that compare bits read the kernel's inv_norm back instead.)"""
    with np.errstate(all="ignore"):
        s = (np.asarray(vectors, np.float64) ** 2).sum(axis=1)
        return np.where((s > 0) & np.isfinite(s), 1.0 / np.sqrt(s), 0.0)


# ---------------------------------------------------------------- the cases
# (d, pool, top_n, rows, lambda, f64 scores). The issue's sets — d {1, 8, 50,
# 64, 65, 128, 200, 256}, pool {1, 2, 63, 64, 65, 100, 257, 1024}, top_n {1,
# 10, pool}, rows {1, 5, 261}, lambda {0, 0.3, 0.7, 1}, both score types — are
# each covered in full; the cross product (4608 cases) is not run. The pairs
# (d, pool) are chosen so that every launch shape of the kernel is hit on both
# of its vector paths: blocks of 64 / 128 / 256 threads, 1, 2 and 4 positions
# per thread (pool 600 is added for the three-of-four case), rows staged in
# LDS (pool * (d | 1) * 4 <= 56 KiB) and re-read from global memory.
Case = namedtuple("Case", "d pool top_n rows lam f64")
CASES = [
    Case(1, 1, 1, 1, 0.7, False),
    Case(8, 2, 2, 5, 0.3, True),
    Case(50, 63, 10, 5, 0.7, False),      # staged, 64 threads
    Case(256, 63, 63, 1, 0.3, True),      # global, 64 threads
    Case(64, 64, 10, 261, 0.7, False),    # staged
    Case(256, 64, 64, 5, 0.0, True),      # global
    Case(65, 65, 65, 5, 0.3, False),      # staged, 128 threads
    Case(256, 65, 10, 1, 1.0, True),      # global, 128 threads
    Case(128, 100, 10, 261, 0.7, False),  # staged
    Case(200, 100, 100, 5, 0.3, True),    # global
    Case(64, 100, 10, 5, 1.0, False),
    Case(64, 100, 100, 5, 0.0, True),
    Case(50, 257, 10, 5, 0.7, True),      # staged, 2 positions per thread
    Case(64, 257, 257, 1, 0.3, False),    # global, 2 per thread
    Case(65, 257, 1, 261, 0.0, False),
    Case(50, 600, 10, 5, 0.7, False),     # global, 3 of 4 per thread
    Case(8, 600, 600, 1, 0.3, True),      # staged, 3 of 4 per thread
    Case(8, 1024, 10, 5, 0.7, False),     # staged, 4 per thread
    Case(1, 1024, 1024, 1, 0.3, True),    # staged; d = 1: every cosine is +-1, ties everywhere
    Case(128, 1024, 10, 5, 0.3, True),    # global, 4 per thread
    Case(256, 1024, 32, 1, 0.7, False),   # global
]
# Exact comparison of the selections: Gaussian vectors of d >= 16 and lambda in
# (0, 1), where the values are in general position (test_mmr_oracle.py checks
# the gap of each against 1e3 * tol).
EXACT_CASES = [c for c in CASES if c.d >= 16 and 0.0 < c.lam < 1.0]


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(pool int64 [rows, pool], scores f32 / f64 [rows, pool], vectors f32
    [n, d]) of a case, seeded by its shape: Gaussian vectors, every row's pool
    a draw of distinct columns, its scores distinct and descending. Cached and
    shared: do not modify."""
    d, P, _, R, _, f64 = case
    rng = np.random.default_rng(1000003 * d + 7919 * P + 31 * R + int(f64))
    n = max(2 * P, 40)
    vectors = rng.standard_normal((n, d)).astype(np.float32)
    pool = np.stack([rng.permutation(n)[:P] for _ in range(R)]).astype(np.int64)
    # position p + a jitter below half a step, scaled to (-4, 4]: distinct in f32 at every pool size
    s = 4.0 - 8.0 * (np.arange(P)[None, :] + rng.random((R, P)) * 0.5) / P
    s = s if f64 else s.astype(np.float32)
    assert all(np.unique(row).size == P for row in s) and (np.diff(s, axis=1) < 0).all()
    for a in (vectors, pool, s):
        a.setflags(write=False)
    return pool, s, vectors


@functools.lru_cache(maxsize=None)
def case_oracle(case):
    """The oracle's Result for a case, with inv_norms(vectors)."""
    pool, s, vectors = case_inputs(case)
    return mmr(pool, s, vectors, inv_norms(vectors), case.lam, case.top_n)
