"""The ALS cold-start fallback as the reference computes it (its
src/als_model.py:78-86 and :93-104), restated with sklearn's own
cosine_similarity on f64 rows, and the seeded inputs the CPU and GPU tests
share. Nothing here goes through the package or the library.

Per item q: the OTHER items in dict (row) order with their similarity to q,
sorted stable and descending; the first 3 of them, kept where sim > 0.5; the
fallback value is np.mean of the kept items' ratings in that order (the
global mean when none is kept). sklearn normalises a row by its norm, with a
norm below 10 * eps taken as 1 (preprocessing.normalize ->
_handle_zeros_in_scale): a row that small is NOT scaled up to a unit vector.

Tolerance. One normalised cosine of dim terms differs between any two f64
evaluation orders, with or without FMA, by at most tol(dim) = (dim + 4) 2^-52
on each side: the dot of two unit vectors has dim roundings of terms bounded
by 1 (Cauchy-Schwarz), the two divisions and the square root give the rest.

A query is *decided* when its list is the same under every such evaluation:
the gaps between consecutive kept similarities, the gap between the 3rd and
the 4th when three are kept, and the distance of each of the first four from
0.5 all exceed MARGIN * tol(dim)."""
import functools
from collections import namedtuple

import numpy as np
from sklearn.metrics.pairwise import cosine_similarity

K = 3            # _find_similar_items' k
THRESHOLD = 0.5  # ... and its sim > 0.5
MARGIN = 1e3     # decided: gaps above MARGIN * tol(dim) (the margin of test_mmr_oracle.py)
SMALL = 10 * np.finfo(np.float64).eps  # sklearn: a norm below this is taken as 1


def tol(dim):
    return (dim + 4) * 2.0 ** -52


def similarity_matrix(X):
    """cosine_similarity(X) [n, n] (the diagonal is the item itself: callers
    leave it out)."""
    return cosine_similarity(np.asarray(X, np.float64))


def pair_similarities(X, q):
    """(others, sims) of item q exactly as the reference's loop takes them: one
    cosine_similarity([target], [other])[0][0] per other item, in row order."""
    X = np.asarray(X, np.float64)
    others = [j for j in range(len(X)) if j != q]
    return others, np.array([cosine_similarity([X[q]], [X[j]])[0][0] for j in others], np.float64)


def matrix_similarities(S, q):
    """(others, sims) of item q from a similarity matrix, in row order."""
    others = [j for j in range(S.shape[0]) if j != q]
    return others, S[q, others]


def ranked(others, sims):
    """The other items and their similarities, sorted stable and descending
    (sorted(..., key=sim, reverse=True) keeps the row order of equals)."""
    order = sorted(range(len(others)), key=lambda p: sims[p], reverse=True)
    return [others[p] for p in order], [sims[p] for p in order]


def kept(others, sims):
    """_find_similar_items: the first K of the ranking with sim > THRESHOLD."""
    ro, rs = ranked(others, sims)
    return [j for j, s in zip(ro[:K], rs[:K]) if s > THRESHOLD]


def mean_rating(ratings, items):
    """np.mean of the kept items' ratings in list order; None for an empty list
    (the caller's global mean)."""
    return np.mean([ratings[j] for j in items]) if items else None


def slack(others, sims, dim):
    """The smallest of the gaps that decide item q's list, divided by
    MARGIN * tol(dim): the query is decided when this is above 1."""
    _, rs = ranked(others, sims)
    n_kept = sum(s > THRESHOLD for s in rs[:K])
    gaps = [rs[i] - rs[i + 1] for i in range(n_kept - 1)]
    if n_kept == K and len(rs) > K:
        gaps.append(rs[K - 1] - rs[K])
    gaps += [abs(s - THRESHOLD) for s in rs[:K + 1]]
    return min(gaps) / (MARGIN * tol(dim)) if gaps else np.inf


Oracle = namedtuple("Oracle", "sim lists means slack")


def fallback(X, ratings):
    """Matrix form for a whole case: sim = cosine_similarity(X) [n, n], lists
    (the kept rows per item), means (np.float64 or None per item) and the
    slack of every query."""
    X = np.asarray(X, np.float64)
    S = similarity_matrix(X)
    lists, means, sl = [], [], []
    for q in range(len(X)):
        others, sims = matrix_similarities(S, q)
        lists.append(kept(others, sims))
        means.append(mean_rating(ratings, lists[-1]))
        sl.append(slack(others, sims, X.shape[1]))
    return Oracle(S, lists, means, np.array(sl))


# ---------------------------------------------------------------- the cases
# "plain": Gaussian features, integer ratings 0 .. 18 stored as floats. The
# widths sit on each side of the pair kernel's template switches (4 | 5, 8 |
# 9) and at its ends (2, 16; dim 1 has every similarity +-1: nothing is
# decided there); n is one past a multiple of the 256-item tile and 256-query
# block (513), several slices per query with a ragged last tile (the rest).
# "edge": the designed rows below written over a plain case.
Case = namedtuple("Case", "n dim edge")
PLAIN_CASES = [Case(300, 2, False), Case(513, 3, False), Case(513, 4, False), Case(600, 5, False),
               Case(700, 8, False), Case(520, 9, False), Case(777, 16, False)]
EDGE_CASES = [Case(513, 2, True), Case(513, 3, True), Case(520, 9, True), Case(300, 16, True)]
CASES = PLAIN_CASES + EDGE_CASES
SEED = 1


def case_id(case):
    return "%s-n%d-d%d" % ("edge" if case.edge else "plain", case.n, case.dim)


# row -> (scale, coefficient of e, coefficient of f), e and f the first two unit
# vectors. Every tiny norm is at least 0.5 % away from 10 * eps = 2.2204e-15,
# so the order of the norm's sum cannot move it across.
EDGE_ROWS = {
    "tiny_a": (3, (1e-16, 1.0, 0.0)),     # parallel to tiny_b, both norms below 10 * eps:
    "tiny_b": (11, (3e-16, 1.0, 0.0)),    # similarity 1e-32 to each other, not 1
    "zero": (20, (0.0, 0.0, 0.0)),
    "above": (33, (2.3e-15, 1.0, 0.0)),   # just above the threshold: normalised to e
    "below": (34, (2.2e-15, 1.0, 0.0)),   # just below: left as it is
    "under_a": (47, (1e-200, 1.0, 0.0)),  # the squares underflow: norm 0
    "under_b": (58, (2e-200, 1.0, 0.2)),
    "partner_a": (100, (1.0, 1.0, 0.1)),  # ordinary rows near e, distinct directions
    "partner_b": (200, (2.0, 1.0, 0.3)),
    "partner_c": (259, (0.5, 1.0, 0.5)),  # in the second 256-item tile
    "tiny_far": (-3, (1e-16, 1.0, 0.05)),  # row n - 3: another tile / slice
}
TINY = ("tiny_a", "tiny_b", "zero", "below", "under_a", "under_b", "tiny_far")


def edge_rows(case):
    """name -> row index of the designed rows of an edge case."""
    return {name: r % case.n for name, (r, _) in EDGE_ROWS.items()}


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(X f64 [n, dim], ratings f64 [n]) of a case. Cached and shared: do not
    modify."""
    rng = np.random.default_rng(SEED)
    X = rng.normal(size=(case.n, case.dim))
    ratings = rng.integers(0, 19, case.n).astype(np.float64)
    if case.edge:
        for r, (scale, ce, cf) in EDGE_ROWS.values():
            X[r] = 0.0
            X[r, 0] = scale * ce
            X[r, 1] = scale * cf
    X.setflags(write=False)
    ratings.setflags(write=False)
    return X, ratings


@functools.lru_cache(maxsize=None)
def case_oracle(case):
    return fallback(*case_inputs(case))
