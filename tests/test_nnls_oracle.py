"""CPU: checks of the checker of the non-negative ALS tests
(tests/nnls_oracle.py, Spark's NNLS.solve restated in numpy f64).
(a) On the row problems of the GPU half-sweep test it lands on the exact
    non-negative least-squares solution (scipy's active-set NNLS of
    min |L^T x - L^-1 b| with A = L L^T) within the one-sweep bound.
(b) Run with the terms of every dot and matrix-vector product in reverse, it
    agrees with itself to a tenth of the GPU tolerances (one sweep: per row
    1e-5 max|row| + 1e-6; a fit: rtol 1e-4 / atol 1e-5): two faithful
    implementations of the iteration differ by less than the tests allow.

Measured: (a) at most 0.11 of the bound (k 64, implicit, sources >= 0). (b) a
sweep at most 0.30 of the tenth; the fits, V / U: 0.17 / 0.17 (k 16 explicit),
0.78 / 0.26 (k 64 implicit), 0.08 / 0.23 (k 64 explicit) of the tenth.
The margin is thinner than these figures suggest at k 64 with alpha 40, where
rows take 50 .. 100 iterations: other orders tried while writing this test (the
kernel's lane order, three random permutations) gave up to 1.02 of the tenth on
that sweep and 0.80 .. 1.10 on that fit, the largest fit difference on an entry
of 3e-5 in a row whose maximum is 0.7 (the solver stops on a norm, so a row's
small entries carry the row's absolute error, while the fit tolerance is per
element). Two faithful orders there differ by about a tenth of the GPU
tolerances, not much less.

(c) Where the iteration branches (nnls_oracle.hard_cases(): the families of
    als_exact plus tiny and ties, which reach the stop rules, the iteration cap
    and multi-entry wall steps that (a) and (b) never see). Six summation
    orders of every row:
    - stable families: a row is stable when all six orders agree with the
      natural one within 1e-6 max|row| after the f32 cast (a tenth of the GPU
      bound, purely relative: tiny and scaled_down have entries near 1e-12 and
      1e-6). At most one unstable row per case and 1 % of all rows; the set is
      pinned (nnls_oracle.UNSTABLE_ROWS). Measured: 717 of 719 rows stable,
      worst stable ratio 0.57 (graded k 20).
    - what each family is for is asserted: scaled_up stops on step < 1e-7 at
      x = 0, tiny explicit too (the 1e-20 guard), tiny implicit runs to the
      cap in every order, ties has steps that zero two entries at once.
    - chaotic families (corr2, corr3, explicit): the orders differ by O(1) of
      a row, so only f(x) = x^T A x / 2 - b^T x is compared: every order ends
      at or below the natural order's iterate after 32 steps (each accepted
      step is an exact line search along a descent direction, cut at the
      bound; a CG step with a non-positive step length is rejected by
      step < 1e-7). Smallest margin measured 2.7e-7 |f| (corr3 k 10), 8.5e-5
      on the rows at the cap. The rows at the cap in all six orders are pinned
      (nnls_oracle.CAP_ROWS)."""
import functools

import numpy as np
import pytest

import nnls_oracle as no

REG, ALPHA = 0.1, 40.0
CASES = [(k, kp, signed, imp) for k, kp in no.KKP for signed in (True, False) for imp in (False, True)]
FITS = [(400, 300, 0.05, 16, False), (300, 200, 0.05, 64, True), (300, 200, 0.05, 64, False)]


def _row_bound(exp, scale=1.0):
    return scale * (1e-5 * np.abs(exp).max(axis=1, keepdims=True) + 1e-6)


def _second_order(k):
    """The terms of every sum in reverse."""
    return np.arange(k)[::-1].copy()


@pytest.mark.parametrize("k,kp,signed,imp", CASES)
def test_oracle_matches_exact_nnls(k, kp, signed, imp):
    from scipy.linalg import solve_triangular
    from scipy.optimize import nnls

    prob = no.sweep_problem(k, kp, signed)
    got, iters = no.half_sweep(*prob, k, REG, imp, ALPHA, return_iters=True)
    eqs = no.normal_equations(*prob, k, REG, imp, ALPHA)
    exact = np.zeros_like(got, dtype=np.float64)
    for r, eq in enumerate(eqs):
        if eq is not None:
            L = np.linalg.cholesky(eq[0])
            exact[r] = nnls(L.T, solve_triangular(L, eq[1], lower=True), maxiter=100 * k)[0]
    err = np.abs(got - exact)
    print("oracle vs exact NNLS, worst err / bound:", float((err / _row_bound(exact)).max()))
    assert (err <= _row_bound(exact)).all()
    assert (got >= 0).all()
    assert eqs[0] is None and iters[0] == 0
    assert (iters <= no.iter_max(k)).all()
    # rows with a non-zero solution take iterations; with signed sources they touch the bound
    solved = [r for r, eq in enumerate(eqs) if eq is not None and exact[r].max() > 0]
    assert solved and all(iters[r] > 0 for r in solved)
    if signed:
        assert all((got[r] == 0).any() for r in solved)
    if imp or not signed:  # no rating > 0 / b <= 0: exactly zero, no iteration
        assert (got[no.ROW_NONPOS] == 0).all() and iters[no.ROW_NONPOS] == 0


@pytest.mark.parametrize("k,kp,signed,imp", CASES)
def test_two_summation_orders_agree_on_a_sweep(k, kp, signed, imp):
    prob = no.sweep_problem(k, kp, signed)
    a = no.half_sweep(*prob, k, REG, imp, ALPHA)
    b = no.half_sweep(*prob, k, REG, imp, ALPHA, perm=_second_order(k))
    err = np.abs(a.astype(np.float64) - b)
    print("two orders, worst err / (bound / 10):", float((err / _row_bound(a, 0.1)).max()))
    assert (err <= _row_bound(a, 0.1)).all()


@pytest.mark.parametrize("n_users,n_items,dens,k,imp", FITS)
def test_two_summation_orders_agree_on_a_fit(n_users, n_items, dens, k, imp):
    ucsr, icsc, U0, Ua, Va = no.synthetic_fit(n_users, n_items, dens, k, imp, ALPHA)
    Ub, Vb = no.fit(ucsr, icsc, U0, k, REG, 3, imp, ALPHA, perm=_second_order(k))
    for a, b in ((Va, Vb), (Ua, Ub)):
        print("two orders over a fit, worst err / (tol / 10):",
              float((np.abs(a.astype(np.float64) - b) / (1e-6 + 1e-5 * np.abs(b))).max()))
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6)
    assert (Ua >= 0).all() and (Va >= 0).all() and (Ua == 0).mean() > 0.05 and (Va == 0).mean() > 0.05


# ------------------------------------------- (c) where the iteration branches
HARD = no.hard_cases()
HARD_STABLE = [c for c in HARD if c[0] in no.STABLE]
HARD_CHAOTIC = [c for c in HARD if c[0] in no.CHAOTIC]


def _id(case):
    return "%s-%d-%s" % (case[0], case[1], no.mode_key(case[3], case[4]))


@functools.lru_cache(maxsize=None)
def _six(case):
    """The case in the six orders, shared read-only: (solved rows, x f32
    [6, rows, k], iterations [6, rows], events [6][rows])."""
    name, k, kp, imp, alpha = case
    ref = no.hard_reference(*case)
    n = len(ref["eqs"])
    solved = [r for r, eq in enumerate(ref["eqs"]) if eq is not None]
    xs, its, evs = np.zeros((6, n, k), np.float32), np.zeros((6, n), np.int64), []
    for o, perm in enumerate(no.orders(k, kp)):
        evs.append([None] * n)
        for r in solved:
            evs[o][r] = {}
            x, its[o, r] = no.solve(*ref["eqs"][r], perm=perm, events=evs[o][r])
            xs[o, r] = x.astype(np.float32)
    assert np.array_equal(xs[0], ref["exp"]) and np.array_equal(its[0], ref["iters"])
    xs.setflags(write=False)
    its.setflags(write=False)
    return solved, xs, its, evs


def _instability(case):
    """Per solved row: max over the orders of |x_order - x_natural|_inf / (1e-6 |x_natural|_inf);
    0 where all orders give the natural order's bits."""
    solved, xs, _, _ = _six(case)
    x = xs.astype(np.float64)
    d = np.abs(x[1:] - x[0]).max(axis=(0, 2))
    scale = 1e-6 * np.abs(x[0]).max(axis=1)
    with np.errstate(all="ignore"):
        return {r: 0.0 if d[r] == 0 else float(d[r] / scale[r]) for r in solved}


def test_defaults_of_solve_are_unchanged():
    """events and max_iter leave the result alone; max_iter gives the iterate on the way."""
    ref = no.hard_reference("gauss", 20, 32, False, 0.0)
    A, b = ref["eqs"][6]
    x, it = no.solve(A, b)
    ev = {}
    x2, it2 = no.solve(A, b, events=ev, max_iter=10 ** 6)
    assert np.array_equal(x, x2) and it == it2 > 5 and ev["stop"] in ("small", "rel")
    ev = {}
    x5, it5 = no.solve(A, b, max_iter=5, events=ev)
    assert it5 == 5 and ev["stop"] == "max_iter" and not np.array_equal(x5, x)
    assert no.objective(A, b, x) < no.objective(A, b, x5) < 0


def test_orders():
    for k, kp in no.KKP:
        o = no.orders(k, kp)
        assert len(o) == 6 and o[0] is None and o[1].tolist() == list(range(k))[::-1]
        assert all(sorted(p.tolist()) == list(range(k)) for p in o[1:])
        assert len({tuple(p.tolist()) for p in o[1:]}) == 5
    assert no.orders(20, 32)[2].tolist()[:6] == [0, 2, 4, 6, 8, 10]


@pytest.mark.parametrize("case", HARD_STABLE, ids=_id)
def test_stable_family_rows_agree_in_six_orders(case):
    name, k, kp, imp, alpha = case
    solved, xs, its, evs = _six(case)
    ratio = _instability(case)
    unstable = tuple(r for r in solved if not ratio[r] <= 1.0)
    print("stable", _id(case), "worst stable ratio:", max([ratio[r] for r in solved if r not in unstable] + [0.0]),
          "unstable rows:", unstable, "iterations:", its[0].tolist())
    assert unstable == no.unstable_rows(*case), "the pinned set of unstable rows"
    assert len(unstable) <= 1
    assert np.isfinite(xs).all() and (xs >= 0).all() and (its <= no.iter_max(k)).all()
    cap = tuple(r for r in solved if (its[:, r] == no.iter_max(k)).all())
    assert cap == no.cap_rows(name, k, imp, alpha), "the pinned set of rows at the cap in every order"
    stops = lambda r: {evs[o][r]["stop"] for o in range(6)}  # noqa: E731
    if name == "scaled_up" and (imp or k >= 20):
        assert all((xs[:, r] == 0).all() and (its[:, r] == 0).all() and stops(r) == {"small"} for r in solved)
    if name == "tiny" and not imp:
        assert all((xs[:, r] == 0).all() and (its[:, r] == 0).all() and stops(r) == {"small"} for r in solved)
    if name == "tiny" and imp:
        assert len(cap) == (len(solved) if k <= 33 else 8) and len(solved) == (9 if k >= 33 else 6)
        assert all(stops(r) == {"cap"} for r in cap)
        # the orders agree to below 1e-10 of the row although they take iter_max(k) tiny steps
        assert max(ratio.values()) <= 1e-4
    if name == "ties" and k >= 16:
        assert sum(evs[0][r]["multi"] for r in solved) >= 1
    # a row with an all-zero result took no step, in any order
    assert all((its[:, r] == 0).all() for r in solved if (xs[0, r] == 0).all())


def test_stable_families_as_a_whole():
    rows = unstable = 0
    seen, rejected = set(), 0
    for case in HARD_STABLE:
        solved, _, _, evs = _six(case)
        rows += len(solved)
        unstable += len(no.unstable_rows(*case))
        seen |= {evs[0][r]["stop"] for r in solved}
        rejected += sum(evs[0][r]["rejected"] for r in solved)
    print("rows:", rows, "unstable:", unstable, "stop rules:", sorted(seen), "rejected CG steps:", rejected)
    assert rows == 719 and unstable <= 0.01 * rows
    assert {"small", "rel", "cap"} <= seen and rejected >= 1


@pytest.mark.parametrize("case", HARD_CHAOTIC, ids=_id)
def test_chaotic_family_rows_descend_in_six_orders(case):
    name, k, kp, imp, alpha = case
    ref = no.hard_reference(*case)
    solved, xs, its, evs = _six(case)
    ratio = _instability(case)
    loose = no.unstable_rows(*case)
    assert [r for r in solved if r not in loose] == [1] and ratio[1] <= 1.0 and (its[:, 1] == 1).all(), \
        "a single rating: one exact step in every order"
    assert (its[:, list(loose)] >= 2).all()
    assert np.isfinite(xs).all() and (xs >= 0).all() and (its <= no.iter_max(k)).all()
    margin = np.inf
    for r in solved:
        A, b = ref["eqs"][r]
        f32 = no.objective(A, b, ref["x32"][r])
        assert f32 < 0
        for o in range(6):
            f = no.objective(A, b, xs[o, r])
            assert f <= f32 + 1e-9 * abs(f32), (r, o, float(f), float(f32))
            margin = min(margin, float((f32 - f) / abs(f32)))
    cap = tuple(r for r in solved if (its[:, r] == no.iter_max(k)).all())
    print("chaotic", _id(case), "worst instability:", max(ratio.values()), "smallest margin of f:", margin,
          "rows at the cap in every order:", cap)
    assert cap == no.cap_rows(name, k, imp, alpha), "the pinned set of rows at the cap in every order"
    if name == "corr3" and k == 64:
        assert len(cap) >= 3
