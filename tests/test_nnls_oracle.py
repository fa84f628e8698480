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
tolerances, not much less."""
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
