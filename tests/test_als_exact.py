"""CPU: the extended-precision ALS reference of tests/als_exact.py is what it
claims to be on every problem the conditioning tests give it — before any
kernel is compared with it.

 * against mpmath at 50 digits (an independent statement of the normal
   equations from the f32 inputs) on the worst-conditioned k = 16 row of
   every family, explicit and implicit: 1e-15 of |x|_inf;
 * the second refinement step moves no row of any family by 1e-15 |x|_inf;
 * the C oracle solves every row of the same problems (no NaN) and |x| stays
   far inside the f32 range;
 * the implicit restatement agrees with tests/implicit_oracle.py;
 * the exact pieces (integer Gramian, int <-> longdouble) are exact."""
import numpy as np
import pytest

import als_exact as ax
import implicit_oracle as io
from oracle import build as obuild

ALL_KKP = ax.KKP_SMALL + ax.KKP_WIDE
LD = np.longdouble


# ------------------------------------------------------------ exact pieces
def test_integer_gramian_is_exact():
    rng = np.random.default_rng(1)
    S = (rng.normal(size=(37, 5)) * 2.0 ** rng.integers(-20, 12, size=(37, 5))).astype(np.float32)
    S[3, 2] = 0.0
    M, E = ax._int_columns(S)
    assert np.array_equal(np.ldexp(M.astype(np.float64), E[None, :].astype(np.int64)), S.astype(np.float64))
    G, Gl = ax._gram(M)
    Mo = M.astype(object)
    want = Mo.T.dot(Mo)
    assert (G == want).all()
    assert all(abs(ax._to_ld(int(want[i, j])) - Gl[i, j]) <= 2.0 ** -60 * abs(Gl[i, j]) for i in range(5) for j in range(5))
    assert (ax._colsum(M) == Mo.sum(axis=0)).all()


def test_longdouble_integer_round_trip():
    rng = np.random.default_rng(2)
    y = (rng.normal(size=40).astype(LD) + LD(2.0) ** -40 * rng.normal(size=40).astype(LD)) * LD(2.0) ** rng.integers(-30, 30, 40)
    y[7] = 0
    Y, q = ax._ld_to_ints(y)
    back = np.array([np.ldexp(ax._to_ld(v), q) for v in Y], LD)
    assert np.array_equal(back, y)  # 64-bit mantissas: _to_ld is exact below 2^120
    from fractions import Fraction

    W, s = ax._int_scale([0.1, 2.5, 0.0, 1e-9], "x")
    assert [Fraction(w, 2 ** s) for w in W] == [Fraction(v) for v in (0.1, 2.5, 0.0, 1e-9)]


# ------------------------------------------------------------------ mpmath
def _mp_solve(indptr, indices, values, src, k, reg, row, implicit, alpha):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    S = [[mp.mpf(float(v)) for v in r[:k]] for r in np.asarray(src, np.float32)]
    A = mp.zeros(k, k)
    b = mp.zeros(k, 1)
    if implicit:
        for y in S:
            for i in range(k):
                for j in range(k):
                    A[i, j] += y[i] * y[j]
    n = 0
    for p in range(int(indptr[row]), int(indptr[row + 1])):
        v, r = S[indices[p]], float(values[p])
        c1 = mp.mpf(float(np.float64(alpha) * abs(np.float64(r))))
        wa, wb = (c1, (1 + c1) if r > 0 else 0) if implicit else (1, mp.mpf(r))
        n += (r > 0) if implicit else 1
        for i in range(k):
            b[i] += wb * v[i]
            for j in range(k):
                A[i, j] += wa * v[i] * v[j]
    lam = mp.mpf(float(np.float64(n) * np.float64(reg)))
    for i in range(k):
        A[i, i] += lam
    x = mp.lu_solve(A, b)
    return [x[i] for i in range(k)], mp


@pytest.mark.parametrize("implicit,alpha", [(False, 0.0), (True, 40.0)], ids=["explicit", "implicit40"])
@pytest.mark.parametrize("name", list(ax.FAMILIES))
def test_longdouble_solver_matches_mpmath(name, implicit, alpha):
    ref = ax.family_reference(name, 16, 16, implicit, alpha)
    row = int(np.argmax(ref["kappa"]))
    want, mp = _mp_solve(*ref["problem"], 16, ref["reg"], row, implicit, alpha)
    Y, q = ax._ld_to_ints(ref["x"][row])
    got = [mp.mpf(v) * mp.mpf(2) ** q for v in Y]  # the longdouble solution, exactly
    norm = max(abs(w) for w in want)
    err = max(abs(g - w) for g, w in zip(got, want)) / norm
    print(f"{name}: kappa {ref['kappa'][row]:.2e}, |x - x_mp|_inf / |x_mp|_inf = {float(err):.2e}")
    assert err <= 1e-15


# ------------------------------------------- refinement, oracle, f32 range
@pytest.mark.parametrize("k,kp", ALL_KKP)
@pytest.mark.parametrize("name", list(ax.FAMILIES))
def test_reference_converged_and_oracle_solves_every_row(name, k, kp):
    ref = ax.family_reference(name, k, kp)
    indptr, indices, values, src = ref["problem"]
    deg = np.diff(indptr)
    assert list(deg) == ax.row_lengths(k, kp) and (src[:, k:] == 0).all()
    assert indices.min() == 0 and indices.max() == src.shape[0] - 1, "the first and the last source row are used"
    assert (values <= 0).any() and (values < 0).any()
    print(f"{name} k={k}: kappa {ref['kappa'][deg > 0].min():.2e} .. {ref['kappa'].max():.2e}, "
          f"last step {ref['last_step'].max():.1e}, |x| max {float(np.abs(ref['x']).max()):.2e}")
    assert (ref["last_step"] < 1e-15).all()
    assert ref["kappa"].max() < 1e12, "beyond this the reference itself is not converged in two steps"
    nz = np.abs(ref["x"][deg > 0])
    assert nz.max() < 1e5 and nz.max(axis=1).min() > 1e-12,"|x| far inside the f32 range"
    assert (ref["x"][0] == 0).all()
    got = obuild.half_sweep(indptr, indices, values, src, k, ref["reg"])
    assert np.isfinite(got).all(), "the C oracle fails on no row"
    # and it is an accurate f64 solver there: rho (als_exact.rho) of order 1, far below the
    # 3 (k + 1) of Cholesky's worst-case backward error — the GPU tests allow 32 x this rho,
    # so a bad oracle build must not be able to widen their bound unnoticed
    rho = ax.rho(got, ref["x"], ref["kappa"])
    print("rho_oracle max:", float(rho.max()))
    assert rho.max() < 8.0


@pytest.mark.parametrize("alpha", ax.ALPHAS)
@pytest.mark.parametrize("k,kp", ax.KKP_IMPLICIT)
@pytest.mark.parametrize("name", list(ax.FAMILIES))
def test_implicit_reference_converged(name, k, kp, alpha):
    ref = ax.family_reference(name, k, kp, True, alpha)
    print(f"{name} k={k} alpha={alpha}: kappa max {ref['kappa'].max():.2e}, last step {ref['last_step'].max():.1e}")
    assert (ref["last_step"] < 1e-15).all()
    assert ref["kappa"].max() < 1e12
    assert np.abs(ref["x"]).max() < 1e5
    assert (ref["x"][0] == 0).all() and (ref["x"][ax.NONPOS_ROW] == 0).all()


@pytest.mark.parametrize("alpha", [0.0] + ax.ALPHAS)
@pytest.mark.parametrize("k,kp", [(10, 16), (33, 64)])
def test_implicit_restatement_matches_implicit_oracle(k, kp, alpha):
    """gauss (kappa < 1e3): the f64 numpy restatement is correctly rounded to
    f32 up to its own kappa u, so it sits inside the bound with rho_max = 32."""
    ref = ax.family_reference("gauss", k, kp, True, alpha)
    indptr, indices, values, src = ref["problem"]
    got = io.half_sweep(indptr, indices, values, src, k, ref["reg"], alpha)
    assert (np.abs(got.astype(LD) - ref["x"]) <= ax.bound(ref["x"], ref["kappa"], 32.0)).all()
    y = ax.yty_longdouble(src, k).astype(np.float64)
    a = np.abs(src[:, :k].astype(np.float64))
    assert (np.abs(y - io.gramian(src[:, :k])) <= src.shape[0] * 2.0 ** -52 * (a.T @ a)).all()


# ------------------------------------------------------------- f32 chunks
def test_mode1_families_are_those_inside_its_documented_limit():
    """accum_mode 1 is run on the families up to corr2 whose first-order
    bound kappa * 16 * 2^-24 stays below 2^-10 at every size."""
    for name in ("gauss", "corr2"):
        worst = max(ax.family_reference(name, k, kp)["kappa"].max() for k, kp in ax.KKP_SMALL) * ax.MODE1_UNIT
        print(f"{name}: kappa * 16 * 2^-24 = {worst:.2e} (limit {2.0 ** -10:.2e})")
        assert (worst <= 2.0 ** -10) == (name in ax.MODE1_FAMILIES)


# ---------------------------------------------------------- singular rows
@pytest.mark.parametrize("k,kp", [(16, 16), (64, 64), (128, 128)])
def test_singular_rows_fail_in_the_oracle_only(k, kp):
    (indptr, indices, values, src), sing = ax.singular_problem(k, kp, np.random.default_rng(k))
    got = obuild.half_sweep(indptr, indices, values, src, k, 0.0)
    assert np.isnan(got[sing]).all() and np.isfinite(got[:sing[0]]).all()
    with pytest.raises(np.linalg.LinAlgError):
        ax.solve_rows(indptr, indices, values, src, k, 0.0)
    st = {}
    x, kappa = ax.solve_rows(indptr[:sing[0] + 1], indices, values, src, k, 0.0, stats=st)
    assert (st["last_step"] < 1e-15).all() and kappa.max() < 1e4
    assert (np.abs(got[:sing[0]].astype(LD) - x) <= ax.bound(x, kappa, 32.0)).all()
