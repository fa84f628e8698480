"""Extended-precision reference of one ALS half-sweep (host only, numpy) and
the ill-conditioned problem families of the conditioning tests.

solve_rows() returns, per destination row, the solution of Spark's normal
equations for the GIVEN f32 inputs:

  explicit:  A = sum v v^T + lambda I,            b = sum r v,   lambda = n * reg
  implicit:  A = YtY + sum c1 v v^T + lambda I,   b = sum_{r > 0} (1 + c1) v,
             c1 = alpha |r|,  lambda = n_pos * reg,  x = 0 when no rating is > 0

(lambda and c1 are the f64 products Spark forms). It is written from those
formulas alone — it shares nothing with oracle/als_oracle.c or the kernels.

How it reaches kappa * 2^-64 and better. An f32 is an integer times a power of
two, so A and b are EXACT integers once every source column is scaled by a
power of two: the Gramian of the integer matrix is summed exactly (20-bit
limbs through f64 matrix products, every partial sum below 2^53) and kept as
Python integers. The system is then solved in numpy.longdouble: a hand-written
Cholesky (column-vectorised) of the longdouble image of A, and two steps of
iterative refinement that reuse the factor and take the residual b - A x from
the exact integers (rounded once, to longdouble). With an exact residual the
refinement contracts by about kappa * 2^-64 per step, so after two steps x is
the longdouble rounding of the exact solution for every kappa < 1e12 or so;
tests/test_als_exact.py checks that against mpmath and on the step sizes.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "als_exact needs the x87 80-bit long double (x86-64)"

_LIMB = 20          # bits per limb: (2^20)^2 * 4096 terms = 2^52 < 2^53
_MAX_TERMS = 4096
_MAX_SHIFT = 36     # 24-bit mantissa << 36 stays below 2^60 = three limbs


# ------------------------------------------------------------ exact pieces
def _int_columns(S):
    """S f32 [n, k] -> (M int64 [n, k], E int64 [k]) with S[:, c] = M[:, c] * 2^E[c] exactly."""
    m, e = np.frexp(np.asarray(S, np.float32).astype(np.float64))
    mi = np.rint(m * 2.0 ** 24).astype(np.int64)  # an f32's 24-bit mantissa: exact
    e = e.astype(np.int64) - 24
    nz = mi != 0
    emin = np.where(nz, e, np.iinfo(np.int64).max).min(axis=0) if S.shape[0] else np.zeros(S.shape[1], np.int64)
    emin = np.where(nz.any(axis=0), emin, 0)
    sh = np.where(nz, e - emin[None, :], 0)
    if sh.size and sh.max() > _MAX_SHIFT:
        raise ValueError("a source column spans more than 2^%d: outside the exact accumulation" % _MAX_SHIFT)
    return mi << sh, emin


def _limbs(M):
    s, a = np.sign(M), np.abs(M)
    return [(s * ((a >> (_LIMB * j)) & ((1 << _LIMB) - 1))).astype(np.float64) for j in range(3)]


def _gram(M):
    """M int64 [n, k], |M| < 2^60 -> (M^T M as Python ints [k, k], its longdouble image)."""
    n, k = M.shape
    if n > _MAX_TERMS:
        raise ValueError("more than %d terms: outside the exact accumulation" % _MAX_TERMS)
    G = np.zeros((k, k), object)
    Gl = np.zeros((k, k), LD)
    if n == 0:
        return G, Gl
    L = _limbs(M)
    for i in range(3):
        for j in range(3):
            P = L[i].T @ L[j]  # integers below 2^53: exact in any summation order
            G = G + (P.astype(np.int64).astype(object) << (_LIMB * (i + j)))
            Gl = Gl + np.ldexp(P.astype(LD), _LIMB * (i + j))
    return G, Gl


def _colsum(M):
    """Exact column sums of an int64 matrix with |M| < 2^60, as Python ints."""
    hi, lo = M >> 30, M & ((1 << 30) - 1)
    return (hi.sum(axis=0).astype(object) << 30) + lo.sum(axis=0).astype(object)


def _int_scale(w, what):
    """f64 values w -> (Python ints W, s) with w = W * 2^-s exactly."""
    if not np.all(np.isfinite(w)):
        raise ValueError(what + " must be finite")
    ratios = [float(v).as_integer_ratio() for v in np.asarray(w, np.float64)]  # denominators: powers of two
    s = max([d.bit_length() - 1 for _, d in ratios] + [0])
    return [n << (s - (d.bit_length() - 1)) for n, d in ratios], s


def _to_ld(n):
    """Python int -> longdouble, relative error below 2^-62."""
    if n == 0:
        return LD(0)
    sh = max(0, abs(n).bit_length() - 120)
    t = n >> sh
    s, t = (-1, -t) if t < 0 else (1, t)
    mask = (1 << 40) - 1
    v = np.ldexp(LD(float(t >> 80)), 80) + np.ldexp(LD(float((t >> 40) & mask)), 40) + LD(float(t & mask))
    return np.ldexp(s * v, sh)


def _ld_to_ints(y):
    """longdouble vector -> (Python ints Y, q) with y = Y * 2^q exactly."""
    m, e = np.frexp(y)
    hi = np.trunc(np.ldexp(m, 32))
    lo = np.ldexp(m - np.ldexp(hi, -32), 64)  # integer-valued, |lo| < 2^32
    hi, lo, e = hi.astype(np.int64), lo.astype(np.int64), e.astype(np.int64) - 64
    q = int(e[m != 0].min()) if np.any(m != 0) else 0
    return [((int(h) << 32) + int(l)) << max(0, int(ee) - q) for h, l, ee in zip(hi, lo, e)], q


# --------------------------------------------------- longdouble Cholesky
def _cholesky(A):
    """Lower L with L L^T = A, column by column (A symmetric positive definite)."""
    k = A.shape[0]
    L = np.zeros((k, k), LD)
    for j in range(k):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(d)
        if j + 1 < k:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _chol_solve(L, b):
    k = len(b)
    y = np.array(b, LD)
    for j in range(k):  # L w = b
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(k - 1, -1, -1):  # L^T x = w
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def _solve_exact(G, Gl, sw, bint, sc, E, lam):
    """x (longdouble) of (D G D 2^-sw + lam I) x = D bint 2^-sc, D = diag(2^E);
    G / bint exact Python ints, Gl the longdouble image of G. Returns (x,
    A in longdouble, |last refinement step|_inf / |x|_inf)."""
    k = len(E)
    Ei = [int(v) for v in E]
    A = np.ldexp(Gl, (E[:, None] + E[None, :] - sw).astype(np.int64))
    A[np.diag_indices(k)] += LD(lam)
    b = np.array([np.ldexp(_to_ld(bint[i]), Ei[i] - sc) for i in range(k)], LD)
    # exact integer image: A = D At D 2^-T with At = G 2^(T - sw) + diag(lam 2^(T - 2 E))
    lm, le = _int_scale([lam], "lambda")
    T = max([sw] + [2 * v + le for v in Ei])
    At = G << (T - sw)
    for i in range(k):
        At[i, i] = At[i, i] + (lm[0] << (T - 2 * Ei[i] - le))
    L = _cholesky(A)
    x = _chol_solve(L, b)
    step = LD(0)
    for _ in range(2):
        Y, q = _ld_to_ints(np.ldexp(x, E))           # y = D x
        AY = At.dot(np.array(Y, object))
        c = min(-sc, q - T)
        r = np.array([np.ldexp(_to_ld((bint[i] << (-sc - c)) - (AY[i] << (q - T - c))), Ei[i] + c)
                      for i in range(k)], LD)         # b - A x, exact before the rounding to longdouble
        d = _chol_solve(L, r)
        x = x + d
        step = np.abs(d).max() / max(np.abs(x).max(), np.finfo(LD).tiny)
    return x, A, step


def yty_longdouble(src, k):
    """Sum over the rows of src[:, :k] (f32) of y y^T: exact, rounded once to longdouble."""
    M, E = _int_columns(np.asarray(src, np.float32)[:, :k])
    return np.ldexp(_gram(M)[1], (E[:, None] + E[None, :]).astype(np.int64))


def solve_rows(indptr, indices, values, src, k, reg, implicit=False, alpha=0.0, stats=None):
    """(x longdouble [n_rows, k], kappa f64 [n_rows]): per row the solution of
    the normal equations above and numpy.linalg.cond of the f64 image of A
    (1.0 for a row that has no system: no rating, or implicit with none > 0).
    stats (optional dict) receives "last_step": |second refinement step|_inf /
    |x|_inf per row."""
    S = np.asarray(src, np.float32)[:, :k]
    values = np.asarray(values, np.float32)
    M, E = _int_columns(S)
    n_rows = len(indptr) - 1
    x = np.zeros((n_rows, k), LD)
    kappa = np.ones(n_rows)
    last = np.zeros(n_rows)
    if implicit:
        Y, Yl = _gram(M)
    for r in range(n_rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            continue
        rows = M[np.asarray(indices[lo:hi], np.int64)]
        rat = values[lo:hi].astype(np.float64)
        if implicit:
            n_pos = int((rat > 0).sum())
            if n_pos == 0:
                continue
            w = np.float64(alpha) * np.abs(rat)
            W, sw = _int_scale(w, "confidence weights")
            W = np.array(W, object)
            G, Gl = Y << sw, np.ldexp(Yl, sw)
            for wv in sorted(set(W.tolist())):
                if wv:
                    g, gl = _gram(rows[np.array([t == wv for t in W])])
                    G, Gl = G + g * wv, Gl + gl * LD(wv)
            coef = [((1 << sw) + int(t)) if p else 0 for t, p in zip(W, rat > 0)]
            sc = sw
            lam = np.float64(n_pos) * np.float64(reg)
        else:
            G, Gl = _gram(rows)
            sw = 0
            coef, sc = _int_scale(rat, "ratings")
            lam = np.float64(hi - lo) * np.float64(reg)
        bint = np.zeros(k, object)
        for cv in set(coef):
            if cv:
                bint = bint + _colsum(rows[np.array([t == cv for t in coef])]) * cv
        x[r], A, last[r] = _solve_exact(G, Gl, sw, bint, sc, E, lam)
        kappa[r] = np.linalg.cond(A.astype(np.float64))
    if stats is not None:
        stats["last_step"] = last
    return x, kappa


# ---------------------------------------------------------------- families
# name -> (reg, what the sources are)
FAMILIES = {
    "gauss": 0.1,        # N(0, 1): the data of the other ALS tests (control)
    "corr2": 1e-3,       # u + 1e-2 z: strongly correlated factor rows
    "corr3": 1e-7,       # u + 1e-3 z
    "corr4": 1e-9,       # u + 1e-4 z
    "short8": 1e-8,      # N(0, 1) with a tiny reg: rows shorter than k carry the conditioning
    "scaled_up": 0.1,    # N(0, 1) * 2^10
    "scaled_down": 0.1,  # N(0, 1) * 2^-10, ratings * 2^-6
    "graded": 1e-3,      # column c scaled by 2^(-c / 4)
}
KKP_SMALL = [(8, 16), (16, 16), (20, 32), (32, 32), (50, 64), (64, 64)]  # one wave per row
KKP_WIDE = [(65, 96), (128, 128), (200, 256), (256, 256)]               # one workgroup per row
KKP_IMPLICIT = [(10, 16), (16, 16), (20, 32), (33, 64), (64, 64)]       # test_gpu_als_implicit's
ALPHAS = [1.0, 40.0]
HALF_STEPS = np.arange(1, 11, dtype=np.float32) * np.float32(0.5)  # 0.5 .. 5.0
NONPOS_ROW = 2  # the row of three ratings: all negative or zero


def row_lengths(k, kp):
    if kp > 64:  # one workgroup per row and a k^3 host reference: six rows
        return [0, 1, k // 2, k - 1, k + 1, 3 * k]
    base = [0, 1, 3, k // 2, k - 1, k, k + 1, 3 * k]
    return base + [64, 65, 257] if kp == 64 else base


def family(name, k, kp, rng):
    """(indptr, indices, values, src) of one family: src [n_src, kp] f32 with
    zero padding columns; row NONPOS_ROW (kp <= 64) holds negative and zero
    ratings only; rows of 3 or more ratings use the first and the last
    source row."""
    deg = row_lengths(k, kp)
    n_src = max(deg) + 5
    z = rng.normal(size=(n_src, k))
    if name.startswith("corr"):
        body = rng.normal(size=k)[None, :] + 10.0 ** -int(name[4:]) * z
    elif name == "scaled_up":
        body = z * 2.0 ** 10
    elif name == "scaled_down":
        body = z * 2.0 ** -10
    elif name == "graded":
        body = z * 2.0 ** (-np.arange(k) / 4.0)[None, :]
    elif name in ("gauss", "short8"):
        body = z
    else:
        raise KeyError(name)
    src = np.zeros((n_src, kp), np.float32)
    src[:, :k] = body.astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.zeros(indptr[-1], np.int32)
    values = rng.choice(HALF_STEPS, indptr[-1]).astype(np.float32)
    for r, n in enumerate(deg):
        lo = indptr[r]
        if n >= 3:
            indices[lo:lo + n] = 1 + rng.choice(n_src - 2, n, replace=False)
            indices[lo], indices[lo + n - 1] = n_src - 1, 0
        elif n:
            indices[lo:lo + n] = rng.choice(n_src, n, replace=False)
        if r == NONPOS_ROW and kp <= 64:
            values[lo:lo + 3] = np.array([-2.0, 0.0, -0.5], np.float32)
    if kp > 64:  # no row of three here: the last row takes a negative and a zero rating
        values[indptr[-1] - 2:] = np.array([-1.5, 0.0], np.float32)
    if name == "scaled_down":
        values *= np.float32(2.0 ** -6)
    return indptr, indices, values, src


def family_seed(name, k):
    return 1000 * sorted(FAMILIES).index(name) + k


_cache = {}


def family_reference(name, k, kp, implicit=False, alpha=0.0):
    """The family's problem with its reference, computed once per process and
    shared read-only: dict(problem, reg, x, kappa, last_step)."""
    key = (name, k, kp, implicit, float(alpha))
    if key not in _cache:
        prob = family(name, k, kp, np.random.default_rng(family_seed(name, k)))
        st = {}
        x, kappa = solve_rows(*prob, k, FAMILIES[name], implicit=implicit, alpha=alpha, stats=st)
        for a in prob + (x, kappa):
            a.setflags(write=False)
        _cache[key] = {"problem": prob, "reg": FAMILIES[name], "x": x, "kappa": kappa, "last_step": st["last_step"]}
    return _cache[key]


# ------------------------------------------------------------ error measure
U53 = 2.0 ** -53
MODE1_UNIT = 16 * 2.0 ** -24  # accum_mode 1: relative perturbation of a Gramian summed in f32 chunks of 16 ratings
# accum_mode 1 runs on the families up to corr2 whose kappa * MODE1_UNIT stays below 2^-10
# (test_als_exact.test_mode1_families_are_those_inside_its_documented_limit: corr2 is beyond it)
MODE1_FAMILIES = ("gauss",)
F32_TERM = 2.0 ** -24 * (1.0 + 2.0 ** -20)


def rho(got, x, kappa, unit=U53):
    """Per row max_i (|got_i - x_i| - 2^-24 |x_i|)_+ / (kappa unit |x|_inf);
    0 for a row whose reference is all zero."""
    got, x = np.asarray(got, LD), np.asarray(x, LD)
    N = np.abs(x).max(axis=1)
    excess = np.maximum(np.abs(got - x) - LD(2.0 ** -24) * np.abs(x), 0).max(axis=1)
    den = np.asarray(kappa, LD) * LD(unit) * N
    return np.where(N > 0, excess / np.where(N > 0, den, 1), 0).astype(np.float64)


def bound(x, kappa, rho_max, unit=U53):
    """2^-24 (1 + 2^-20) |x_i| + rho_max kappa unit |x|_inf, per component."""
    x = np.asarray(x, LD)
    N = np.abs(x).max(axis=1, keepdims=True)
    return LD(F32_TERM) * np.abs(x) + LD(rho_max) * np.asarray(kappa, LD)[:, None] * LD(unit) * N


# ---------------------------------------------- exactly singular rows (reg 0)
def singular_problem(k, kp, rng):
    """reg = 0: rows 0..2 have 2k+ independent Gaussian ratings (definite);
    row 3 is a single rating and row 4 two ratings of ONE source row whose
    entries are in {0, 1, 2}: Gramians v v^T and 2 v v^T, exactly singular
    and exactly representable. Returns (problem, singular row numbers)."""
    deg = [2 * k + 3, 3 * k, 2 * k, 1, 2]
    n_src = 3 * k + 2
    src = np.zeros((n_src, kp), np.float32)
    src[:, :k] = rng.normal(size=(n_src, k)).astype(np.float32)
    src[n_src - 1, :k] = np.array([2, 1, 0, 1, 2, 2, 0, 1], np.float32)[np.arange(k) % 8]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = np.zeros(indptr[-1], np.int32)
    for r in range(3):
        indices[indptr[r]:indptr[r + 1]] = rng.choice(n_src - 1, deg[r], replace=False)
    indices[indptr[3]:] = n_src - 1
    values = rng.choice(HALF_STEPS, indptr[-1]).astype(np.float32)
    return (indptr, indices, values, src), [3, 4]
