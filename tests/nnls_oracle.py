"""f64 numpy restatement of Spark 3.5 mllib.optimization.NNLS.solve as
ml.recommendation.ALS.NNLSSolver calls it (the checker of the non-negative
ALS tests): projected gradients with conjugate-gradient directions on the
normal equations of a destination row,
  explicit: A = sum v v^T + reg n I,             b = sum r v
  implicit: A = YtY + sum c1 v v^T + reg n_pos I, b = sum_{r > 0} (1 + c1) v,
x from 0, at most max(400, 20 n) iterations, rounded to f32.

`perm` reorders the terms of every dot product and matrix-vector product (a
second faithful summation order; None = the natural order)."""
import functools

import numpy as np

from implicit_oracle import coo_to_csr, gramian  # noqa: F401  (re-exported)


DEG = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, 6, 6]
KKP = [(10, 16), (16, 16), (20, 32), (33, 64), (64, 64)]
RATINGS = np.array([-2, -0.5, 0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5, 5], np.float32)
ROW_NONPOS, ROW_DUP = len(DEG) - 2, len(DEG) - 1


def sweep_problem(k, kp, signed):
    """The row problems of the half-sweep tests: (indptr, indices, values, src
    [n_src, kp] f32). signed: Gaussian sources and ratings of both signs
    (about half of a row's entries end at the bound); else |Gaussian| sources
    and positive ratings (long rows have no active bound). Row ROW_NONPOS has
    no rating > 0 (all < 0 when not signed: with sources >= 0 its explicit b
    is <= 0), row ROW_DUP duplicate column entries."""
    rng = np.random.default_rng(100 + k + (0 if signed else 1000))
    n_src = max(2 * k, 140)
    indptr = np.concatenate([[0], np.cumsum(DEG)]).astype(np.int64)
    indices = rng.integers(0, n_src, indptr[-1]).astype(np.int32)
    indices[::7] = n_src - 1
    indices[3::11] = 0
    values = rng.choice(RATINGS if signed else RATINGS[3:], indptr[-1]).astype(np.float32)
    r = ROW_NONPOS
    values[indptr[r]: indptr[r + 1]] = np.array([-2, -0.5, 0, 0, -2, -0.5] if signed else
                                                [-2, -0.5, -1, -3, -2, -0.5], np.float32)
    r = ROW_DUP
    indices[indptr[r]: indptr[r + 1]] = np.array([5, 5, 9, 5, 9, 11], np.int32)
    values[indptr[r]: indptr[r + 1]] = np.array([1, 3, -2 if signed else 2, 1, 0.5, 4], np.float32)
    src = np.zeros((n_src, kp), np.float32)
    g = rng.normal(size=(n_src, k)) / np.sqrt(k)
    src[:, :k] = (g if signed else np.abs(g)).astype(np.float32)
    return indptr, indices, values, src


def iter_max(n):
    return max(400, 20 * n)


def solve(A, b, perm=None):
    """(x f64 [n], iterations that moved x)."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    n = len(b)
    if perm is None:
        def mv(v):
            return A @ v

        def dot(u, v):
            return np.float64(u @ v)
    else:
        Ap = np.ascontiguousarray(A[:, perm])

        def mv(v):
            return Ap @ v[perm]

        def dot(u, v):
            return np.float64(u[perm] @ v[perm])

    def steplen(d, res):
        return dot(d, res) / (dot(mv(d), d) + 1e-20)

    def stop(step, ndir, nx):
        return bool(np.isnan(step) or step < 1e-7 or step > 1e40 or ndir < 1e-12 * nx or ndir < 1e-32)

    x = np.zeros(n)
    last_dir = np.zeros(n)
    last_norm = np.float64(0.0)
    last_wall = 0
    iterno = 0
    with np.errstate(all="ignore"):
        while iterno < iter_max(n):
            res = mv(x) - b
            grad = res.copy()
            grad[(grad > 0) & (x == 0)] = 0.0
            ngrad = dot(grad, grad)
            direc = grad
            step = steplen(grad, res)
            nx = dot(x, x)
            if iterno > last_wall + 1:
                direc = grad + (ngrad / last_norm) * last_dir
                dstep = steplen(direc, res)
                ndir = dot(direc, direc)
                if stop(dstep, ndir, nx):  # reject the CG step
                    direc = grad
                    ndir = dot(direc, direc)
                else:
                    step = dstep
            else:
                ndir = dot(direc, direc)
            if stop(step, ndir, nx):
                break
            # don't cross a wall: Spark's loop over i ascending with its shrinking step. An entry
            # that fails the test against the first step fails it against every smaller one, so
            # only those that pass it are walked.
            for i in np.flatnonzero(step * direc > x):
                if step * direc[i] > x[i]:
                    step = x[i] / direc[i]
            hit = step * direc > x * (1 - 1e-14)
            if hit.any():
                last_wall = iterno
            x = np.where(hit, 0.0, x - step * direc)
            last_dir = direc
            last_norm = ngrad
            iterno += 1
    return x, iterno


def normal_equations(indptr, indices, values, src, k, reg, implicit=False, alpha=0.0, yty=None):
    """[(A, b) or None per row] in f64; None for a row that is not solved (no
    ratings; implicit: no rating > 0)."""
    s = np.asarray(src, np.float64)[:, :k]
    if implicit:
        yty = gramian(s) if yty is None else np.asarray(yty, np.float64)[:k, :k]
    out = []
    for r in range(len(indptr) - 1):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            out.append(None)
            continue
        V = s[indices[lo:hi]]
        rating = np.asarray(values[lo:hi], np.float64)
        if implicit:
            c1 = alpha * np.abs(rating)
            A = yty + (V * c1[:, None]).T @ V
            b = ((1.0 + c1) * (rating > 0)) @ V
            n = int((rating > 0).sum())
        else:
            A = V.T @ V
            b = rating @ V
            n = hi - lo
        if n == 0:
            out.append(None)
            continue
        A[np.diag_indices(k)] += reg * n
        out.append((A, b))
    return out


def half_sweep(indptr, indices, values, src, k, reg, implicit=False, alpha=0.0, yty=None, perm=None,
               return_iters=False):
    """src [n_src, >= k] f32 -> [n_rows, k] f32 (and int32 iterations per row)."""
    eqs = normal_equations(indptr, indices, values, src, k, reg, implicit, alpha, yty)
    out = np.zeros((len(eqs), k), np.float32)
    iters = np.zeros(len(eqs), np.int32)
    for r, eq in enumerate(eqs):
        if eq is not None:
            x, iters[r] = solve(eq[0], eq[1], perm)
            out[r] = x.astype(np.float32)
    return (out, iters) if return_iters else out


def fit(user_csr, item_csc, U0, k, reg, iters, implicit=False, alpha=0.0, perm=None):
    """Items from users, then users from items; (U, V) f32."""
    U = np.asarray(U0, np.float32)[:, :k].copy()
    V = None
    for _ in range(iters):
        V = half_sweep(*item_csc, U, k, reg, implicit, alpha, perm=perm)
        U = half_sweep(*user_csr, V, k, reg, implicit, alpha, perm=perm)
    return U, V


@functools.lru_cache(maxsize=None)
def synthetic_fit(n_users, n_items, dens, k, implicit, alpha, reg=0.1, iters=3):
    """The engine-fit case of the tests on the host, computed once per process
    and shared (do not modify the arrays): (user CSR, item CSC, U0, U, V) from
    the synthetic ratings and the counter-based initial factors that
    DeviceALS.init_user_factors(synthetic.SEED_INIT) produces on the device."""
    from oracle import build as obuild
    from oracle import synth as osyn
    from src import synthetic

    ucsr = obuild.synth_csr(n_users, n_items, dens, 0, 0, n_users, synthetic.SEED, synthetic.SEED2)
    icsc = obuild.synth_csr(n_users, n_items, dens, 1, 0, n_items, synthetic.SEED, synthetic.SEED2)
    U0 = osyn.init_factors(synthetic.SEED_INIT, 0, n_users, k)
    U, V = fit(ucsr, icsc, U0, k, reg, iters, implicit, alpha)
    return ucsr, icsc, U0, U, V
