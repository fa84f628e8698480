"""f64 numpy restatement of Spark 3.5 mllib.optimization.NNLS.solve as
ml.recommendation.ALS.NNLSSolver calls it (the checker of the non-negative
ALS tests): projected gradients with conjugate-gradient directions on the
normal equations of a destination row,
  explicit: A = sum v v^T + reg n I,             b = sum r v
  implicit: A = YtY + sum c1 v v^T + reg n_pos I, b = sum_{r > 0} (1 + c1) v,
x from 0, at most max(400, 20 n) iterations, rounded to f32.

`perm` reorders the terms of every dot product and matrix-vector product (a
second faithful summation order; None = the natural order). The second half
of the file holds the problem families on which the iteration branches (stop
rules, the cap, multi-entry wall steps) and what the tests pin of them."""
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


def solve(A, b, perm=None, max_iter=None, events=None):
    """(x f64 [n], iterations that moved x). max_iter caps the loop below
    iter_max(n) (the iterate after that many steps). events (a dict) receives
    "stop": the rule that ended the loop, in the order Spark tests them (nan,
    small: step < 1e-7, big: step > 1e40, rel: ndir < 1e-12 nx, abs: ndir <
    1e-32), cap at iter_max(n), or max_iter; "rejected": CG steps tried and
    rejected; "walls": steps that set an entry to zero; "multi": steps that
    set two or more entries with x > 0 to zero."""
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

    def why(step, ndir, nx):
        return ("nan" if np.isnan(step) else "small" if step < 1e-7 else "big" if step > 1e40 else
                "rel" if ndir < 1e-12 * nx else "abs")

    limit = iter_max(n) if max_iter is None else min(int(max_iter), iter_max(n))
    ev = {"stop": None, "rejected": 0, "walls": 0, "multi": 0}
    x = np.zeros(n)
    last_dir = np.zeros(n)
    last_norm = np.float64(0.0)
    last_wall = 0
    iterno = 0
    with np.errstate(all="ignore"):
        while iterno < limit:
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
                    ev["rejected"] += 1
                    direc = grad
                    ndir = dot(direc, direc)
                else:
                    step = dstep
            else:
                ndir = dot(direc, direc)
            if stop(step, ndir, nx):
                ev["stop"] = why(step, ndir, nx)
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
                ev["walls"] += 1
                ev["multi"] += int((hit & (x > 0)).sum() >= 2)
            x = np.where(hit, 0.0, x - step * direc)
            last_dir = direc
            last_norm = ngrad
            iterno += 1
    if events is not None:
        if ev["stop"] is None:
            ev["stop"] = "cap" if iterno == iter_max(n) else "max_iter"
        events.update(ev)
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


# ----------------------------------------- where the iteration branches
# The families of the conditioning tests (tests/test_gpu_als_nonneg_conditioning.py, checked on
# the CPU in tests/test_nnls_oracle.py): those of als_exact plus two of gauss.
STABLE = ("gauss", "graded", "short8", "scaled_up", "scaled_down", "tiny", "ties")
CHAOTIC = ("corr2", "corr3")  # explicit, at CHAOTIC_K
CHAOTIC_K = (10, 33, 64)
MODES = [(False, 0.0), (True, 1.0), (True, 40.0)]  # (implicit, alpha)


def hard_problem(name, k, kp):
    """((indptr, indices, values, src), reg) of one family."""
    import als_exact as ax

    base = name if name in ax.FAMILIES else "gauss"
    indptr, indices, values, src = ax.family(base, k, kp, np.random.default_rng(ax.family_seed(base, k)))
    if name in ax.FAMILIES:
        return (indptr, indices, values, src), ax.FAMILIES[name]
    if name == "tiny":  # the 1e-20 guard of the step length dominates
        values = values * np.float32(2.0 ** -40)
        src = src * np.float32(2.0 ** -40)
    elif name == "ties":  # duplicated source columns: entries reach the bound together
        for c in range(0, k - 1, 4):
            src[:, c + 1] = src[:, c]
        values[::3] *= -1
    else:
        raise KeyError(name)
    return (indptr, indices, values, src), 0.1


def orders(k, kp):
    """Six faithful summation orders: natural, reversed, the kernel's lane
    order, three random permutations."""
    lane = [(q % 16) * (kp // 16) + q // 16 for q in range(kp)]
    rng = np.random.default_rng(3)
    return [None, np.arange(k)[::-1].copy(), np.array([c for c in lane if c < k])] + \
        [rng.permutation(k) for _ in range(3)]


def hard_cases():
    """(name, k, kp, implicit, alpha) of every case: the stable families in
    three modes (graded explicit only: its implicit rows at k >= 33 are
    unstable), the chaotic ones explicit at CHAOTIC_K."""
    out = [(name, k, kp, imp, alpha) for name in STABLE for k, kp in KKP for imp, alpha in MODES
           if not (imp and name == "graded")]
    return out + [(name, k, kp, False, 0.0) for name in CHAOTIC for k, kp in KKP if k in CHAOTIC_K]


def objective(A, b, x):
    """x^T A x / 2 - b^T x in longdouble."""
    A, b, x = (np.asarray(a, np.float64).astype(np.longdouble) for a in (A, b, x))
    return x @ (A @ x) / 2 - b @ x


X32_ITERS = 32  # the iterate that bounds the objective of an unstable row from above


@functools.lru_cache(maxsize=None)
def hard_reference(name, k, kp, implicit, alpha):
    """The case in the natural order, computed once per process and shared
    read-only: dict(problem, reg, eqs, exp [rows, k] f32, iters, events [per
    row: dict or None], x32 [rows, k] f64: the iterate after X32_ITERS steps)."""
    prob, reg = hard_problem(name, k, kp)
    eqs = normal_equations(*prob, k, reg, implicit, alpha)
    n = len(eqs)
    exp, x32 = np.zeros((n, k), np.float32), np.zeros((n, k))
    iters = np.zeros(n, np.int32)
    events = [None] * n
    for r, eq in enumerate(eqs):
        if eq is not None:
            events[r] = {}
            x, iters[r] = solve(*eq, events=events[r])
            exp[r] = x.astype(np.float32)
            x32[r] = x if iters[r] <= X32_ITERS else solve(*eq, max_iter=X32_ITERS)[0]
    for a in prob + (exp, x32, iters):
        a.setflags(write=False)
    return {"problem": prob, "reg": reg, "eqs": eqs, "exp": exp, "iters": iters, "events": events, "x32": x32}


# What tests/test_nnls_oracle.py pins of these cases over the six orders (the GPU test relies on it).
_MODE_KEYS = {(False, 0.0): "explicit", (True, 1.0): "implicit1", (True, 40.0): "implicit40"}
# rows on which the six orders disagree by more than 1e-6 max|row| (stable families)
UNSTABLE_ROWS = {("short8", 64, "explicit"): (3,), ("scaled_up", 10, "explicit"): (3,)}
# rows that run to iter_max(k) in all six orders
_TINY_CAP = {10: (1, 3, 4, 5, 6, 7), 16: (1, 3, 4, 5, 6, 7), 20: (1, 3, 4, 5, 6, 7),
             33: (1, 3, 4, 5, 6, 7, 8, 9, 10), 64: (1, 3, 4, 5, 6, 7, 8, 9)}  # k 64: row 10 stops on step < 1e-7
CAP_ROWS = {("short8", 64, "explicit"): (3,),
            ("corr2", 10, "explicit"): (), ("corr2", 33, "explicit"): (8,), ("corr2", 64, "explicit"): (4,),
            ("corr3", 10, "explicit"): (), ("corr3", 33, "explicit"): (3, 4, 5, 6, 7, 8, 10),
            ("corr3", 64, "explicit"): (3, 4, 5, 6, 7, 8, 9, 10)}
CAP_ROWS.update({("tiny", k, m): rows for k, rows in _TINY_CAP.items() for m in ("implicit1", "implicit40")})


def mode_key(implicit, alpha):
    return _MODE_KEYS[(bool(implicit), float(alpha))]


def cap_rows(name, k, implicit, alpha):
    return CAP_ROWS.get((name, k, mode_key(implicit, alpha)), ())


def unstable_rows(name, k, kp, implicit, alpha):
    """The rows of a case that are compared through invariants only: the
    pinned ones of the stable families; of a chaotic case every solved row
    with more than one rating (a single rating is one exact step in any
    order)."""
    if name in CHAOTIC:
        ref = hard_reference(name, k, kp, implicit, alpha)
        deg = np.diff(ref["problem"][0])
        return tuple(r for r, eq in enumerate(ref["eqs"]) if eq is not None and deg[r] > 1)
    return UNSTABLE_ROWS.get((name, k, mode_key(implicit, alpha)), ())
