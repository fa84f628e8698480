"""A numpy oracle of hrec_als_explain's contract (include/hrec.h), written from
its formulas, one kernel row at a time, in two precisions: np.float64 with
np.linalg.solve, and np.longdouble with a hand-written Cholesky. Nothing here
calls the package. Also the generated calls that the GPU test runs (CALLS) and
the gap condition under which their positions may be compared exactly."""
import numpy as np

F64 = np.float64
LD = np.longdouble
GAP = 1e-9  # relative gap between neighbouring top contributions (of max |c|)
FLOOR = 2.0 ** -50


def normal_equations(Y, k, cols, vals, reg, implicit, alpha, yty, dt):
    """(A [k, k], beta [n], eligible [n], y_j [n, k]) of one history in dtype dt."""
    Yh = np.asarray(Y)[np.asarray(cols, np.int64), :k].astype(dt)
    r = np.asarray(vals).astype(dt)
    n = len(r)
    eye = np.eye(k, dtype=dt)
    if implicit:
        c1 = dt(alpha) * np.abs(r)
        elig = r > 0
        beta = np.where(elig, 1 + c1, dt(0)).astype(dt)
        G = np.asarray(yty)[:k, :k].astype(dt) if yty is not None else np.asarray(Y)[:, :k].astype(dt).T @ np.asarray(
            Y)[:, :k].astype(dt)
        A = G + (Yh * c1[:, None]).T @ Yh + dt(reg) * dt(int(elig.sum())) * eye
    else:
        elig = np.ones(n, bool)
        beta = r
        A = Yh.T @ Yh + dt(reg) * dt(n) * eye
    return A, beta, elig, Yh


def cholesky_ld(A):
    """Lower L of A = L L^T in longdouble, or None when a pivot is not positive and finite."""
    k = A.shape[0]
    L = np.zeros((k, k), LD)
    for j in range(k):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not (np.isfinite(d) and d > 0):
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < k:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_ld(L, B):
    k = L.shape[0]
    Z = np.array(B, dtype=LD)
    for j in range(k):
        Z[j] = (Z[j] - L[j, :j] @ Z[:j]) / L[j, j]
    for j in range(k - 1, -1, -1):
        Z[j] = (Z[j] - L[j + 1:, j] @ Z[j + 1:]) / L[j, j]
    return Z


def solve(A, B, dt):
    """A^-1 B, or None when the factorisation is not usable."""
    if dt is LD:
        L = cholesky_ld(A)
        return None if L is None else solve_ld(L, B)
    if not np.isfinite(A).all():
        return None
    try:
        np.linalg.cholesky(A)  # the usability test only
        X = np.linalg.solve(A, np.asarray(B, F64))
    except np.linalg.LinAlgError:
        return None
    return X if np.isfinite(X).all() else None


class Row:
    """One kernel row: c [m, n] (NaN rows: invalid list entries), eligible [n],
    x [k] = A^-1 b (None: nothing to explain), ok."""

    def __init__(self, c, elig, x, ok):
        self.c, self.elig, self.x, self.ok = c, elig, x, ok

    def total(self):
        m = self.c.shape[0]
        if not self.ok:
            return np.full(m, np.nan)
        return self.c[:, self.elig].sum(axis=1)


def explain_row(Y, k, cols, vals, entries, reg, implicit, alpha, yty=None, dt=F64):
    """entries: the list's columns (invalid ones included; they give NaN rows)."""
    Y = np.asarray(Y)
    n_items = Y.shape[0]
    entries = np.asarray(entries, np.int64)
    m, n = len(entries), len(cols)
    blank = Row(np.full((m, n), np.nan, dt), np.zeros(n, bool), None, False)
    if n == 0:
        return blank
    A, beta, elig, Yh = normal_equations(Y, k, cols, vals, reg, implicit, alpha, yty, dt)
    if not elig.any():
        return blank
    valid = (entries >= 0) & (entries < n_items)
    Yi = Y[np.where(valid, entries, 0), :k].astype(dt)
    sol = solve(A, np.concatenate([Yi.T, (Yh.T @ beta)[:, None]], axis=1), dt)
    if sol is None:
        return blank
    W, x = sol[:, :m], sol[:, m]
    c = (W.T @ Yh.T) * beta[None, :]
    c[~valid] = np.nan
    return Row(c, elig, x, True)


def top_lists(row, top_m):
    """(pos [m, top_m] (-1 filled), val, len) of a Row: the largest eligible
    contributions, descending, equal values: the earlier position."""
    m, n = row.c.shape
    pos = np.full((m, top_m), -1, np.int32)
    val = np.full((m, top_m), np.nan, row.c.dtype)
    ln = np.zeros(m, np.int32)
    if not row.ok:
        return pos, val, ln
    idx = np.nonzero(row.elig)[0]
    for i in range(m):
        if np.isnan(row.c[i]).all():
            continue
        ci = row.c[i, idx]
        order = np.lexsort((idx, -ci))[:top_m]
        ln[i] = len(order)
        pos[i, :len(order)] = idx[order]
        val[i, :len(order)] = ci[order]
    return pos, val, ln


def gaps_ok(row, top_m):
    """The first top_m + 1 ranks of every valid entry differ pairwise by more than GAP * max |c|."""
    if not row.ok:
        return True
    pos, val, ln = top_lists(row, top_m + 1)
    for i in range(row.c.shape[0]):
        if ln[i] < 2:
            continue
        v = val[i, :ln[i]]
        scale = np.abs(row.c[i, row.elig]).max()
        if not (np.abs(np.diff(v)) > GAP * scale).all():  # sorted: neighbours are the closest pairs
            return False
    return True


# ------------------------------------------------------------ generated calls
N_ITEMS = 200
REG = 0.1
HIST_LENGTHS = (1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 128, 129, 200)
RANKS = ((10, 16), (16, 16), (20, 32), (50, 64), (64, 64))


class Call:
    """The operands of one hrec_als_explain call, as numpy arrays."""

    def __init__(self, name, k, kp, implicit, alpha, seed, lengths, hist_rows, list_n, top_m, ragged=True,
                 bad_entries=False, nonpos_segment=None):
        rng = np.random.default_rng(seed)
        self.name, self.k, self.kp, self.implicit, self.alpha, self.reg = name, k, kp, implicit, alpha, REG
        self.top_m, self.list_n = top_m, list_n
        self.Y = np.zeros((N_ITEMS, kp), np.float32)
        self.Y[:, :k] = rng.standard_normal((N_ITEMS, k)).astype(np.float32)
        self.indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        # distinct items per segment (a repeated item with the same rating would tie), continuous ratings
        self.cols = np.concatenate([rng.permutation(N_ITEMS)[:n] for n in lengths] + [[]]).astype(np.int32)
        if implicit:  # about a quarter <= 0: ineligible entries
            vals = rng.uniform(0.5, 5.0, self.cols.size) * np.where(rng.random(self.cols.size) < 0.25, -1.0, 1.0)
            for s in range(len(lengths)):  # a segment keeps a positive rating
                if lengths[s] and not (vals[self.indptr[s]:self.indptr[s + 1]] > 0).any():
                    vals[self.indptr[s]] = abs(vals[self.indptr[s]])
            if nonpos_segment is not None:
                seg = slice(self.indptr[nonpos_segment], self.indptr[nonpos_segment + 1])
                vals[seg] = -np.abs(vals[seg])
                vals[self.indptr[nonpos_segment]] = 0.0
        else:
            vals = rng.uniform(0.5, 5.0, self.cols.size) * np.where(rng.random(self.cols.size) < 0.25, -1.0, 1.0)
        self.vals = vals.astype(np.float32)
        self.hist_rows = np.asarray(hist_rows, np.int64)
        n_rows = len(self.hist_rows)
        self.lists = rng.integers(0, N_ITEMS, (n_rows, list_n)).astype(np.int64)
        if bad_entries and list_n:
            self.lists[::3, 0] = -1
            self.lists[1::3, list_n - 1] = N_ITEMS
            self.lists[2::5, list_n // 2] = -7
        self.list_len = rng.integers(0, list_n + 1, n_rows).astype(np.int32) if ragged and n_rows else None
        if self.list_len is not None and n_rows:
            self.list_len[0] = list_n  # one full row at the least
            if n_rows > 2:
                self.list_len[2] = list_n + 5  # longer than the matrix: clipped

    def row_len(self, r):
        return self.list_n if self.list_len is None else int(min(max(self.list_len[r], 0), self.list_n))

    def row_entries(self, r):
        """Row r's list with the entries past its length turned invalid."""
        e = self.lists[r].copy()
        e[self.row_len(r):] = -1
        return e

    def segment(self, r):
        q = int(self.hist_rows[r])
        if q < 0:
            return np.zeros(0, np.int32), np.zeros(0, np.float32)
        return self.cols[self.indptr[q]:self.indptr[q + 1]], self.vals[self.indptr[q]:self.indptr[q + 1]]

    def oracle_row(self, r, dt, yty=None):
        cols, vals = self.segment(r)
        return explain_row(self.Y, self.k, cols, vals, self.row_entries(r), self.reg, self.implicit, self.alpha,
                           yty=yty, dt=dt)


def _calls():
    out = []
    seed = 1000
    every = list(range(len(HIST_LENGTHS)))
    for k, kp in RANKS:  # every history length at every rank, both models
        for imp in (0, 1):
            seed += 1
            out.append(Call("len-k%d-kp%d-%s" % (k, kp, "imp" if imp else "exp"), k, kp, imp, 0.5 * imp, seed,
                            HIST_LENGTHS, every, 17, 5))
    for list_n in (1, 16, 17, 33):  # the group of 16 entries and its neighbours
        for top_m in (1, 5, 32):  # 32 > the 3-entry history: out_len is the history length
            for imp in (0, 1):
                seed += 1
                out.append(Call("list%d-top%d-%s" % (list_n, top_m, "imp" if imp else "exp"), 20, 32, imp, 2.0 * imp,
                                seed, (3, 65, 129), (0, 1, 2, 1), list_n, top_m))
    for imp in (0, 1):  # more rows than resident waves; shared segments, no history, bad entries
        seed += 1
        lengths = (5, 40, 64, 7, 130, 1, 9)
        rows = [(-1 if r % 11 == 4 else r % len(lengths)) for r in range(300)]
        out.append(Call("rows300-%s" % ("imp" if imp else "exp"), 10, 16, imp, 1.0 * imp, seed, lengths, rows, 3, 5,
                        bad_entries=True, nonpos_segment=3 if imp else None))
    seed += 1
    out.append(Call("one-row", 50, 64, 0, 0.0, seed, (70,), (0,), 2, 5, ragged=False))
    seed += 1
    out.append(Call("alpha0", 16, 16, 1, 0.0, seed, (33, 2), (0, 1), 4, 5, ragged=False))
    return out


CALLS = _calls()
