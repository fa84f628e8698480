"""GPU: hrec_dot_topk_excluding (csrc/dot_topk.hip) — hrec_dot_topk over the
items a query has not seen.

The expected result is built from the device's own full score matrix
(hrec_dot_scores): numpy argsort(-scores, kind="stable") of each row, the
query's excluded items deleted, the first kk = min(top_k, N) kept; the length
is min(kk, N - distinct in-range excluded columns). Ids, score BITS and lengths
are compared exactly (the convention of tests/test_gpu_dot.py): nothing here
has a tolerance.

Shapes: N 300 / 16384 (the small path; 16384 is its last catalogue), 16385
(the first sampled one: S = 8192, step 2, the last item outside the sample),
20000 / 70000 (sampled); B 3 (GEMV filter, f32), 5 / 130 (resident-user
kernel), 20 at f32 d = 256 (tile kernel); bf16 at dk 64 / 256, f32 at dk 32
and at d = 50 padded to 64; top_k 1 / 10 / 64 / 65 / 100 (cap and sample
formula change at 65) and kk = min(top_k, N) with N = 40.

Every shape runs twice: with the exclusion patterns that keep a bound, where
one call of the library entry must answer without overflow (so the lists
compared are the fused path's own), and with the patterns that leave none,
which overflow on the sampled path and end in the binding's fallback. A third
test makes the refinement round carry a result.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PATTERNS = 8


def _h():
    from src import _hrec

    return _hrec


def _vecs(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def _sample(N, kk):
    """(S, step) of hrec_dot_topk's strided sample (dot_cap / dot_sample)."""
    cap = 8192 if kk <= 64 else 128 * kk
    if N <= 16384:
        return N, 1
    S = min(N, max(8192, -(-4 * kk * N // cap)))
    return S, N // S


def _cap(kk):
    return 8192 if kk <= 64 else 128 * kk


def _patterns(B, N, kk, order, seed, patterns=range(N_PATTERNS), tie=None):
    """One exclusion column list per query (None: the empty set given as a
    negative excl_rows entry), the patterns cycled over the queries."""
    g = np.random.default_rng(seed)
    S, step = _sample(N, kk)
    pats = list(patterns)
    out = []
    for b in range(B):
        p = pats[b % len(pats)]
        if p == 0:
            cols = None
        elif p == 1:    # the query's own unfiltered top-kk
            cols = np.sort(order[b, :kk])
        elif p == 2:    # a random 30 %
            cols = np.flatnonzero(g.random(N) < 0.3)
        elif p == 3:    # every sample item but three: no bound for kk > 3
            samp = np.arange(S, dtype=np.int64) * step
            cols = np.delete(samp, g.choice(S, size=min(3, S), replace=False))
        elif p == 4:    # every item: length 0
            cols = np.arange(N)
        elif p == 5:    # all but three: length 3
            cols = np.delete(np.arange(N), g.choice(N, size=min(3, N), replace=False))
        elif p == 6:    # one member (the smaller index) of a tied pair
            cols = np.array([min(tie[b])]) if tie and b in tie else np.array([int(order[b, 0])])
        else:           # duplicate columns (the query's two best items among them), a negative
                        # column, columns >= n_items
            t0, t1 = int(order[b, 0]), int(order[b, min(1, N - 1)])
            cols = np.sort(np.array([-5, 3, 3, 7, 7, 7, t0, t0, t1, N - 1, N - 1, N, N + 100]))
        out.append(None if cols is None else np.asarray(cols, np.int64))
    return out


def _csr(cols_per_query, device):
    """CSR with the queries' rows in REVERSE order plus one unused row in
    front (excl_rows is an indirection, not the identity); None -> -1."""
    B = len(cols_per_query)
    rows = np.full(B, -1, np.int64)
    indptr, cols = [0, 2], [np.array([1, 2], np.int64)]  # row 0: unused
    for r, b in enumerate(reversed(range(B))):
        c = cols_per_query[b]
        if c is not None:
            rows[b] = r + 1
            cols.append(c)
        indptr.append(indptr[-1] + (0 if c is None else len(c)))
    return (torch.as_tensor(rows, device=device), torch.as_tensor(np.asarray(indptr, np.int64), device=device),
            torch.as_tensor(np.concatenate(cols).astype(np.int32), device=device))


def _expected(scores, order, cols_per_query, kk):
    B, N = scores.shape
    idx = np.zeros((B, kk), np.int64)
    val = np.zeros((B, kk), np.float32)
    lens = np.zeros(B, np.int32)
    for b in range(B):
        c = cols_per_query[b]
        o = order[b]
        if c is not None:
            gone = np.zeros(N, bool)
            gone[c[(c >= 0) & (c < N)]] = True
            o = o[~gone[o]]
        m = min(kk, len(o))
        idx[b, :m], val[b, :m], lens[b] = o[:m], scores[b, o[:m]], m
    return idx, val, lens


def _raw(h, U, V, kk, rows, indptr, cols, thr=None, idx_offset=0, top_k=None):
    """One round of the library entry: (idx, val, lens, overflow flag). top_k
    (default kk) is what the library is given; it cuts it to kk itself."""
    dk, bf = h._dot_args(U, V)
    B, N = U.shape[0], V.shape[0]
    dev = U.device
    oi = torch.empty((B, kk), dtype=torch.int64, device=dev)
    ov = torch.empty((B, kk), dtype=torch.float32, device=dev)
    on = torch.empty(B, dtype=torch.int32, device=dev)
    flag = torch.full((1,), 7, dtype=torch.int32, device=dev)
    need = int(h.lib().hrec_dot_topk_excluding_workspace_bytes(B, N, kk))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    h._check("hrec_dot_topk_excluding", h.lib().hrec_dot_topk_excluding(
        h._vp(U.data_ptr()), B, h._vp(V.data_ptr()), N, dk, bf, kk if top_k is None else int(top_k),
        None if thr is None else h._vp(thr.data_ptr()), int(idx_offset), h._vp(rows.data_ptr()),
        *h._excl_args("test", indptr, cols), h._vp(oi.data_ptr()), h._vp(ov.data_ptr()), h._vp(on.data_ptr()),
        h._vp(flag.data_ptr()), h._vp(ws.data_ptr()), need, h._stream()))
    return oi, ov, on, int(flag.item())


def _assert_lists(got, exp, what=""):
    gi, gv, gn = (t.cpu().numpy() for t in got)
    ei, ev, en = exp
    np.testing.assert_array_equal(gn, en, err_msg=f"{what}: lengths")
    live = np.arange(ei.shape[1])[None, :] < en[:, None]
    np.testing.assert_array_equal(np.where(live, gi, 0), np.where(live, ei, 0), err_msg=f"{what}: ids")
    np.testing.assert_array_equal(np.where(live, gv.view(np.int32), 0), np.where(live, ev.view(np.int32), 0),
                                  err_msg=f"{what}: score bits")


CASES = [
    # N, B, dtype, d, top_ks
    (300, 5, torch.float32, 32, (1, 10, 100)),
    (40, 3, torch.float32, 64, (100,)),              # kk = min(top_k, N) = 40; GEMV scores
    (16384, 130, torch.bfloat16, 64, (10, 65)),      # the last catalogue of the small path
    (16384, 20, torch.float32, 256, (64,)),          # small path, tile kernel scores
    (16385, 5, torch.float32, 64, (1, 10, 64, 65)),  # the first sampled catalogue
    (20000, 3, torch.float32, 128, (10, 100)),       # GEMV filter
    (20000, 130, torch.bfloat16, 256, (10, 64)),     # resident-user kernel, bf16 dk 256
    (70000, 20, torch.float32, 256, (10, 65)),       # tile kernel filter
    (70000, 5, torch.float32, 50, (10,)),            # d = 50 zero-padded to dk 64
    (70000, 130, torch.bfloat16, 64, (100,)),
]
# Patterns whose queries keep a bound (none, own top-kk, random 30 %, tied pair,
# odd columns): the fused path answers in one round. The others (every sample
# item but three, every item, all but three) leave no bound and overflow on
# the sampled path, so they run in calls of their own.
FUSED = (0, 1, 2, 6, 7)
UNBOUNDED = (3, 4, 5, 0)


def _operands(h, device, N, B, dtype, d, pats):
    """Device operands, the device's score matrix, each row's stable order,
    and the tied pairs of the queries that take pattern 6: a second item row
    identical to the query's (host-estimated) best item."""
    U, V = _vecs(B, d, 100 + B), _vecs(N, d, 200 + N % 1000)
    tie = {}
    est = U.astype(np.float64) @ V.astype(np.float64).T
    for i, b in enumerate(b for b in range(B) if pats[b % len(pats)] == 6):
        top, slot = int(np.argmax(est[b])), N - 1 - 7 * i
        if slot != top and slot >= 0:
            V[slot] = V[top]
            tie[b] = (top, slot)
    Ud = h.dot_operand(torch.from_numpy(U).to(device), dtype)
    Vd = h.dot_operand(torch.from_numpy(V).to(device), dtype)
    assert Ud.shape[1] == h.dot_dk(d)
    scores = h.dot_scores(Ud, Vd).cpu().numpy()
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")
    for b, (t0, t1) in tie.items():
        assert scores[b, t0].view(np.int32) == scores[b, t1].view(np.int32)
    return Ud, Vd, scores, order, tie


def _survivors(scores, per_q, kk):
    """Per query, from the device's score matrix: the scores at or above the
    bound the sampled path forms (the kk-th best non-excluded sample score);
    N when fewer than kk sample items are left (no bound)."""
    B, N = scores.shape
    S, step = _sample(N, kk)
    samp = np.arange(S) * step
    out = np.zeros(B, np.int64)
    for b in range(B):
        keep = np.ones(N, bool)
        c = per_q[b]
        if c is not None:
            keep[c[(c >= 0) & (c < N)]] = False
        s = scores[b, samp][keep[samp]]
        out[b] = N if s.size < kk else np.count_nonzero(scores[b] >= np.sort(s)[::-1][kk - 1])
    return out


@pytest.mark.parametrize("N,B,dtype,d,top_ks", CASES)
def test_fused_round_matches_filtered_stable_ranking(device, N, B, dtype, d, top_ks):
    """Queries that keep a bound: ONE call of the library entry, no refinement
    and no fallback, gives the expected ids, score bits and lengths. Before
    the call the host counts each query's survivors from the same score
    matrix; all are within the list cap, so *overflow must be 0 and every list
    is the fused path's own (strided mask, filter, drop, rank)."""
    h = _h()
    Ud, Vd, scores, order, tie = _operands(h, device, N, B, dtype, d, FUSED)
    for top_k in top_ks:
        kk = min(top_k, N)
        per_q = _patterns(B, N, kk, order, seed=7 * N + top_k, patterns=FUSED, tie=tie)
        rows, indptr, cols = _csr(per_q, device)
        exp = _expected(scores, order, per_q, kk)
        if N > 16384:
            counts = _survivors(scores, per_q, kk)
            assert np.all(counts >= exp[2]) and np.all(counts <= _cap(kk)), counts.max()
        got = _raw(h, Ud, Vd, kk, rows, indptr, cols, top_k=top_k)
        assert got[3] == 0
        _assert_lists(got[:3], exp, f"one round, top_k={top_k}")
        got = h.dot_topk_excluding(Ud, Vd, top_k, rows, indptr, cols)
        assert tuple(got[0].shape) == (B, kk)
        _assert_lists(got, exp, f"binding, top_k={top_k}")


@pytest.mark.parametrize("N,B,dtype,d,top_ks", CASES)
def test_queries_without_a_bound(device, N, B, dtype, d, top_ks):
    """Every sample item but three / every item / all but three excluded (and
    one query with nothing excluded). On the small path one call answers. On
    the sampled path these queries admit all N > cap scores: *overflow is 1,
    out_len is still exact (it comes from the exclusion row), and the binding
    answers through its rounds and the materialised chain."""
    h = _h()
    Ud, Vd, scores, order, tie = _operands(h, device, N, B, dtype, d, UNBOUNDED)
    for top_k in top_ks:
        kk = min(top_k, N)
        per_q = _patterns(B, N, kk, order, seed=11 * N + top_k, patterns=UNBOUNDED)
        rows, indptr, cols = _csr(per_q, device)
        exp = _expected(scores, order, per_q, kk)
        ri, rv, rn, flag = _raw(h, Ud, Vd, kk, rows, indptr, cols, top_k=top_k)
        np.testing.assert_array_equal(rn.cpu().numpy(), exp[2], err_msg="out_len comes from the exclusion row")
        if N > 16384:
            assert N > _cap(kk) and flag == 1
        else:
            assert flag == 0
            _assert_lists((ri, rv, rn), exp, f"one round, top_k={top_k}")
        _assert_lists(h.dot_topk_excluding(Ud, Vd, top_k, rows, indptr, cols), exp, f"binding, top_k={top_k}")


@pytest.mark.parametrize("N,B,dtype,d,pats", [
    (16385, 3, torch.float32, 64, (3,)),              # GEMV filter, step 2
    (20000, 5, torch.float32, 64, (3,)),              # resident-user kernel
    (20000, 8, torch.bfloat16, 64, (3, 0, 1, 2)),
    (70000, 20, torch.float32, 256, (3, 0, 1, 2)),    # tile kernel, step 8
    (70000, 5, torch.bfloat16, 256, (3,)),
])
def test_refinement_round_succeeds(device, N, B, dtype, d, pats):
    """Every sample item but three excluded, kk = 10: no bound, so round 1
    admits all N > cap scores and raises *overflow. Its out_val[:, kk - 1] is
    the kk-th best non-excluded entry of a truncated list of real candidates:
    given back as thr_in it must bound the answer from below, and round 2 then
    fits the cap (*overflow 0) and gives the exact lists. The queries of the
    other patterns did not overflow; their out_val[:, kk - 1] is their exact
    kk-th best, an equally valid bound."""
    h = _h()
    kk = 10
    Ud, Vd, scores, order, tie = _operands(h, device, N, B, dtype, d, pats)
    per_q = _patterns(B, N, kk, order, seed=13 * N + B, patterns=pats)
    rows, indptr, cols = _csr(per_q, device)
    exp = _expected(scores, order, per_q, kk)
    assert np.all(exp[2] == kk)
    _, rv, rn, flag = _raw(h, Ud, Vd, kk, rows, indptr, cols)
    assert flag == 1
    np.testing.assert_array_equal(rn.cpu().numpy(), exp[2])
    thr = rv[:, kk - 1].contiguous()
    thr_h = thr.cpu().numpy()
    assert not np.isnan(thr_h).any()
    assert np.all(thr_h <= exp[1][:, kk - 1])  # a lower bound of the kk-th best non-excluded score
    got = _raw(h, Ud, Vd, kk, rows, indptr, cols, thr=thr)
    assert got[3] == 0
    _assert_lists(got[:3], exp, "refinement round")
    _assert_lists(h.dot_topk_excluding(Ud, Vd, kk, rows, indptr, cols), exp, "binding")


@pytest.mark.parametrize("N", [300, 20000])
def test_idx_offset_with_local_columns(device, N):
    h = _h()
    B, d, kk, off = 6, 64, 10, 1_000_000_007
    Ud = torch.from_numpy(_vecs(B, d, 1)).to(device)
    Vd = torch.from_numpy(_vecs(N, d, 2)).to(device)
    scores = h.dot_scores(Ud, Vd).cpu().numpy()
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")
    per_q = _patterns(B, N, kk, order, seed=3, patterns=(0, 1, 2))
    rows, indptr, cols = _csr(per_q, device)
    ei, ev, en = _expected(scores, order, per_q, kk)
    got = h.dot_topk_excluding(Ud, Vd, kk, rows, indptr, cols, idx_offset=off)
    _assert_lists(got, (ei + off, ev, en), "idx_offset")


def test_all_equal_scores_both_rounds_overflow_then_chain(device):
    """One item vector tiled: every score equals the bound, so the filter
    overflows in the first round and, with the k-th best as bound, in the
    second; the materialised chain then returns the first kk non-excluded
    indices."""
    h = _h()
    B, N, d, kk = 5, 20000, 64, 10
    Ud = torch.from_numpy(_vecs(B, d, 5)).to(device)
    Vd = torch.from_numpy(np.tile(_vecs(1, d, 6), (N, 1))).to(device)
    scores = h.dot_scores(Ud, Vd).cpu().numpy()
    assert np.all(scores.view(np.int32) == scores.view(np.int32)[:, :1])
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")
    np.testing.assert_array_equal(order[0], np.arange(N))
    per_q = _patterns(B, N, kk, order, seed=9, patterns=(0, 1, 2))
    rows, indptr, cols = _csr(per_q, device)
    exp = _expected(scores, order, per_q, kk)
    _, rv, rn, flag = _raw(h, Ud, Vd, kk, rows, indptr, cols)
    assert flag == 1
    np.testing.assert_array_equal(rn.cpu().numpy(), exp[2])
    thr = rv[:, kk - 1].contiguous()
    _, _, _, flag2 = _raw(h, Ud, Vd, kk, rows, indptr, cols, thr=thr)
    assert flag2 == 1
    got = h.dot_topk_excluding(Ud, Vd, kk, rows, indptr, cols)
    _assert_lists(got, exp, "chain")
    for b in range(B):  # the first kk indices that are not excluded
        gone = set() if per_q[b] is None else set(per_q[b].tolist())
        first = [j for j in range(3 * kk + int(0.5 * N)) if j not in gone][:kk]
        assert got[0][b].cpu().tolist() == first


def test_designated_case_does_not_overflow(device):
    """N = 20000, f32 d = 64, Gaussian vectors, kk = 10, patterns none / own
    top-kk / random 30 %. The bound of a query is the kk-th best non-excluded
    score among the sample items 0, 2, ..., 16382; the host counts, from the
    same score matrix, the scores at or above it: all within the list cap of
    8192, so *overflow must be 0."""
    h = _h()
    B, N, d, kk = 6, 20000, 64, 10
    assert _sample(N, kk) == (8192, 2) and _cap(kk) == 8192
    Ud = torch.from_numpy(_vecs(B, d, 21)).to(device)
    Vd = torch.from_numpy(_vecs(N, d, 22)).to(device)
    scores = h.dot_scores(Ud, Vd).cpu().numpy()
    order = np.argsort(-scores.astype(np.float64), axis=1, kind="stable")
    per_q = _patterns(B, N, kk, order, seed=23, patterns=(0, 1, 2))
    samp = np.arange(8192) * 2
    for b in range(B):
        keep = np.ones(N, bool)
        if per_q[b] is not None:
            keep[per_q[b]] = False
        s = scores[b, samp][keep[samp]]
        assert s.size >= kk
        bound = np.sort(s)[::-1][kk - 1]
        count = int(np.count_nonzero(scores[b] >= bound))
        assert kk <= count <= 8192, count
    rows, indptr, cols = _csr(per_q, device)
    ri, rv, rn, flag = _raw(h, Ud, Vd, kk, rows, indptr, cols)
    assert flag == 0
    _assert_lists((ri, rv, rn), _expected(scores, order, per_q, kk), "designated")


@pytest.mark.parametrize("N,B,dtype,d", [(300, 5, torch.float32, 32), (20000, 3, torch.float32, 64),
                                         (20000, 130, torch.bfloat16, 64), (30000, 20, torch.float32, 256)])
def test_empty_rows_equal_dot_topk(device, N, B, dtype, d):
    """hrec_dot_topk and the excluding entry with every row empty: the same
    ids and score bits (rows given as -1, and as rows of length 0)."""
    h = _h()
    Ud = h.dot_operand(torch.from_numpy(_vecs(B, d, 31)).to(device), dtype)
    Vd = h.dot_operand(torch.from_numpy(_vecs(N, d, 32)).to(device), dtype)
    for kk in (10, 65):
        bi, bv = h.dot_topk(Ud, Vd, kk)
        none = torch.full((B,), -1, dtype=torch.int64, device=device)
        empty_rows = torch.arange(B, dtype=torch.int64, device=device)
        indptr = torch.zeros(B + 1, dtype=torch.int64, device=device)
        cols = torch.zeros(0, dtype=torch.int32, device=device)
        for rows in (none, empty_rows):
            gi, gv, gn = h.dot_topk_excluding(Ud, Vd, kk, rows, indptr, cols)
            assert gn.cpu().tolist() == [kk] * B
            np.testing.assert_array_equal(gi.cpu().numpy(), bi.cpu().numpy())
            np.testing.assert_array_equal(gv.cpu().numpy().view(np.int32), bv.cpu().numpy().view(np.int32))
