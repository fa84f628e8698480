"""GPU: seen-item exclusion on the bf16-pruned ALS top-k path
(hrec_als_score_topk_pruned_excluding) and DeviceALSFactors.recommend(exclude=)
on top of it, with its two fallback levels.

Models and expected lists are made as in tests/test_gpu_als_exclude.py:
DeviceALSFactors from host arrays, factors 0.3 N(0, 1) in f32 from a fixed
seed, padding columns zero, raw ids spaced 3 (users) and 7 (items) apart from a
negative start, rows 7 and 20 the twins of rows 2 and 9 on the item side, row 7
the twin of row 2 on the user side, one all-zero user row (not in the "f"
models). Expected lists: the numpy JVM chain over the full score matrix (f32,
one rounded product and one rounded sum per column), np.argsort(-scores,
kind="stable"), the query's excluded entries deleted, the first num kept. Ids,
score bits and lengths are compared exactly.

The exclusion of query q is pattern PATTERNS[q % 8] (the "f" models: FLAG0_ROWS,
FLAG0_ROWS_LONG above num 10):
nothing; exactly its unfiltered top-num; a random 30 %; all of the first 8192
candidates but a run of 200; all of the first 8192 but two; every candidate; all
but three; one member of the tied pair (candidate 2, the twin of 7).

Flag-0 shapes. _restated() restates the bound on the host: bf16 round-to-
nearest-even operands, f32 accumulation, the sample's excluded scores -inf, t_b
the kk-th of the 64 lane maxima (kk <= 64) or the kk-th best (above), E_b, tau_b
and tau_b - E_b as pr_bounds forms them. From it: whether every t_b is finite,
and an upper bound of the pairs the filter keeps (the restated scores against
tau_b - E_b lowered by 1e-5, far above the 1e-6 by which another f32
accumulation order can move a score of this size). The designated (model, num)
cases assert, before anything runs on the device, that every bound is finite
and that the kept pairs stay below the list cap, below the fused kernel's 2048
LDS candidates for kk <= 8, and below n_items / 4; only then *overflow == 0 is
asserted on the device. The seeds and the patterns of the "f" models were chosen
on the host so that this holds: above num 10 the 200 items that "but200" leaves
of the sample put the bound near the median score (the restatement counts about 750
to 6800 kept pairs), so those rows take the random 30 % instead, and at 2049
items the 64 lane maxima are over 32 items each, whose 64th keeps up to 763 >
2049 / 4 pairs: (f2049, 64) is left to the recommend tests ("s2049")."""
import numpy as np
import pytest
import torch
from ranking_oracle import mean_metrics

pytestmark = pytest.mark.gpu

#        name: users, items, k, kp, with the all-zero user row
SHAPES = {"s2048": (10, 2048, 10, 16, True),    # the last catalogue handed to hrec_als_score_topk_excluding
          "s2049": (10, 2049, 10, 16, True),    # the first on the pruned path (the sample is the catalogue)
          "s8192": (10, 8192, 10, 16, True),    # the sample is still the catalogue
          "s8193": (10, 8193, 10, 16, True),    # one item past the sample
          "u9000": (24, 9000, 10, 16, True),    # rank 10 at kp 16: dk 32
          "items": (9000, 40, 10, 16, True),    # side "item": 40 queries over 9000 users
          "wide": (16, 9000, 65, 96, True),     # rank 65 at kp 96: dk 128
          "many": (600, 2100, 10, 16, True),    # more queries than one grid pass
          "f2048": (8, 2048, 10, 16, False),    # the flag-0 models: Gaussian rows only
          "f2049": (8, 2049, 10, 16, False),
          "f8192": (8, 8192, 10, 16, False),
          "f8193": (8, 8193, 10, 16, False),
          "f9000": (8, 9000, 10, 16, False),
          "fwide": (8, 9000, 65, 96, False)}
CASES = [("s2048", "user"), ("s2049", "user"), ("s8192", "user"), ("s8193", "user"), ("u9000", "user"),
         ("items", "item"), ("wide", "user"), ("many", "user")]
# 1..8: the fused rescore-and-rank kernel (templates 2, 4, 8); 64 / 65: the two bound kernels
NUMS = [1, 2, 4, 5, 8, 9, 10, 64, 65, 100]
PATTERNS = ("none", "top", "random", "but200", "but2", "all", "but3", "tie")
FLAG0_ROWS = ("none", "top", "random", "but200", "tie", "random", "top", "none")
FLAG0_ROWS_LONG = ("none", "top", "random", "random", "tie", "random", "top", "none")  # num > 10
FLAG0 = [(name, num) for name in ("f2049", "f8192", "f8193", "f9000", "fwide") for num in NUMS
         if (name, num) != ("f2049", 64)]
ZERO_USER = 4
SAMPLE = 8192   # kPruneSample
CAP = 4096      # kCap
LDS_CANDS = 2048
REL = 2.0 ** -7 + 2.0 ** -13
_CACHE = {}
_EXCL = {}


def _host(name):
    """(user_ids, item_ids, U, V, k, score matrix by the JVM chain)."""
    if name not in _CACHE:
        nu, ni, k, kp, zero = SHAPES[name]
        rng = np.random.default_rng(nu * 10007 + ni + k)
        U, V = np.zeros((nu, kp), np.float32), np.zeros((ni, kp), np.float32)
        U[:, :k] = (0.3 * rng.standard_normal((nu, k))).astype(np.float32)
        V[:, :k] = (0.3 * rng.standard_normal((ni, k))).astype(np.float32)
        V[7], V[20] = V[2], V[9]
        U[7] = U[2]
        if zero:
            U[ZERO_USER] = 0.0
        acc = np.zeros((nu, ni), np.float32)
        for c in range(k):
            acc = (acc + (U[:, c, None] * V[None, :, c]).astype(np.float32)).astype(np.float32)
        for a in (U, V, acc):
            a.setflags(write=False)
        _CACHE[name] = (-50 + 3 * np.arange(nu, dtype=np.int64), -40 + 7 * np.arange(ni, dtype=np.int64), U, V, k, acc)
    return _CACHE[name]


def _api_model(device, name):
    """An ALSModel over the host factors (one per test: the cached operands start empty)."""
    from src.als_model import ALSModel, DeviceALSFactors, DeviceSession

    user_ids, item_ids, U, V, k, _ = _host(name)
    m = ALSModel(rank=k)
    m.spark = DeviceSession()
    m.model = DeviceALSFactors(user_ids, item_ids, torch.as_tensor(U, device=device), torch.as_tensor(V, device=device),
                               k)
    return m


def _scores(name, side):
    """(scores [queries, candidates], the candidates' raw ids, the queries' raw ids)."""
    user_ids, item_ids, _, _, _, acc = _host(name)
    return (acc, item_ids, user_ids) if side == "user" else (acc.T, user_ids, item_ids)


def _pattern(p, scores_q, num, rng):
    n_c = scores_q.shape[0]
    e = np.zeros(n_c, bool)
    if p == "top":
        e[np.argsort(-scores_q, kind="stable")[:num]] = True
    elif p == "random":
        e = rng.random(n_c) < 0.3
    elif p == "but200":  # a run: every lane of the sample's lane maxima keeps three items
        e[:SAMPLE] = True
        start = int(rng.integers(0, min(n_c, SAMPLE) - 200 + 1))
        e[start: start + 200] = False
    elif p == "but2":
        e[:SAMPLE] = True
        e[rng.choice(min(n_c, SAMPLE), 2, replace=False)] = False
    elif p == "all":
        e[:] = True
    elif p == "but3":
        e[:] = True
        e[rng.choice(n_c, 3, replace=False)] = False
    elif p == "tie":
        e[2] = True
    return e


def _excl(name, side, num):
    """bool [queries, candidates]: the exclusion pattern of each query row."""
    key = (name, side, num)
    if key not in _EXCL:
        scores = _scores(name, side)[0]
        n_q, n_c = scores.shape
        rng = np.random.default_rng(1000 * n_q + n_c + num)
        pats = PATTERNS if SHAPES[name][4] else (FLAG0_ROWS if num <= 10 else FLAG0_ROWS_LONG)
        E = np.stack([_pattern(pats[q % 8], scores[q], num, rng) for q in range(n_q)])
        E.setflags(write=False)
        _EXCL[key] = E
    return _EXCL[key]


def _pairs(name, side, E, rows=None):
    """(userId, itemId) arrays of the exclusion matrix's pairs (queries = rows, default all)."""
    _, cand_ids, query_ids = _scores(name, side)
    q, c = np.nonzero(E)
    if rows is not None:
        q = np.asarray(rows)[q]
    return (query_ids[q], cand_ids[c]) if side == "user" else (cand_ids[c], query_ids[q])


def _expected(name, side, num, E, rows=None):
    """(ids [n, kk], scores [n, kk], lens [n]): id 0 and NaN past a list's length."""
    scores, cand_ids, _ = _scores(name, side)
    if rows is not None:
        scores = scores[rows]
    n_q, n_c = scores.shape
    kk = min(num, n_c)
    ids = np.zeros((n_q, kk), np.int64)
    vals = np.full((n_q, kk), np.nan, np.float32)
    lens = np.zeros(n_q, np.int32)
    for q in range(n_q):
        order = np.argsort(-scores[q], kind="stable")
        lst = order[~E[q][order]][:kk]
        lens[q] = len(lst)
        ids[q, : len(lst)] = cand_ids[lst]
        vals[q, : len(lst)] = scores[q][lst]
    assert np.array_equal(lens, np.minimum(kk, n_c - E.sum(axis=1)))
    return ids, vals, lens


def _assert_lists(got, exp):
    (gi, gv, gl), (ei, ev, el) = got, exp
    assert gi.dtype == torch.int64 and gv.dtype == torch.float32 and gl.dtype == torch.int32
    assert gi.is_cuda and gv.is_cuda and gl.is_cuda
    gi, gv, gl = gi.cpu().numpy(), gv.cpu().numpy(), gl.cpu().numpy()
    assert gi.shape == ei.shape and gv.shape == ev.shape and gl.shape == el.shape
    assert np.array_equal(gl, el)
    assert np.array_equal(gi, ei)
    assert np.array_equal(gv.view(np.uint32) | (np.isnan(gv) * np.uint32(0xFFFFFFFF)),
                          ev.view(np.uint32) | (np.isnan(ev) * np.uint32(0xFFFFFFFF)))  # every NaN alike


def _exclusion(model, name, side, E, rows=None):
    users, items = _pairs(name, side, E, rows)
    return model.exclusion(side, users, items)


def _same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
            and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


def _bf16(x):
    """f32 -> the nearest bf16 (ties to even), as f32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(np.float32)


def _restated(name, num, E):
    """(every t_b finite, an upper bound of the pairs the bf16 filter keeps per query), side "user"."""
    _, _, U, V, k, _ = _host(name)
    n_q, n_c = E.shape
    kk, S = min(num, n_c), min(n_c, SAMPLE)
    uh, vh = _bf16(U[:, :k]), _bf16(V[:, :k])
    st = np.zeros((n_q, n_c), np.float32)
    for c in range(k):  # bf16 products are exact in f32
        st = (st + uh[:, c, None] * vh[None, :, c]).astype(np.float32)
    samp = st[:, :S].copy()
    samp[E[:, :S]] = -np.inf
    if kk <= 64:
        lanes = np.full((n_q, 64), -np.inf, np.float32)
        for lane in range(64):
            if lane < S:
                lanes[:, lane] = samp[:, lane::64].max(axis=1)
        t = -np.sort(-lanes, axis=1)[:, kk - 1]
    else:
        t = -np.sort(-samp, axis=1)[:, kk - 1]
    max_norm = np.float64(np.nextafter(np.float32((np.sqrt((V[:, :k].astype(np.float64) ** 2).sum(axis=1))
                                                   * (1.0 + 1e-6)).max()), np.float32(np.inf)))
    e = REL * (np.sqrt((U[:, :k].astype(np.float64) ** 2).sum(axis=1)) * (1.0 + 1e-6)) * max_norm + 1e-30
    finite = np.isfinite(t)
    tau = np.nextafter((np.where(finite, t, 0.0).astype(np.float64) - e).astype(np.float32), np.float32(-np.inf))
    thr2 = np.nextafter((tau.astype(np.float64) - e).astype(np.float32), np.float32(-np.inf))
    kept = (st.astype(np.float64) >= thr2[:, None].astype(np.float64) - 1e-5).sum(axis=1)
    return bool(finite.all()), kept


def _direct(device, model, name, rows, num, excl, ws=None):
    """The library entry itself on side "user": (out_idx, out_val, out_len, overflow)."""
    from src import _hrec

    _, item_ids, _, _, k, _ = _host(name)
    Q, F, Ft, bf, _ = model._recommend_operands("user")
    flag = torch.full((1,), 7, dtype=torch.int32, device=device)
    out = _hrec.als_score_topk_pruned_excluding(Q, torch.as_tensor(rows, dtype=torch.int64, device=device), Ft, F, bf,
                                                len(item_ids), k, num, *excl, overflow_out=flag, workspace=ws)
    torch.cuda.synchronize()
    return out + (int(flag.item()),)


# ------------------------------------------------------ 1. the library entry
@pytest.mark.parametrize("name,num", FLAG0)
def test_entry_answers_without_the_flag(device, name, num):
    from src import _hrec

    model = _api_model(device, name).model
    _, item_ids, _, _, k, _ = _host(name)
    n_q, n_i = SHAPES[name][0], len(item_ids)
    E = _excl(name, "user", num)
    # the conditions of the flag-0 shapes, from the host restatement of the bound
    assert (min(n_i, SAMPLE) - E[:, :SAMPLE].sum(axis=1) >= num).all()
    finite, kept_bound = _restated(name, num, E)
    limit = min(CAP, n_i // 4, LDS_CANDS if num <= 8 else CAP)
    print(name, num, "restated: finite", finite, "kept <=", kept_bound.tolist(), "limit", limit)
    assert finite and (kept_bound < limit).all()
    excl = _exclusion(model, name, "user", E)
    need = int(_hrec.lib().hrec_als_score_topk_pruned_excluding_workspace_bytes(n_q, n_i, num, k))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    out_i, out_v, out_n, flag = _direct(device, model, name, np.arange(n_q), num, excl, ws)
    assert flag == 0
    ei, ev, el = _expected(name, "user", num, E)
    assert out_n.dtype == torch.int32 and np.array_equal(out_n.cpu().numpy(), el) and (el == num).all()
    assert np.array_equal(item_ids[out_i.cpu().numpy()], ei)
    assert np.array_equal(out_v.cpu().numpy().view(np.uint32), ev.view(np.uint32))
    # the bound pruned: a path that keeps everything cannot pass
    kept, cands = _hrec.als_topk_pruned_counts(ws, n_q, n_i, num, k)
    kept, cands = kept.cpu().numpy(), cands.cpu().numpy()
    print("kept", kept.tolist(), "candidates", cands.tolist())
    assert (kept < CAP).all() and (kept < n_i / 4).all()
    assert (kept >= num).all() and (cands >= num).all() and (cands <= kept).all()


@pytest.mark.parametrize("num", [1, 8, 10, 65])
def test_entry_at_the_delegation_boundary(device, num):
    """2048 items: hrec_als_score_topk_excluding answers the call (no bf16 filter: the counts read zero)."""
    from src import _hrec

    model = _api_model(device, "f2048").model
    _, item_ids, _, _, k, _ = _host("f2048")
    E = _excl("f2048", "user", num)
    excl = _exclusion(model, "f2048", "user", E)
    need = int(_hrec.lib().hrec_als_score_topk_pruned_excluding_workspace_bytes(8, 2048, num, k))
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    out_i, out_v, out_n, flag = _direct(device, model, "f2048", np.arange(8), num, excl, ws)
    assert flag == 0
    ei, ev, el = _expected("f2048", "user", num, E)
    assert np.array_equal(out_n.cpu().numpy(), el)
    assert np.array_equal(item_ids[out_i.cpu().numpy()], ei)
    assert np.array_equal(out_v.cpu().numpy().view(np.uint32), ev.view(np.uint32))
    kept, cands = _hrec.als_topk_pruned_counts(ws, 8, 2048, num, k)
    assert not kept.any() and not cands.any()


def _flag1_exclusion():
    """u9000: nothing excluded but row 12, which keeps two items of the sample."""
    E = np.zeros((24, 9000), bool)
    E[12] = _pattern("but2", _host("u9000")[5][12], 10, np.random.default_rng(12))
    assert E[12].sum() == SAMPLE - 2
    return E


@pytest.mark.parametrize("num", [5, 10, 65])
def test_flag_and_both_fallback_levels(device, monkeypatch, num):
    """The all-zero user row (9000 tied items: the lists overflow) and the row
    with two items of the sample left (a -inf bound) set the flag, each on its
    own; recommend then answers through hrec_als_score_topk_excluding and, for
    what that flags too (both rows keep all 9000 > 4096 items there), the
    masked score matrix in sub-batches of 2 rows."""
    from src import _hrec
    from src.als_model import DeviceALSFactors

    model = _api_model(device, "u9000").model
    acc = _host("u9000")[5]
    E = _flag1_exclusion()
    assert not acc[ZERO_USER].any()
    excl = _exclusion(model, "u9000", "user", E)
    assert _direct(device, model, "u9000", [ZERO_USER], num, excl)[3] == 1
    assert _direct(device, model, "u9000", [12], num, excl)[3] == 1
    assert _direct(device, model, "u9000", [0, 1, 2, 3], num, excl)[3] == 0
    calls = {"pruned": 0, "exact": 0, "scores": 0}
    for key, fn_name in (("pruned", "als_score_topk_pruned_excluding"), ("exact", "als_score_topk_excluding"),
                         ("scores", "als_score")):
        def counted(*a, _f=getattr(_hrec, fn_name), _k=key, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(_hrec, fn_name, counted)
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_FALLBACK_BYTES", 2 * 4 * 9000)
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_BATCH", 8)
    got = model.recommend("user", np.arange(24), num, exclude=excl)
    # three batches; batches 0 (the zero row) and 1 (row 12) through both levels, 4 sub-batches of 2 rows each
    assert calls == {"pruned": 3, "exact": 2, "scores": 8}
    _assert_lists(got, _expected("u9000", "user", num, E))


# ------------------------------------------------------------ 2. recommend
@pytest.mark.parametrize("num", NUMS)
@pytest.mark.parametrize("name,side", CASES)
def test_recommend_excluding_matches_the_host_ranking(device, name, side, num):
    model = _api_model(device, name).model
    scores, _, query_ids = _scores(name, side)
    n, n_other = scores.shape
    E = _excl(name, side, num)
    excl = _exclusion(model, name, side, E)
    assert int(excl[0][-1].item()) == int(E.sum()) == excl[1].numel()
    ids, vals, lens = model.recommend(side, torch.arange(n, device=device), num, exclude=excl)
    torch.cuda.synchronize()
    assert ids.shape == (n, min(num, n_other))
    _assert_lists((ids, vals, lens), _expected(name, side, num, E))


@pytest.mark.parametrize("num", [5, 10, 100])
@pytest.mark.parametrize("name", ["s8193", "u9000"])
def test_empty_exclusion_is_the_unfiltered_ranking(device, name, num):
    model = _api_model(device, name).model
    n, n_other = _scores(name, "user")[0].shape
    rows = torch.arange(n, device=device)
    plain = model.recommend("user", rows, num)
    assert isinstance(plain, tuple) and len(plain) == 2  # without exclude: today's pair
    excl = model.exclusion("user", np.zeros(0, np.int64), np.zeros(0, np.int64))
    ids, vals, lens = model.recommend("user", rows, num, exclude=excl)
    assert torch.equal(ids, plain[0]) and torch.equal(vals.view(torch.int32), plain[1].view(torch.int32))
    assert lens.tolist() == [num] * n


@pytest.mark.parametrize("num", [5, 10])
def test_batches_and_repeats_give_the_same_tensors(device, monkeypatch, num):
    from src.als_model import DeviceALSFactors

    model = _api_model(device, "u9000").model
    rows_h = np.random.default_rng(3).permutation(24)
    rows = torch.as_tensor(rows_h, device=device)
    E = _excl("u9000", "user", num)
    excl = _exclusion(model, "u9000", "user", E)  # over the factor rows: any row order, any subset
    one = model.recommend("user", rows, num, exclude=excl)
    assert _same(one, model.recommend("user", rows, num, exclude=excl))
    for batch in (16, 4):
        monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_BATCH", batch)
        assert _same(one, model.recommend("user", rows, num, exclude=excl))
    _assert_lists(one, _expected("u9000", "user", num, E[rows_h], rows_h))


@pytest.mark.parametrize("num", [8, 10, 64, 100])
def test_recommend_equals_the_exact_entry(device, num):
    """9000 items: what hrec_als_score_topk_excluding gives for the same inputs."""
    from src import _hrec

    model = _api_model(device, "f9000").model
    _, item_ids, _, _, k, _ = _host("f9000")
    E = _excl("f9000", "user", num)
    excl = _exclusion(model, "f9000", "user", E)
    # without row 3 at num <= 10: "but200" leaves none of that entry's 2048-item sample, which keeps
    # all 9000 > 4096 items and sets its flag (the answer would be incomplete)
    rows = torch.as_tensor([0, 1, 2, 4, 5, 6, 7], device=device)
    Q, F, Ft, _, ids = model._recommend_operands("user")
    flag = torch.ones(1, dtype=torch.int32, device=device)
    old_i, old_v, old_n = _hrec.als_score_topk_excluding(Q, rows, Ft, 9000, k, num, *excl, overflow_out=flag)
    assert int(flag.item()) == 0 and old_n.tolist() == [num] * 7
    got = model.recommend("user", rows, num, exclude=excl)
    assert _same(got, (ids[old_i], old_v, old_n))


# ------------------------------------------------------- 3. public methods
ORACLE_ORDER = ("precisionAtK", "recallAtK", "meanAveragePrecision", "meanAveragePrecisionAtK", "ndcgAtK")


def test_subset_and_ranking_metrics_with_exclude(device, monkeypatch):
    """recommend_for_user_subset and ranking_metrics under "drop" on the 9000-item
    model, through the pruned entry: train holds each user's 5 best-scored items
    and 20 others, held_out three of the ranks 6..15 (hit only once train is
    excluded), one train item and three others; two unknown users."""
    import pandas as pd
    from src import _hrec

    m = _api_model(device, "f9000")
    assert m.cold_start_strategy == "drop"
    user_ids, item_ids, _, _, _, acc = _host("f9000")
    rng = np.random.default_rng(31)
    order = np.argsort(-acc, axis=1, kind="stable")
    E = np.zeros(acc.shape, bool)
    for u in range(8):
        E[u, order[u, :5]] = True
        E[u, rng.integers(0, 9000, 20)] = True
    tu, ti = _pairs("f9000", "user", E)
    train = pd.DataFrame({"userId": np.r_[tu, tu[:30], [5000]], "itemId": np.r_[ti, ti[:30], [int(item_ids[3])]]})
    users, items = [], []
    for u in range(8):
        picks = (list(item_ids[rng.permutation(order[u, 5:15])[:3]]) + [int(item_ids[order[u, 0]])]
                 + list(item_ids[rng.integers(0, 9000, 3)]))
        users += [user_ids[u]] * len(picks)
        items += picks
    users += [5000, 5001]
    items += [int(item_ids[0]), int(item_ids[1])]
    held = pd.DataFrame({"userId": np.array(users, np.int64), "itemId": np.array(items, np.int64)})
    calls = []

    def counted(*a, _f=_hrec.als_score_topk_pruned_excluding, **kw):
        calls.append(1)
        return _f(*a, **kw)
    monkeypatch.setattr(_hrec, "als_score_topk_pruned_excluding", counted)
    urows = [1, 3, 6]
    frame = m.recommend_for_user_subset([int(user_ids[r]) for r in (6, 1, 3, 6)] + [10 ** 6], 10, exclude=train)
    assert len(calls) == 1
    ei, ev, el = _expected("f9000", "user", 10, E[urows], urows)
    assert frame["userId"].tolist() == list(user_ids[urows])
    for r, rec in enumerate(frame["recommendations"]):
        assert [i for i, _ in rec] == ei[r].tolist() and len(rec) == el[r] == 10
        assert [np.float32(s).view(np.uint32) for _, s in rec] == ev[r].view(np.uint32).tolist()
    for k in (1, 10):
        lists = [item_ids[order[u][~E[u][order[u]]][:k]].tolist() for u in range(8)]
        labs = [sorted(set(held["itemId"][held["userId"] == user_ids[u]].tolist())) for u in range(8)]
        exp = mean_metrics(lists, labs, k)
        n_calls = len(calls)
        res = m.ranking_metrics(held, k=k, exclude=train)
        assert len(calls) == n_calls + 1
        assert res["count"] == 8 and res["dropped"] == 2
        for name, e in zip(ORACLE_ORDER, exp):
            np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0)
