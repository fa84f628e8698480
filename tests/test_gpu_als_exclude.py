"""GPU: seen-item exclusion in DeviceALSFactors.recommend (exclude=), the four
ALSModel.recommend_for_* methods and ALSModel.ranking_metrics / evaluate_ranking.

Models are made as in tests/test_gpu_als_recommend.py: DeviceALSFactors from
host arrays, factors 0.3 N(0, 1) in f32 from a fixed seed, padding columns
zero, raw ids spaced 3 (users) and 7 (items) apart from a negative start, two
item rows that repeat another item's row and one all-zero user row.

Expected lists: the numpy JVM chain over the full score matrix (f32, one
rounded product and one rounded sum per column), np.argsort(-scores,
kind="stable"), the query's excluded entries deleted, the first num kept. Ids,
score bits and lengths are compared exactly; past a list's length recommend
returns id 0 and a NaN score.

The exclusion of query q is pattern q % 7: nothing; exactly its unfiltered
top-num; a random 30 %; all of the first 2048 candidates but two; every
candidate; all but three; one member of the tied pair (candidate 2, the twin
of 7).

Ranking metrics: tests/ranking_oracle.py over the host lists, counts exact,
metrics at rtol 1e-12 (means of <= 70 per-row values that are themselves
exact; the oracle's math.log gain table and the wrapper's numpy one may
differ in the last bit, 1.1e-16 relative)."""
import numpy as np
import pytest
import torch
from ranking_oracle import mean_metrics

pytestmark = pytest.mark.gpu

#        name: users, items, k, kp
SHAPES = {"small": (37, 29, 10, 16),      # the small-catalogue path, kk clamped to 29
          "s2048": (5, 2048, 10, 16),     # the last catalogue scored whole
          "s2049": (5, 2049, 10, 16),     # the first with a sample and a filter pass
          "filter": (70, 2500, 10, 16),   # sample + filter; at most 2500 candidates: no overflow
          "items": (2500, 40, 10, 16),    # the same for side="item" (40 queries over 2500 users)
          "neginf": (6, 3000, 10, 16),    # -inf bounds with every item a candidate, no overflow
          "over": (6, 4200, 10, 16),      # rows 4 and 5 keep 4200 > 4096 candidates: the overflow flag
          "wide": (20, 2100, 65, 96),     # a wide rank that is no multiple of 4
          "many": (600, 300, 3, 16)}      # more queries than one grid pass
CASES = [("small", "user"), ("small", "item"), ("s2048", "user"), ("s2049", "user"), ("filter", "user"),
         ("items", "item"), ("neginf", "user"), ("over", "user"), ("wide", "user"), ("many", "user")]
NUMS = [1, 5, 10, 64, 65, 100]  # 64 / 65: the lane-maxima bound / the sample top-k
ZERO_USER = 4
_CACHE = {}
_EXCL = {}


def _host(name):
    """(user_ids, item_ids, U, V, k, score matrix by the JVM chain)."""
    if name not in _CACHE:
        nu, ni, k, kp = SHAPES[name]
        rng = np.random.default_rng(nu * 10007 + ni)
        U, V = np.zeros((nu, kp), np.float32), np.zeros((ni, kp), np.float32)
        U[:, :k] = (0.3 * rng.standard_normal((nu, k))).astype(np.float32)
        V[:, :k] = (0.3 * rng.standard_normal((ni, k))).astype(np.float32)
        V[7], V[20] = V[2], V[9]
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


def _excl(name, side, num):
    """bool [queries, candidates]: the exclusion pattern of each query row."""
    key = (name, side, num)
    if key not in _EXCL:
        scores = _scores(name, side)[0]
        n_q, n_c = scores.shape
        rng = np.random.default_rng(1000 * n_q + n_c + num)
        E = np.zeros((n_q, n_c), bool)
        for q in range(n_q):
            p = q % 7
            if p == 1:
                E[q, np.argsort(-scores[q], kind="stable")[:num]] = True
            elif p == 2:
                E[q] = rng.random(n_c) < 0.3
            elif p == 3:
                E[q, :2048] = True
                E[q, rng.choice(min(n_c, 2048), 2, replace=False)] = False
            elif p == 4:
                E[q] = True
            elif p == 5:
                E[q] = True
                E[q, rng.choice(n_c, 3, replace=False)] = False
            elif p == 6:
                E[q, 2] = True
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


# ------------------------------------------------------------ 1. recommend
@pytest.mark.parametrize("num", NUMS)
@pytest.mark.parametrize("name,side", CASES)
def test_recommend_excluding_matches_the_host_ranking(device, name, side, num):
    model = _api_model(device, name).model
    scores, _, query_ids = _scores(name, side)
    n, n_other = scores.shape
    E = _excl(name, side, num)
    excl = _exclusion(model, name, side, E)
    assert excl[0].dtype == torch.int64 and excl[1].dtype == torch.int32 and excl[0].numel() == n + 1
    assert int(excl[0][-1].item()) == int(E.sum()) == excl[1].numel()
    ids, vals, lens = model.recommend(side, torch.arange(n, device=device), num, exclude=excl)
    torch.cuda.synchronize()
    assert ids.shape == (n, min(num, n_other))
    exp = _expected(name, side, num, E)
    _assert_lists((ids, vals, lens), exp)
    # the bits transform / predict_pairs gives for those pairs
    live = np.arange(ids.shape[1])[None, :] < exp[2][:, None]
    own = np.broadcast_to(np.asarray(query_ids)[:, None], live.shape)[live]
    other = exp[0][live]
    if own.size:
        pairs = model.predict_pairs(own, other) if side == "user" else model.predict_pairs(other, own)
        got = vals[torch.as_tensor(live, device=device)]
        assert torch.equal(pairs.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("num", [5, 10, 65])
def test_overflow_flag_and_fallback(device, num):
    """6 x 4200: the zero row (everything excluded: a -inf bound) and the row
    that excludes all but three items keep all 4200 > 4096 candidates, so the
    flag is certain at every num; recommend then takes the masked fallback, in
    sub-batches of 2 rows."""
    from src import _hrec
    from src.als_model import DeviceALSFactors

    model = _api_model(device, "over").model
    user_ids, item_ids, _, _, k, acc = _host("over")
    E = _excl("over", "user", num)
    assert E[ZERO_USER].all() and not acc[ZERO_USER].any() and E[5].sum() == 4200 - 3
    excl = _exclusion(model, "over", "user", E)
    Q, F, Ft, _, _ = model._recommend_operands("user")
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    _hrec.als_score_topk_excluding(Q, torch.arange(len(user_ids), device=device), Ft, len(item_ids), k, num, *excl,
                                   overflow_out=flag)
    assert int(flag.item()) == 1, "this model is meant to take the overflow path"
    old = DeviceALSFactors.RECOMMEND_FALLBACK_BYTES
    DeviceALSFactors.RECOMMEND_FALLBACK_BYTES = 2 * 4 * len(item_ids)
    try:
        got = model.recommend("user", np.arange(len(user_ids)), num, exclude=excl)
    finally:
        DeviceALSFactors.RECOMMEND_FALLBACK_BYTES = old
    _assert_lists(got, _expected("over", "user", num, E))
    assert int(got[2][ZERO_USER].item()) == 0 and int(got[2][5].item()) == 3


def test_no_overflow_below_the_cap(device):
    """6 x 3000: rows 3, 4 and 5 have a -inf bound and keep all 3000 <= 4096 candidates: no flag."""
    from src import _hrec

    model = _api_model(device, "neginf").model
    user_ids, item_ids, _, _, k, _ = _host("neginf")
    E = _excl("neginf", "user", 10)
    excl = _exclusion(model, "neginf", "user", E)
    Q, F, Ft, _, ids = model._recommend_operands("user")
    flag = torch.ones(1, dtype=torch.int32, device=device)
    out_i, out_v, out_n = _hrec.als_score_topk_excluding(Q, torch.arange(6, device=device), Ft, 3000, k, 10, *excl,
                                                         overflow_out=flag)
    assert int(flag.item()) == 0
    ei, ev, el = _expected("neginf", "user", 10, E)
    assert np.array_equal(out_n.cpu().numpy(), el)
    for q in range(6):  # entries past out_len are unspecified
        assert np.array_equal(item_ids[out_i[q, : el[q]].cpu().numpy()], ei[q, : el[q]])
        assert np.array_equal(out_v[q, : el[q]].cpu().numpy().view(np.uint32), ev[q, : el[q]].view(np.uint32))


@pytest.mark.parametrize("name", ["small", "s2049"])
def test_raw_csr_with_duplicates_and_out_of_range_columns(device, name):
    """The library's own contract: duplicates count once, a column outside
    [0, n_items) is ignored; hrec_mask_rows_f32 writes and counts the same set."""
    from src import _hrec

    model = _api_model(device, name).model
    user_ids, item_ids, _, _, k, acc = _host(name)
    n_u, n_i = acc.shape
    top = np.argsort(-acc[1], kind="stable")[:2]
    row1 = sorted([int(top[0])] * 2 + [int(top[1])] + [3, 3, 3])
    seg = {0: [-7, -1, 0, 0, 5, n_i, n_i + 1, 1 << 30], 1: [-3] + row1 + [n_i], 3: [n_i, 1 << 30]}
    indptr = np.zeros(n_u + 1, np.int64)
    for r, s in seg.items():
        indptr[r + 1] = len(s)
    indptr = np.cumsum(indptr)
    cols = np.array([c for r in sorted(seg) for c in seg[r]], np.int32)
    E = np.zeros((n_u, n_i), bool)
    E[0, [0, 5]] = True
    E[1, row1] = True
    excl = (torch.as_tensor(indptr, device=device), torch.as_tensor(cols, device=device))
    got = model.recommend("user", torch.arange(n_u, device=device), 10, exclude=excl)
    _assert_lists(got, _expected(name, "user", 10, E))
    rows = torch.as_tensor([3, 1, 0, 1], device=device)
    vals = torch.as_tensor(np.ascontiguousarray(acc[[3, 1, 0, 1]]), device=device)
    kept = _hrec.mask_rows(vals, rows, *excl, fill=-7.5)
    exp = acc[[3, 1, 0, 1]].copy()
    exp[E[[3, 1, 0, 1]]] = -7.5
    assert np.array_equal(vals.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    assert kept.dtype == torch.int32 and kept.tolist() == [n_i, n_i - len(set(row1)), n_i - 2, n_i - len(set(row1))]


@pytest.mark.parametrize("name,side", [("small", "user"), ("filter", "user"), ("items", "item")])
def test_empty_exclusion_is_the_unfiltered_ranking(device, name, side):
    model = _api_model(device, name).model
    n, n_other = _scores(name, side)[0].shape
    rows = torch.arange(n, device=device)
    plain = model.recommend(side, rows, 10)
    assert isinstance(plain, tuple) and len(plain) == 2  # without exclude: today's pair
    excl = model.exclusion(side, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert excl[0].numel() == n + 1 and not excl[0].any() and excl[1].numel() == 0
    ids, vals, lens = model.recommend(side, rows, 10, exclude=excl)
    assert torch.equal(ids, plain[0]) and torch.equal(vals.view(torch.int32), plain[1].view(torch.int32))
    assert lens.tolist() == [min(10, n_other)] * n
    _assert_lists((ids, vals, lens), _expected(name, side, 10, np.zeros((n, n_other), bool)))


def test_batches_sub_batches_and_repeats_give_the_same_tensors(device, monkeypatch):
    from src.als_model import DeviceALSFactors

    def same(a, b):
        return (torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
                and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))

    model = _api_model(device, "filter").model
    rows_h = np.random.default_rng(3).permutation(70)
    rows = torch.as_tensor(rows_h, device=device)
    E = _excl("filter", "user", 10)
    excl = _exclusion(model, "filter", "user", E)  # over the factor rows: any row order, any subset
    one = model.recommend("user", rows, 10, exclude=excl)
    assert same(one, model.recommend("user", rows, 10, exclude=excl))
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_BATCH", 16)
    assert same(one, model.recommend("user", rows, 10, exclude=excl))
    _assert_lists(one, _expected("filter", "user", 10, E[rows_h], rows_h))
    monkeypatch.setattr(DeviceALSFactors, "EXCLUSION_HOST_PAIRS", 0)  # the device builder
    on_dev = _exclusion(model, "filter", "user", E)
    assert torch.equal(on_dev[0], excl[0]) and torch.equal(on_dev[1], excl[1]) and on_dev[1].dtype == torch.int32
    monkeypatch.undo()
    # the fallback in one sub-batch and in sub-batches of one row
    over = _api_model(device, "over").model
    E = _excl("over", "user", 10)
    excl = _exclusion(over, "over", "user", E)
    whole = over.recommend("user", np.arange(6), 10, exclude=excl)
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_FALLBACK_BYTES", 4 * 4200)
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_BATCH", 4)
    assert same(whole, over.recommend("user", np.arange(6), 10, exclude=excl))
    # errors: shapes of the pair, rows, num
    got = model.recommend("user", rows[:0], 10, exclude=_exclusion(model, "filter", "user", _excl("filter", "user", 10)))
    assert got[0].shape == (0, 10) and got[2].shape == (0,)
    good = model.exclusion("user", np.zeros(0, np.int64), np.zeros(0, np.int64))
    for bad in ((good[0][:-1], good[1]), (good[0].to(torch.int32), good[1]), (good[0], good[1].to(torch.int64))):
        with pytest.raises(ValueError):
            model.recommend("user", rows, 10, exclude=bad)
    for bad_rows in ([70], [-1]):
        with pytest.raises(ValueError):
            model.recommend("user", bad_rows, 10, exclude=good)
    with pytest.raises(ValueError):
        model.recommend("user", rows, 1025, exclude=good)
    with pytest.raises(ValueError):
        model.exclusion("users", [1], [1])
    with pytest.raises(ValueError):
        model.exclusion("user", [1, 2], [1])


# ------------------------------------------------------- 2. public methods
def _assert_frame(frame, col, own_ids, exp, E, cand_ids):
    assert list(frame.columns) == [col, "recommendations"]
    assert frame[col].tolist() == list(own_ids)
    ei, ev, el = exp
    for r, rec in enumerate(frame["recommendations"]):
        assert isinstance(rec, list) and len(rec) == el[r]
        assert all(type(i) is int and type(s) is float for i, s in rec)
        assert [i for i, _ in rec] == ei[r, : el[r]].tolist()
        assert [np.float32(s).view(np.uint32) for _, s in rec] == ev[r, : el[r]].view(np.uint32).tolist()
        assert not set(i for i, _ in rec) & set(cand_ids[E[r]].tolist())  # no excluded pair appears


def test_recommend_for_all_and_subsets_with_exclude(device):
    import pandas as pd

    m = _api_model(device, "small")
    user_ids, item_ids = _host("small")[:2]
    E = _excl("small", "user", 5)
    users, items = _pairs("small", "user", E)
    rng = np.random.default_rng(5)
    again = rng.integers(0, len(users), 40)
    # duplicates, a pair of an unknown user and one of an unknown item: they change nothing
    users = np.r_[users, users[again], [10 ** 6, int(user_ids[0])]]
    items = np.r_[items, items[again], [int(item_ids[0]), -39]]
    perm = rng.permutation(len(users))
    train = pd.DataFrame({"userId": users[perm].astype(np.int32), "itemId": items[perm].astype(np.float64),
                          "average_review_rating": 3.0})
    assert not E[0].any() and E[4].all() and E[5].sum() == 26
    frame = m.recommend_for_all_users(5, exclude=train)
    _assert_frame(frame, "userId", user_ids, _expected("small", "user", 5, E), E, item_ids)
    assert frame["recommendations"][4] == [] and len(frame["recommendations"][5]) == 3  # the row stays, empty
    # the item side reads the same frame transposed
    _assert_frame(m.recommend_for_all_items(40, exclude=train), "itemId", item_ids,
                  _expected("small", "item", 40, E.T), E.T, user_ids)
    urows, irows = [2, 4, 11, 30], [0, 28]
    exp = _expected("small", "user", 3, E[urows], urows)
    got = m.recommend_for_user_subset([int(user_ids[r]) for r in (30, 2, 30, 11, 4)] + [10 ** 6], 3, exclude=train)
    _assert_frame(got, "userId", user_ids[urows], exp, E[urows], item_ids)
    exp = _expected("small", "item", 4, E.T[irows], irows)
    got = m.recommend_for_item_subset(pd.DataFrame({"itemId": item_ids[[28, 0, 28]]}), 4, exclude=train)
    _assert_frame(got, "itemId", item_ids[irows], exp, E.T[irows], user_ids)
    # an empty frame: the unfiltered lists
    empty = train.iloc[:0]
    plain, same = m.recommend_for_all_users(5), m.recommend_for_all_users(5, exclude=empty)
    assert plain["recommendations"].tolist() == same["recommendations"].tolist()
    with pytest.raises(ValueError):
        m.recommend_for_all_users(5, exclude=pd.DataFrame({"userId": [1.5], "itemId": [2]}))


# ------------------------------------------------------------ 3. evaluator
@pytest.fixture(scope="module")
def split():
    """(train, held_out) for the 70 x 2500 model, as a fitted model sees them:
    train holds each user's 5 best-scored items and 20 others (user row 6:
    every item; unknown ids and duplicates besides); held_out, over 40 users,
    three of the ranks 6..15 (hit only once train is excluded), one train item
    (never hit, counted in the set size), three others; two unknown users."""
    import pandas as pd

    user_ids, item_ids, _, _, _, acc = _host("filter")
    rng = np.random.default_rng(29)
    order = np.argsort(-acc, axis=1, kind="stable")
    E = np.zeros(acc.shape, bool)
    for u in range(70):
        E[u, order[u, :5]] = True
        E[u, rng.integers(0, 2500, 20)] = True
    E[6] = True
    tu, ti = _pairs("filter", "user", E)
    tu, ti = np.r_[tu, tu[:30], [5000, int(user_ids[1])]], np.r_[ti, ti[:30], [int(item_ids[3]), -39]]
    train = pd.DataFrame({"userId": tu, "itemId": ti})
    users, items = [], []
    for u in [6] + [int(x) for x in rng.permutation(70)[:39] if x != 6]:
        picks = (list(item_ids[rng.permutation(order[u, 5:15])[:3]]) + [int(item_ids[order[u, 0]])]
                 + list(item_ids[rng.integers(0, 2500, 3)]))
        users += [user_ids[u]] * len(picks)
        items += picks
    users += [5000, 5000, 5001]
    items += [int(item_ids[0]), -39, int(item_ids[1])]
    users, items = np.array(users, np.int64), np.array(items, np.int64)
    perm = rng.permutation(len(users))
    held = pd.DataFrame({"userId": users[perm], "itemId": items[perm],
                         "average_review_rating": rng.integers(2, 11, len(perm)) / 2.0})
    return train, held, E


def _oracle(frame, k, known_only, E):
    """(metrics by the oracle, users evaluated, unknown users) for the host ranking minus E (None: nothing)."""
    user_ids, item_ids, _, _, _, acc = _host("filter")
    row_of = {int(u): r for r, u in enumerate(user_ids)}
    lists, labs, unknown = [], [], 0
    for u in sorted(set(frame["userId"].tolist())):
        lab = sorted(set(frame["itemId"][frame["userId"] == u].tolist()))
        if u in row_of:
            order = np.argsort(-acc[row_of[u]], kind="stable")
            if E is not None:
                order = order[~E[row_of[u]][order]]
            lst = item_ids[order[:k]].tolist()
        else:
            unknown += 1
            if known_only:
                continue
            lst = []
        lists.append(lst)
        labs.append(lab)
    return mean_metrics(lists, labs, k), len(lists), unknown


ORACLE_ORDER = ("precisionAtK", "recallAtK", "meanAveragePrecision", "meanAveragePrecisionAtK", "ndcgAtK")


def _assert_metrics(res, exp, count, dropped):
    assert res["count"] == count and res["dropped"] == dropped and len(res) == 7
    for name, e in zip(ORACLE_ORDER, exp):
        np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0)


@pytest.mark.parametrize("k", [1, 10, 37])
def test_ranking_metrics_with_exclude_match_the_oracle(device, split, k):
    train, held, E = split
    m = _api_model(device, "filter")
    exp, n_known, n_unknown = _oracle(held, k, True, E)
    assert n_unknown == 2 and n_known >= 39
    res = m.ranking_metrics(held, k=k, exclude=train)
    print(res, exp)
    _assert_metrics(res, exp, n_known, 2)
    plain = m.ranking_metrics(held, k=k)
    _assert_metrics(plain, _oracle(held, k, True, None)[0], n_known, 2)
    assert res["precisionAtK"] != plain["precisionAtK"] and res["ndcgAtK"] != plain["ndcgAtK"]
    for name in m.RANKING_METRIC_NAMES:
        v = m.evaluate_ranking(held, name, k=k, exclude=train)
        assert type(v) is float and v == res[name]
    m.cold_start_strategy = "nan"
    exp_all, n_all, _ = _oracle(held, k, False, E)
    res_nan = m.ranking_metrics(held, k=k, exclude=train)
    assert n_all == n_known + 2
    _assert_metrics(res_nan, exp_all, n_all, 0)
    for name in m.RANKING_METRIC_NAMES:  # the unknown users add zeros: the means scale by n_known / n_all
        np.testing.assert_allclose(res_nan[name], res[name] * n_known / n_all, rtol=1e-12, atol=0)
