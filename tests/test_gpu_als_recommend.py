"""GPU: DeviceALSFactors.recommend, ALSModel.recommend_for_all_users / _items /
_user_subset / _item_subset and ALSModel.ranking_metrics / evaluate_ranking.

Models are DeviceALSFactors built from host arrays: factors 0.3 N(0, 1) in
f32 from a fixed seed, padding columns zero, raw ids spaced 3 (users) and 7
(items) apart from a negative start. Every model has two item rows that
repeat another item's row and one all-zero user row (all its scores 0.0).

Expected lists: the JVM chain of tests/test_gpu_als_pairs.py (numpy, f32, one
rounded product and one rounded sum per column) over the full score matrix,
then np.argsort(-scores, kind="stable")[:num]: descending, equal scores in
row order = ascending raw id. Ids and score bits are compared exactly.

Ranking metrics: the oracle of tests/ranking_oracle.py over the host lists,
counts exact, metrics at rtol 1e-12 (means of <= 70 per-row values that are
themselves exact; the oracle's math.log gain table and the wrapper's numpy
one may differ in the last bit, 1.1e-16 relative)."""
import math

import numpy as np
import pytest
import torch
from ranking_oracle import mean_metrics

pytestmark = pytest.mark.gpu

#        name: users, items, k, kp
SHAPES = {"fused": (37, 29, 10, 16),       # <= 2048 candidates: the fused path, kk clamped to 29
          "pruned": (70, 2500, 10, 16),    # the bf16-pruned path
          "items": (2500, 40, 10, 16),     # the pruned path for side="item"
          "wide": (20, 2100, 65, 96),      # a wide rank
          "ties": (6, 4200, 10, 16)}       # the zero user row has 4200 > 4096 survivors: the overflow flag
NUMS = [1, 5, 8, 9, 10, 100]
ZERO_USER = 4
_CACHE = {}


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


def _expected(name, side, num, rows=None):
    user_ids, item_ids, _, _, _, acc = _host(name)
    scores, ids = (acc, item_ids) if side == "user" else (acc.T, user_ids)
    if rows is not None:
        scores = scores[rows]
    order = np.argsort(-scores, axis=1, kind="stable")[:, :num]
    return ids[order], np.take_along_axis(scores, order, axis=1)


def _assert_lists(got, exp):
    (gi, gv), (ei, ev) = got, exp
    assert gi.dtype == torch.int64 and gv.dtype == torch.float32 and gi.is_cuda and gv.is_cuda
    gi, gv = gi.cpu().numpy(), gv.cpu().numpy()
    assert gi.shape == ei.shape and gv.shape == ev.shape
    assert np.array_equal(gi, ei)
    assert np.array_equal(gv.view(np.uint32), np.ascontiguousarray(ev).view(np.uint32))


# ------------------------------------------------------------ 1. recommend
@pytest.mark.parametrize("num", NUMS)
@pytest.mark.parametrize("name,side", [("fused", "user"), ("fused", "item"), ("pruned", "user"), ("items", "item"),
                                       ("items", "user"), ("wide", "user"), ("ties", "user")])
def test_recommend_matches_the_host_ranking(device, name, side, num):
    model = _api_model(device, name).model
    n = len(model.user_ids if side == "user" else model.item_ids)
    rows = torch.arange(n, device=device)
    ids, scores = model.recommend(side, rows, num)
    torch.cuda.synchronize()
    n_other = len(model.item_ids if side == "user" else model.user_ids)
    assert ids.shape == (n, min(num, n_other))
    _assert_lists((ids, scores), _expected(name, side, num))
    # the bits transform / predict_pairs gives for those pairs
    own = np.repeat(np.asarray(model.user_ids if side == "user" else model.item_ids), ids.shape[1])
    other = ids.cpu().numpy().reshape(-1)
    pairs = model.predict_pairs(own, other) if side == "user" else model.predict_pairs(other, own)
    assert torch.equal(pairs.view(torch.int32), scores.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("name", ["pruned", "ties"])
@pytest.mark.parametrize("num", [5, 10])
def test_ties_keep_the_smaller_raw_id(device, name, num):
    """The all-zero user row: every score is 0.0 and the list is the num
    smallest raw ids; the repeated item rows tie in every other list. At 4200
    items the zero row overflows the survivor list: resolved on the device at
    num = 5, through the host fallback (in sub-batches of 2 rows) at num = 10."""
    from src import _hrec
    from src.als_model import DeviceALSFactors

    model = _api_model(device, name).model
    user_ids, item_ids, _, _, k, acc = _host(name)
    assert not acc[ZERO_USER].any() and np.array_equal(acc[:, 7], acc[:, 2]) and np.array_equal(acc[:, 20], acc[:, 9])
    if name == "ties":
        Q, F, Ft, bf, _ = model._recommend_operands("user")
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        _hrec.als_score_topk_pruned(Q, torch.arange(len(user_ids), device=device), Ft, F, bf, len(item_ids), k, num,
                                    check_overflow=False, overflow_out=flag)
        assert int(flag.item()) == 1, "this model is meant to take the overflow path"
    old = DeviceALSFactors.RECOMMEND_FALLBACK_BYTES
    DeviceALSFactors.RECOMMEND_FALLBACK_BYTES = 2 * 4 * len(item_ids)
    try:
        ids, scores = model.recommend("user", np.arange(len(user_ids)), num)
    finally:
        DeviceALSFactors.RECOMMEND_FALLBACK_BYTES = old
    _assert_lists((ids, scores), _expected(name, "user", num))
    assert ids[ZERO_USER].tolist() == item_ids[:num].tolist() and not scores[ZERO_USER].any()


def test_batches_give_the_same_tensors(device, monkeypatch):
    from src.als_model import DeviceALSFactors

    model = _api_model(device, "pruned").model
    rows = torch.as_tensor(np.random.default_rng(3).permutation(70), device=device)
    one = model.recommend("user", rows, 10)
    monkeypatch.setattr(DeviceALSFactors, "RECOMMEND_BATCH", 16)
    many = model.recommend("user", rows, 10)
    assert torch.equal(one[0], many[0]) and torch.equal(one[1].view(torch.int32), many[1].view(torch.int32))
    _assert_lists(many, _expected("pruned", "user", 10, rows.cpu().numpy()))
    assert model.recommend("user", rows[:0], 10)[0].shape == (0, 10)
    for bad in ([70], [-1]):
        with pytest.raises(ValueError):
            model.recommend("user", bad, 10)
    with pytest.raises(ValueError):
        model.recommend("users", rows, 10)


# ------------------------------------------------------- 2. public methods
def _assert_frame(frame, col, own_ids, exp):
    assert list(frame.columns) == [col, "recommendations"]
    assert frame[col].tolist() == list(own_ids)
    ei, ev = exp
    for r, rec in enumerate(frame["recommendations"]):
        assert isinstance(rec, list) and len(rec) == ei.shape[1]
        assert all(type(i) is int and type(s) is float for i, s in rec)
        assert [i for i, _ in rec] == ei[r].tolist()
        assert [np.float32(s).view(np.uint32) for _, s in rec] == ev[r].view(np.uint32).tolist()


def test_recommend_for_all(device):
    m = _api_model(device, "fused")
    user_ids, item_ids = _host("fused")[:2]
    _assert_frame(m.recommend_for_all_users(5), "userId", user_ids, _expected("fused", "user", 5))
    _assert_frame(m.recommend_for_all_items(40), "itemId", item_ids, _expected("fused", "item", 40))  # 37 users


def test_recommend_for_subsets(device):
    import pandas as pd

    m = _api_model(device, "fused")
    user_ids, item_ids = _host("fused")[:2]
    urows, irows = [30, 2, 11], [28, 0]
    users = [int(user_ids[r]) for r in (30, 2, 30, 11)] + [-49, 10 ** 6]  # a duplicate and two unknown ids
    exp = _expected("fused", "user", 3, sorted(urows))
    _assert_frame(m.recommend_for_user_subset(users, 3), "userId", sorted(user_ids[urows]), exp)
    frame = pd.DataFrame({"userId": np.array(users, np.int32), "other": 1.0})
    _assert_frame(m.recommend_for_user_subset(frame, 3), "userId", sorted(user_ids[urows]), exp)
    items = np.array([item_ids[28], item_ids[0], 5, item_ids[28]])
    exp = _expected("fused", "item", 4, sorted(irows))
    _assert_frame(m.recommend_for_item_subset(items, 4), "itemId", sorted(item_ids[irows]), exp)
    _assert_frame(m.recommend_for_item_subset(pd.DataFrame({"itemId": items}), 4), "itemId", sorted(item_ids[irows]),
                  exp)
    none = m.recommend_for_user_subset([10 ** 6], 3)
    assert len(none) == 0 and list(none.columns) == ["userId", "recommendations"]


def test_recommend_errors(device):
    from src.als_model import ALSModel

    m = _api_model(device, "fused")
    for call in (lambda x: x.recommend_for_all_users(3), lambda x: x.recommend_for_all_items(3),
                 lambda x: x.recommend_for_user_subset([1], 3), lambda x: x.recommend_for_item_subset([1], 3),
                 lambda x: x.ranking_metrics(None), lambda x: x.evaluate_ranking(None)):
        with pytest.raises(RuntimeError):
            call(ALSModel())
    for num in (0, 1025, -1):
        with pytest.raises(ValueError):
            m.recommend_for_all_users(num)
        with pytest.raises(ValueError):
            m.recommend_for_item_subset([-40], num)
    with pytest.raises(ValueError):
        m.recommend_for_user_subset([1.5], 3)


# ------------------------------------------------------------ 3. evaluator
@pytest.fixture(scope="module")
def held_out():
    """~300 rows over 40 users of the 70 x 2500 model: three of the user's
    ten best items (so lists hit) and four others per user, a few items the
    model does not know, two unknown users, some rows twice."""
    import pandas as pd

    user_ids, item_ids, _, _, _, acc = _host("pruned")
    rng = np.random.default_rng(17)
    top = np.argsort(-acc, axis=1, kind="stable")[:, :10]
    users, items = [], []
    for u in rng.permutation(70)[:40]:
        picks = list(item_ids[rng.permutation(top[u])[:3]]) + list(item_ids[rng.integers(0, 2500, 4)])
        users += [user_ids[u]] * len(picks)
        items += picks
    users += [int(user_ids[3])] * 2 + [5000, 5000, 5001]
    items += [-39, 10 ** 5, int(item_ids[0]), -39, int(item_ids[1])]  # -39 and 10^5: unknown items
    users, items = np.array(users, np.int64), np.array(items, np.int64)
    again = rng.integers(0, len(users), 12)
    users, items = np.r_[users, users[again]], np.r_[items, items[again]]
    perm = rng.permutation(len(users))
    return pd.DataFrame({"userId": users[perm], "itemId": items[perm],
                         "average_review_rating": rng.integers(2, 11, len(perm)) / 2.0,
                         "stars": rng.integers(1, 6, len(perm)).astype(np.float64)})


def _oracle(frame, k, known_only):
    """(metrics by the oracle, users evaluated, unknown users) for the host ranking of the 70 x 2500 model."""
    user_ids, item_ids, _, _, _, acc = _host("pruned")
    row_of = {int(u): r for r, u in enumerate(user_ids)}
    lists, labs, unknown = [], [], 0
    for u in sorted(set(frame["userId"].tolist())):
        lab = sorted(set(frame["itemId"][frame["userId"] == u].tolist()))
        if u in row_of:
            lst = item_ids[np.argsort(-acc[row_of[u]], kind="stable")[:k]].tolist()
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


@pytest.mark.parametrize("host_rows", [1 << 16, 0])  # the label CSR built on the host / on the device
@pytest.mark.parametrize("k", [1, 10, 37])
def test_ranking_metrics_match_the_oracle(device, held_out, k, host_rows, monkeypatch):
    from src.als_model import ALSModel

    monkeypatch.setattr(ALSModel, "RANKING_HOST_ROWS", host_rows)
    m = _api_model(device, "pruned")
    assert len(held_out) >= 290
    exp, n_known, n_unknown = _oracle(held_out, k, True)
    assert n_unknown == 2
    if k == 10:
        assert exp[0] > 0.2 and exp[4] > 0.1, "the frame is built so that the lists hit"
    res = m.ranking_metrics(held_out, k=k)
    print(res, exp)
    _assert_metrics(res, exp, n_known, 2)
    m.cold_start_strategy = "nan"
    exp_all, n_all, _ = _oracle(held_out, k, False)
    res_nan = m.ranking_metrics(held_out, k=k)
    assert n_all == n_known + 2
    _assert_metrics(res_nan, exp_all, n_all, 0)
    for name in m.RANKING_METRIC_NAMES:  # the unknown users add zeros: the means scale by n_known / n_all
        np.testing.assert_allclose(res_nan[name], res[name] * n_known / n_all, rtol=1e-12, atol=0)


def test_min_rating_evaluate_ranking_and_errors(device, held_out):
    import pandas as pd

    m = _api_model(device, "pruned")
    kept = held_out[held_out["stars"] >= 3.0]
    assert 0 < kept["userId"].nunique() <= held_out["userId"].nunique() and len(kept) < len(held_out)
    exp, n_known, n_unknown = _oracle(kept, 10, True)
    res = m.ranking_metrics(held_out, k=10, label_col="stars", min_rating=3.0)
    _assert_metrics(res, exp, n_known, n_unknown)
    by_default_col = m.ranking_metrics(held_out, k=10, min_rating=3.0)
    exp_d, n_d, u_d = _oracle(held_out[held_out["average_review_rating"] >= 3.0], 10, True)
    _assert_metrics(by_default_col, exp_d, n_d, u_d)
    assert m.RANKING_METRIC_NAMES == ("meanAveragePrecision", "meanAveragePrecisionAtK", "precisionAtK", "recallAtK",
                                      "ndcgAtK")
    for name in m.RANKING_METRIC_NAMES:
        v = m.evaluate_ranking(held_out, name, k=10, label_col="stars", min_rating=3.0)
        assert type(v) is float and v == res[name]
    assert m.evaluate_ranking(held_out) == m.ranking_metrics(held_out)["meanAveragePrecision"]
    with pytest.raises(ValueError, match="meanAveragePrecision, meanAveragePrecisionAtK"):
        m.evaluate_ranking(held_out, "map")
    for k in (0, 1025):
        with pytest.raises(ValueError):
            m.ranking_metrics(held_out, k=k)
    # nobody left: NaN metrics, count 0
    res = m.ranking_metrics(held_out, min_rating=99.0)
    assert res["count"] == 0 and res["dropped"] == 0 and all(math.isnan(res[n]) for n in m.RANKING_METRIC_NAMES)
    only_unknown = pd.DataFrame({"userId": [5000, 5001], "itemId": [2, 9]})
    res = m.ranking_metrics(only_unknown)
    assert res["count"] == 0 and res["dropped"] == 2 and math.isnan(res["ndcgAtK"])
    m.cold_start_strategy = "nan"
    res = m.ranking_metrics(only_unknown)
    assert res["count"] == 2 and res["dropped"] == 0 and all(res[n] == 0.0 for n in m.RANKING_METRIC_NAMES)


# ----------------------------------------------------------- 4. end to end
def test_implicit_fit_recommend_evaluate(device):
    import pandas as pd
    from src.als_model import ALSModel

    rng = np.random.default_rng(23)
    pairs = rng.permutation(60 * 80)[:700]
    train = pd.DataFrame({"userId": 11 + 2 * (pairs // 80), "itemId": 5 + 3 * (pairs % 80),
                          "average_review_rating": rng.integers(1, 6, 700).astype(np.float64),
                          "rating": 3.0, "price": 1.0, "number_of_reviews": 2.0})
    model = ALSModel(rank=8, max_iter=3, implicit_prefs=True, alpha=10, seed=5)
    assert model.train(train)
    user_ids, item_ids = np.asarray(model.model.user_ids), np.asarray(model.model.item_ids)
    scores = model.model.score(user_ids, item_ids).cpu().numpy()  # transform's bits, the whole matrix
    lists = [item_ids[np.argsort(-scores[r], kind="stable")[:10]].tolist() for r in range(len(user_ids))]
    labs = [sorted(set(train["itemId"][train["userId"] == u].tolist())) for u in user_ids]
    exp = mean_metrics(lists, labs, 10)
    res = model.ranking_metrics(train, k=10)
    _assert_metrics(res, exp, len(user_ids), 0)
    for name in model.RANKING_METRIC_NAMES:
        v = model.evaluate_ranking(train, name)
        assert type(v) is float and math.isfinite(v) and 0.0 < v <= 1.0 and v == res[name]
    frame = model.recommend_for_all_users(10)
    assert frame["userId"].tolist() == user_ids.tolist()
    assert [[i for i, _ in rec] for rec in frame["recommendations"]] == lists
