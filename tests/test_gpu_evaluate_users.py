"""GPU: HybridRecommendationSystem.evaluate_users and RecommenderEvaluator.
evaluate_scores / summarize against the per-user RecommenderEvaluator.

Small models built the way test_gpu_hybrid_adaptive's are (ALS rank 8, two
iterations, a freshly built two-tower model, a shuffled candidate frame), over
50 and 4097 candidates — the second is past HYBRID_LISTS_SAMPLE, so the bounded
mode of the lists and of the per-model selections runs. 20 users: user 19 is
cold for the ALS model, user 7 has a single rated item, the others hold rated
items inside and outside the candidate frame.

Expected row of user u and a model: precision_at_k / recall_at_k / ndcg_at_k /
mae_rmse on (actual = {itemId: rating} of the user's rows in frame order,
predicted = dict(model.predict_for_user(u, ...)) or dict(adaptive_fusion(...))).
Precision, Recall and the undefined cases exactly; NDCG, MAE and RMSE within
rtol 2 (m + 8) 2^-52 (another summation order). adaptive_fusion lists the union
in Python set order, so for the hybrid Precision and Recall are compared for
the users whose top max(k) + 1 fused scores are strictly decreasing — at least
80 % of them.
"""
import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.preprocessing import MinMaxScaler

import user_metrics_oracle as um

pytestmark = pytest.mark.gpu

N_USERS, N_WARM = 20, 19
KS = (5, 10, 15, 20)
WEIGHTS = {True: (0.5, 0.1), False: (0.1, 0.5)}
MODELS = ("als", "twotower", "hybrid")
SUB = 7  # users per sub-batch


class Setup:
    def __init__(self, n_items, seed):
        from src.als_model import ALSModel
        from src.evaluation import RecommenderEvaluator
        from src.hybrid_system import HybridRecommendationSystem
        from src.two_tower_model import TwoTowerModel

        rng = np.random.default_rng(seed)
        self.n_items = n_items
        ids = rng.permutation(n_items).astype(np.int64)  # shuffled: frame row != itemId order
        self.ids = ids
        self.frame = pd.DataFrame({"itemId": ids, "manufacturer_id": rng.integers(0, 30, n_items),
                                   "category_id": rng.integers(0, 10, n_items), "price": rng.random(n_items) * 100,
                                   "average_review_rating": rng.integers(0, 11, n_items).astype(np.float64) / 2})
        pool = np.sort(rng.choice(n_items, min(n_items - 5, 270), replace=False))
        rows = [(u, int(i), float(rng.integers(1, 6))) for u in range(N_WARM) for i in rng.choice(pool, 8, False)]
        self.train = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
        self.als = ALSModel(rank=8, max_iter=2, reg_param=0.1, seed=seed)
        assert self.als.train(self.train) is True
        feats = rng.random((n_items, 4))
        self.als.item_features = {int(i): {"features": feats[i], "rating": float(rng.integers(1, 11)) / 2}
                                  for i in range(n_items)}
        self.tt = TwoTowerModel(N_USERS, n_items + 8, 30, 10, embedding_size=64, seed=seed)
        self.tt.build_model()
        self.tt.scaler = MinMaxScaler().fit(self.frame[["price", "average_review_rating"]])
        self.h = HybridRecommendationSystem()
        self.h.als_model, self.h.twotower_model, self.h.models_loaded = self.als, self.tt, True
        self.cand = self.tt.candidates(self.frame)
        # the evaluated frame: rated items inside and outside the candidate frame
        rows = []
        for u in range(N_USERS):
            if u == 7:
                rows.append((u, int(ids[3]), 4.0))  # a single rated item
                continue
            inside = rng.choice(ids, int(rng.integers(2, min(12, n_items))), replace=False)
            outside = n_items + 100 + rng.choice(50, int(rng.integers(0, 4)), replace=False)
            for i in np.concatenate([inside, outside]):
                rows.append((u, int(i), float(np.round(rng.uniform(1, 5), 1))))
        self.data = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"]) \
            .sample(frac=1.0, random_state=seed).reset_index(drop=True)
        self.actual = {u: {int(i): float(r) for i, r in zip(g["itemId"], g["average_review_rating"])}
                       for u, g in self.data.groupby("userId", sort=True)}
        self.ev = RecommenderEvaluator()
        self.preds = {u: (self.als.predict_for_user(u, ids), self.tt.predict_for_user(u, self.frame))
                      for u in range(N_USERS)}
        self._exp = {}

    def weights(self, als_wins):
        self.h.als_f1_score, self.h.twotower_f1_score = WEIGHTS[als_wins]

    def predicted(self, u, model, als_wins):
        a, t = self.preds[u]
        if model == "als":
            return dict(a)
        if model == "twotower":
            return dict(t)
        saved = self.h.als_f1_score, self.h.twotower_f1_score
        self.weights(als_wins)
        fused = self.h.adaptive_fusion(a, t)
        self.h.als_f1_score, self.h.twotower_f1_score = saved
        assert len(fused) == self.n_items
        return dict(fused)

    def expected(self, u, model, als_wins):
        """(values in the frame's column order, NDCG raised, MAE / RMSE raised, common items, strict ranking)."""
        key = (u, model, als_wins if model == "hybrid" else None)
        if key in self._exp:
            return self._exp[key]
        act, pred = self.actual[u], self.predicted(u, model, als_wins)
        vals = []
        for k in KS:
            vals += [self.ev.precision_at_k(act, pred, k), self.ev.recall_at_k(act, pred, k)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                vals.append(float(self.ev.ndcg_at_k(act, pred, 10)))
                nd_raised = False
            except ValueError:
                vals.append(math.nan)
                nd_raised = True
            try:
                vals += [float(x) for x in self.ev.mae_rmse(act, pred)]
                err_raised = False
            except ValueError:
                vals += [math.nan, math.nan]
                err_raised = True
        top = sorted(pred.values(), reverse=True)[: max(KS) + 1]
        strict = all(x > y for x, y in zip(top, top[1:]))
        self._exp[key] = (vals, nd_raised, err_raised, len(set(act) & set(pred)), strict)
        return self._exp[key]


_CACHE = {}


def _setup(device, n_items):
    if n_items not in _CACHE:
        _CACHE[n_items] = Setup(n_items, seed={50: 31, 4097: 32}[n_items])
    return _CACHE[n_items]


def _columns():
    cols = ["userId"]
    for k in KS:
        cols += [f"Precision@{k}", f"Recall@{k}"]
    return cols + ["NDCG", "MAE", "RMSE", "status"]


def _assert_row(row, exp, model, u, check_ranking=True):
    vals, nd_raised, err_raised, m, _ = exp
    got = [float(row[c]) for c in _columns()[1:-1]]
    st = int(row["status"])
    assert bool(st & um.NDCG_UNDEFINED) == nd_raised and bool(st & um.ERR_UNDEFINED) == err_raised, (model, u, st)
    assert bool(st & um.NO_COMMON) == (m == 0)
    if check_ranking:
        assert got[: 2 * len(KS)] == vals[: 2 * len(KS)], (model, u)
    for g, e in zip(got[2 * len(KS):], vals[2 * len(KS):]):
        if math.isnan(e) or e == 0.0:
            assert (math.isnan(g) and math.isnan(e)) or g == e, (model, u, g, e)
        else:
            assert abs(g - e) <= um.rtol(m) * abs(e), (model, u, g, e, m)


def _assert_frames(res, s, als_wins_of):
    users = sorted(s.actual)
    n_strict = 0
    for model in MODELS:
        df = res[model]
        assert list(df.columns) == _columns()
        assert df["userId"].tolist() == users
        assert df["status"].dtype == np.int32 and df["NDCG"].dtype == np.float64
        for (_, row), u in zip(df.iterrows(), users):
            exp = s.expected(u, model, als_wins_of(u))
            strict = model != "hybrid" or exp[4]
            n_strict += model == "hybrid" and exp[4]
            _assert_row(row, exp, model, u, check_ranking=strict)
    assert n_strict >= 0.8 * len(users)


def _same(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for c in a.columns:
        assert a[c].to_numpy().tobytes() == b[c].to_numpy().tobytes(), c


@pytest.mark.parametrize("als_wins", [True, False])
@pytest.mark.parametrize("n_items", [50, 4097])
def test_evaluate_users_matches_per_user(device, n_items, als_wins, monkeypatch):
    s = _setup(device, n_items)
    m = s.als.model
    assert (m._lookup(m.user_ids, np.arange(N_USERS)) < 0).sum() == N_USERS - N_WARM  # a cold ALS user is evaluated
    assert len(s.actual[7]) == 1
    assert any(i >= n_items for u in s.actual for i in s.actual[u])  # rated items outside the frame
    s.weights(als_wins)
    whole = s.h.evaluate_users(s.data, s.cand)
    _assert_frames(whole, s, lambda u: als_wins)
    assert (s.h.als_f1_score, s.h.twotower_f1_score) == WEIGHTS[als_wins]  # untouched
    row7 = whole["als"][whole["als"]["userId"] == 7].iloc[0]
    assert int(row7["status"]) & um.NDCG_UNDEFINED and int(row7["status"]) & um.ERR_UNDEFINED
    monkeypatch.setitem(s.h.__dict__, "RECOMMEND_SCORE_BYTES", 8 * n_items * SUB)  # several sub-batches
    parts = s.h.evaluate_users(s.data, s.frame)
    for model in MODELS:
        _same(parts[model], whole[model])
    one = s.h.evaluate_users(s.data, s.cand, models=("hybrid",))
    assert list(one) == ["hybrid"]
    _same(one["hybrid"], whole["hybrid"])
    # users without rows do not appear; other k values and another rating column
    some = s.data[s.data["userId"].isin([2, 7, 19])].rename(columns={"average_review_rating": "stars"})
    res = s.h.evaluate_users(some, s.cand, k_values=(3, 20), ndcg_k=5, models=("twotower",), rating_col="stars")
    df = res["twotower"]
    assert df["userId"].tolist() == [2, 7, 19] and "Precision@3" in df.columns and "Recall@20" in df.columns
    for (_, row), u in zip(df.iterrows(), [2, 7, 19]):
        act, pred = s.actual[u], s.predicted(u, "twotower", als_wins)
        assert row["Precision@3"] == s.ev.precision_at_k(act, pred, 3)
        assert row["Recall@20"] == s.ev.recall_at_k(act, pred, 20)
        if u != 7:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                e = float(s.ev.ndcg_at_k(act, pred, 5))
            assert abs(row["NDCG"] - e) <= um.rtol(len(act)) * abs(e)


@pytest.mark.parametrize("n_items", [50, 4097])
def test_actual_gives_each_user_its_own_weights(device, n_items):
    from src.als_model import compute_f1_score

    s = _setup(device, n_items)
    s.weights(True)
    # users 0, 3, 6, ...: the two-tower side's own top 10 as labels (so (0.2, 0.8) for them), 1, 4, ...: the ALS side's
    rows, own = [], {}
    for u in range(N_USERS):
        if u % 3 == 2:
            continue
        side = dict(s.preds[u][1] if u % 3 == 0 else s.preds[u][0])
        items = [int(i) for i, _ in sorted(side.items(), key=lambda x: x[1], reverse=True)[:10]]
        rows += [(u, i) for i in items]
        act = {i: 1.0 for i in items}
        own[u] = compute_f1_score(act, dict(s.preds[u][0])) > compute_f1_score(act, dict(s.preds[u][1]))
    assert any(own.values()) and not all(own.values())
    actual = pd.DataFrame(rows, columns=["userId", "itemId"])
    res = s.h.evaluate_users(s.data, s.cand, actual=actual)
    _assert_frames(res, s, lambda u: own.get(u, True))
    plain = s.h.evaluate_users(s.data, s.cand)
    _same(res["als"], plain["als"])
    _same(res["twotower"], plain["twotower"])
    assert res["hybrid"]["RMSE"].to_numpy().tobytes() != plain["hybrid"]["RMSE"].to_numpy().tobytes()
    # the weights' own k
    res3 = s.h.evaluate_users(s.data, s.cand, actual=actual, f1_k=3, models=("hybrid",))
    own3 = {}
    for u in own:
        act = {int(i): 1.0 for i in actual["itemId"][actual["userId"] == u]}
        own3[u] = compute_f1_score(act, dict(s.preds[u][0]), k=3) > compute_f1_score(act, dict(s.preds[u][1]), k=3)
    for (_, row), u in zip(res3["hybrid"].iterrows(), sorted(s.actual)):
        exp = s.expected(u, "hybrid", own3.get(u, True))
        _assert_row(row, exp, "hybrid", u, check_ranking=exp[4])


@pytest.mark.parametrize("n_items", [50, 4097])
def test_forced_overflow_goes_through_mode_1(device, n_items, monkeypatch):
    from src import _hrec

    s = _setup(device, n_items)
    s.weights(False)
    whole = s.h.evaluate_users(s.data, s.cand)
    monkeypatch.setitem(s.h.__dict__, "RECOMMEND_SCORE_BYTES", 8 * n_items * SUB)
    real_f1, real_lists = _hrec.hybrid_model_f1, _hrec.hybrid_lists_rowwise
    calls = []

    def f1_over(als, tt, *a, **k):
        calls.append(("f1", als.shape[0], k.get("mode", 0)))
        res = real_f1(als, tt, *a, **k)
        if k.get("mode", 0) == 0:
            res[2].fill_(1)
            res[3].zero_()
        return res

    def lists_over(als, tt, *a, **k):
        calls.append(("lists", als.shape[0], k.get("mode", 0)))
        res = real_lists(als, tt, *a, **k)
        if k.get("mode", 0) == 0:
            res[0].zero_()
            res[3].fill_(1)
        return res

    monkeypatch.setattr(_hrec, "hybrid_model_f1", f1_over)
    res = s.h.evaluate_users(s.data, s.cand)
    for model in MODELS:
        _same(res[model], whole[model])
    assert [x[1] for x in calls if x[0] == "f1" and x[2] == 0] == [SUB, SUB, 6]
    assert [x[1] for x in calls if x[0] == "f1" and x[2] == 1] == [3, 3, 1, 3, 3, 1, 3, 3]
    calls.clear()
    monkeypatch.setattr(_hrec, "hybrid_model_f1", real_f1)
    monkeypatch.setattr(_hrec, "hybrid_lists_rowwise", lists_over)
    res = s.h.evaluate_users(s.data, s.cand)
    for model in MODELS:
        _same(res[model], whole[model])
    assert [x[1] for x in calls if x[2] == 1] == [3, 3, 1, 3, 3, 1, 3, 3]


@pytest.mark.parametrize("n_items", [50, 4097])
def test_evaluate_scores_and_summarize(device, n_items):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, n_items)
    s.weights(True)
    whole = s.h.evaluate_users(s.data, s.cand)
    users = np.arange(N_USERS, dtype=np.int64)
    a, t = s.h._scores(users, s.cand)
    fb = s.h._als_fallback(users, s.cand.item_ids)
    assert fb is not None
    a64 = torch.where(torch.isnan(a), fb.unsqueeze(0).expand_as(a), a.double())
    _same(RecommenderEvaluator.evaluate_scores(s.data, t, users, s.ids), whole["twotower"])
    _same(RecommenderEvaluator.evaluate_scores(s.data, a64, users, s.ids), whole["als"])
    # host arrays, users in another order, a user without rows in `data` and one outside the scores
    perm = np.random.default_rng(1).permutation(N_USERS)
    data = s.data[s.data["userId"] != 4]
    extra = pd.concat([data, pd.DataFrame({"userId": [N_USERS + 3], "itemId": [int(s.ids[0])],
                                           "average_review_rating": [2.0]})], ignore_index=True)
    got = s.ev.evaluate_scores(extra, t.cpu().numpy()[perm], users[perm], s.ids)
    _same(got, whole["twotower"][whole["twotower"]["userId"] != 4].reset_index(drop=True))
    # summarize: the mean over the users where a metric is defined, and their count
    for model in MODELS:
        df = whole[model]
        summ = RecommenderEvaluator.summarize(df)
        assert list(summ.columns) == ["mean", "count"] and list(summ.index) == _columns()[1:-1]
        for name in summ.index:
            col = df[name].to_numpy()
            assert summ.loc[name, "count"] == np.sum(~np.isnan(col))
            assert summ.loc[name, "mean"] == np.nanmean(col)
        assert summ.loc["NDCG", "count"] < len(df) and summ.loc["Precision@5", "count"] == len(df)


def test_errors(device):
    from src.evaluation import RecommenderEvaluator
    from src.hybrid_system import HybridRecommendationSystem

    s = _setup(device, 50)
    s.weights(True)
    dup = pd.concat([s.data, s.data.iloc[:1]], ignore_index=True)
    with pytest.raises(ValueError, match="more than once"):
        s.h.evaluate_users(dup, s.cand)
    with pytest.raises(ValueError, match="more than once"):
        RecommenderEvaluator.evaluate_scores(dup, np.zeros((N_USERS, 50)), np.arange(N_USERS), s.ids)
    with pytest.raises(ValueError, match="Models not loaded"):
        HybridRecommendationSystem().evaluate_users(s.data, s.frame)
    with pytest.raises(ValueError, match="models must be among"):
        s.h.evaluate_users(s.data, s.cand, models=("als", "svd"))
    for bad in ((), (0,), (1025,), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="k_values"):
            s.h.evaluate_users(s.data, s.cand, k_values=bad)
    with pytest.raises(ValueError, match="ndcg_k"):
        s.h.evaluate_users(s.data, s.cand, ndcg_k=0)
    with pytest.raises(ValueError, match="f1_k must be in"):
        s.h.evaluate_users(s.data, s.cand, f1_k=0)
    feats = s.als.item_features
    try:
        s.als.item_features = None
        with pytest.raises(ValueError, match="unknown to the ALS model"):
            s.h.evaluate_users(s.data, s.frame)
    finally:
        s.als.item_features = feats
    empty = s.h.evaluate_users(s.data.iloc[:0], s.cand)
    assert list(empty) == list(MODELS) and all(len(df) == 0 and list(df.columns) == _columns()
                                               for df in empty.values())
