"""GPU: rank_of / full_ranking_metrics / evaluate_full_ranking of the ALS, the
two-tower and the hybrid model.

Small models: 60 users x 300 candidate items; ALS rank 8, two iterations,
trained on users 0 .. 49 and about nine tenths of the items; two-tower
embedding_size 50 and 64, freshly built; the candidate frame is shuffled.

The promise of rank_of is checked against the models' existing list methods;
the metrics against tests/rank_positions_oracle.py run on the scores each model
materialises itself (ALS: DeviceALSFactors.score; two-tower: hrec_tt_score;
hybrid: adaptive_fusion of the two per-user calls). Counts exactly, the means
within rtol (terms + 8) 2^-52 (f64 sums in another order)."""
import math

import numpy as np
import pandas as pd
import pytest
import torch
from sklearn.preprocessing import MinMaxScaler

import rank_positions_oracle as rpo

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_WARM = 60, 300, 50
EPS = 2.0 ** -52
HYBRID_USERS = list(range(0, 18)) + list(range(48, 54))  # warm and cold


class Setup:
    def __init__(self, d, seed):
        from src.als_model import ALSModel
        from src.hybrid_system import HybridRecommendationSystem
        from src.two_tower_model import TwoTowerModel

        rng = np.random.default_rng(seed)
        ids = rng.permutation(N_ITEMS).astype(np.int64)  # shuffled: frame row != itemId order
        self.ids = ids
        self.frame = pd.DataFrame({"itemId": ids, "manufacturer_id": rng.integers(0, 30, N_ITEMS),
                                   "category_id": rng.integers(0, 10, N_ITEMS), "price": rng.random(N_ITEMS) * 100,
                                   "average_review_rating": rng.integers(0, 11, N_ITEMS).astype(np.float64) / 2})
        pool = np.sort(rng.choice(N_ITEMS, 270, replace=False))
        rows = [(u, int(i), float(rng.integers(1, 6))) for u in range(N_WARM) for i in rng.choice(pool, 8, False)]
        self.train = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
        self.als = ALSModel(rank=8, max_iter=2, reg_param=0.1, seed=seed)
        assert self.als.train(self.train) is True
        feats = rng.random((N_ITEMS, 4))
        self.als.item_features = {int(i): {"features": feats[i], "rating": float(rng.integers(1, 11)) / 2}
                                  for i in range(N_ITEMS)}
        self.tt = TwoTowerModel(N_USERS, N_ITEMS + 8, 30, 10, embedding_size=d, seed=seed)
        self.tt.build_model()
        self.tt.scaler = MinMaxScaler().fit(self.frame[["price", "average_review_rating"]])
        self.h = HybridRecommendationSystem()
        self.h.als_model, self.h.twotower_model, self.h.models_loaded = self.als, self.tt, True
        self.h.als_f1_score, self.h.twotower_f1_score = 0.5, 0.1
        self.cand = self.tt.candidates(self.frame)
        # held-out pairs: twelve per user, two of them training pairs where the user has any, one item outside
        # every catalogue, one pair repeated; a weight and a rating per row
        held = []
        for u in range(N_USERS):
            own = self.train["itemId"][self.train["userId"] == u].to_numpy()
            items = rng.choice(N_ITEMS, 9, replace=False).tolist() + own[:2].tolist() + [N_ITEMS + 50]
            held += [(u, int(i)) for i in items] + [(u, int(items[0]))]
        order = rng.permutation(len(held))
        self.data = pd.DataFrame([held[i] for i in order], columns=["userId", "itemId"])
        self.data["w"] = rng.integers(0, 5, len(held)).astype(np.float64) + rng.random(len(held))
        self.data["average_review_rating"] = rng.integers(1, 6, len(held)).astype(np.float64)
        self._scores = {}

    def scores(self, model):
        """(users: row -> userId, candidate ids: column -> itemId, the model's own score matrix as numpy)."""
        if model in self._scores:
            return self._scores[model]
        from src import _hrec

        if model == "als":
            m = self.als.model
            users, cols = np.asarray(m.user_ids, np.int64), np.asarray(m.item_ids, np.int64)
            s = m.score(users, cols).cpu().numpy()
        elif model == "tt":
            users, cols = np.arange(N_USERS, dtype=np.int64), self.ids
            U = self.tt.model.user_vectors(torch.as_tensor(users.astype(np.int32), device=self.tt.model.device))
            s = _hrec.tt_score(U, self.cand.vectors).cpu().numpy()
        else:
            users, cols = np.array(HYBRID_USERS, np.int64), self.ids
            s = np.empty((users.size, N_ITEMS))
            for r, u in enumerate(users):
                fused = dict(self.h.adaptive_fusion(self.als.predict_for_user(int(u), self.ids),
                                                    self.tt.predict_for_user(int(u), self.frame)))
                assert len(fused) == N_ITEMS
                s[r] = [fused[int(i)] for i in self.ids]
        self._scores[model] = (users, cols, s)
        return self._scores[model]

    def frame_of(self, model):
        """The held-out pairs the model is asked about."""
        if model == "hybrid":
            return self.data[self.data["userId"].isin(HYBRID_USERS)].reset_index(drop=True)
        return self.data

    def call(self, model, name, data, *args, **kw):
        if model == "als":
            return getattr(self.als, name)(data, *args, **kw)
        return getattr(self.tt if model == "tt" else self.h, name)(data, self.cand, *args, **kw)

    def lists(self, model, users, n, exclude):
        """{userId: [itemId, ...]} from the model's existing top-n method."""
        if model == "als":
            df = self.als.recommend_for_user_subset(users, n, exclude=exclude)
        else:
            df = (self.tt if model == "tt" else self.h).recommend_for_users(users, self.cand, n, exclude=exclude)
        return {int(u): [int(i) for i, _ in rec] for u, rec in zip(df["userId"], df["recommendations"])}

    def oracle(self, model, data, weight_col=None, exclude=None):
        """(rank per row of data, sums) of the oracle over the model's own scores."""
        users, cols, s = self.scores(model)
        col_of = {int(i): j for j, i in enumerate(cols)}
        row_of = {int(u): r for r, u in enumerate(users)}
        du, di = data["userId"].to_numpy(), data["itemId"].to_numpy()
        rank = np.full(len(data), -1, np.int64)
        sums = dict.fromkeys(rpo.SUMS, 0.0)
        for u in np.unique(du):
            at = np.flatnonzero(du == u)
            if int(u) not in row_of:
                sums["unranked"] += at.size
                continue
            lc = [col_of.get(int(i), -1) for i in di[at]]
            ex = None
            if exclude is not None:
                ex = [col_of[int(i)] for i in exclude["itemId"][exclude["userId"] == u] if int(i) in col_of]
            w = None if weight_col is None else data[weight_col].to_numpy()[at]
            rk, (auc, rr, swpr, sw), (_, ranked, unranked) = rpo.row_positions(s[row_of[int(u)]], lc, w, ex)
            rank[at] = rk
            if not math.isnan(auc):
                sums["sum_auc"] += auc
                sums["n_auc"] += 1
            if not math.isnan(rr):
                sums["sum_reciprocal_rank"] += rr
                sums["n_reciprocal_rank"] += 1
            sums["sum_w_pr"] += swpr
            sums["sum_w"] += sw
            sums["ranked"] += ranked
            sums["unranked"] += unranked
        return rank, sums


_CACHE = {}


def _setup(d):
    if d not in _CACHE:
        _CACHE[d] = Setup(d, seed={50: 21, 64: 22}[d])
    return _CACHE[d]


MODELS = [("als", 50), ("tt", 50), ("tt", 64), ("hybrid", 50), ("hybrid", 64)]
IDS = [f"{m}-{d}" for m, d in MODELS]


@pytest.mark.parametrize("model,d", MODELS, ids=IDS)
def test_rank_of_is_the_position_in_the_lists(device, model, d):
    s = _setup(d)
    data = s.frame_of(model)
    users = np.unique(data["userId"].to_numpy())
    n_cand = len(s.als.model.item_ids) if model == "als" else N_ITEMS
    for exclude in (None, s.train):
        out = s.call(model, "rank_of", data, exclude=exclude)
        assert list(out.columns) == list(data.columns) + ["rank"] and out["rank"].dtype == np.int64
        known = out["userId"].to_numpy()
        assert len(out) == (int((data["userId"] < N_WARM).sum()) if model == "als" else len(data))  # "drop"
        for n in (1, 10, min(n_cand, 1024)):
            lists = s.lists(model, users, n, exclude)
            for u, i, r in zip(known, out["itemId"].to_numpy(), out["rank"].to_numpy()):
                lst = lists[int(u)]
                if 0 <= r < n:
                    assert r < len(lst) and lst[r] == i, (u, i, r, n)
                else:
                    assert i not in lst, (u, i, r, n)
        # per user, the labels ranked below k are the hits of the existing top-k list
        k = 10
        lists = s.lists(model, users, k, exclude)
        for u in np.unique(known):
            mine = out[out["userId"] == u]
            below = set(mine["itemId"][(mine["rank"] >= 0) & (mine["rank"] < k)].tolist())
            assert below == set(lists[int(u)]) & set(mine["itemId"].tolist()), u
        assert (out["rank"] >= 0).any() and (out["rank"] < 0).any()
        if exclude is not None:  # the training pairs among the held-out ones are unranked
            seen = set(zip(s.train["userId"], s.train["itemId"]))
            hit = np.array([(u, i) in seen for u, i in zip(out["userId"], out["itemId"])])
            assert hit.any() and (out["rank"].to_numpy()[hit] == -1).all()


def _assert_metrics(res, sums, n_pairs, dropped=0):
    exp = rpo.metrics(sums)
    assert res["count"] == int(sums["n_reciprocal_rank"]) and res["pairs"] == int(sums["ranked"])
    assert res["unranked"] == n_pairs - int(sums["ranked"]) and res["dropped"] == dropped
    for name, terms in (("meanPercentileRank", sums["ranked"]), ("auc", sums["n_auc"]),
                        ("meanReciprocalRank", sums["n_reciprocal_rank"])):
        # numerator and denominator are sums of `terms` non-negative f64 values in another order, then one division
        assert abs(res[name] - exp[name]) <= (terms + 8) * EPS * abs(exp[name]), (name, res[name], exp[name])
    assert 0.0 <= res["meanPercentileRank"] <= 1.0 and 0.0 <= res["auc"] <= 1.0


@pytest.mark.parametrize("model,d", MODELS, ids=IDS)
def test_metrics_match_the_oracle_on_the_models_own_scores(device, model, d):
    s = _setup(d)
    data = s.frame_of(model)
    if model == "als":  # "drop": the cold users' pairs leave before anything is counted
        kept = data[data["userId"] < N_WARM]
        dropped = int(data["userId"][data["userId"] >= N_WARM].nunique())
    else:
        kept, dropped = data, 0
    for exclude in (None, s.train):
        for weight_col in (None, "w"):
            rank, sums = s.oracle(model, kept, weight_col, exclude)
            res = s.call(model, "full_ranking_metrics", data, weight_col=weight_col, exclude=exclude)
            _assert_metrics(res, sums, len(kept), dropped)
            if weight_col is None:
                out = s.call(model, "rank_of", data, exclude=exclude)
                assert np.array_equal(out["rank"].to_numpy(), rank)
    # min_rating keeps the rows at or above it; evaluate_full_ranking returns one of the three
    sub = kept[kept["average_review_rating"] >= 4.0]
    _, sums = s.oracle(model, sub)
    res = s.call(model, "full_ranking_metrics", data, min_rating=4.0)
    _assert_metrics(res, sums, len(sub), dropped)
    for name in ("meanPercentileRank", "auc", "meanReciprocalRank"):
        assert s.call(model, "evaluate_full_ranking", data, metric_name=name, min_rating=4.0) == res[name]
    with pytest.raises(ValueError):
        s.call(model, "evaluate_full_ranking", data, metric_name="ndcgAtK")
    # nothing to rank: NaN metrics
    none = pd.DataFrame({"userId": [1, 2], "itemId": [N_ITEMS + 50, N_ITEMS + 51]})
    res = s.call(model, "full_ranking_metrics", none)
    assert all(math.isnan(res[k]) for k in ("meanPercentileRank", "auc", "meanReciprocalRank"))
    assert (res["count"], res["pairs"], res["unranked"]) == (0, 0, 2)


@pytest.mark.parametrize("model", ["als", "tt", "hybrid"])
def test_label_csr_built_on_the_device_gives_the_same_bits(device, model):
    """Frames above RANKING_HOST_ROWS rows sort and look up their labels on the device."""
    s = _setup(50)
    data = s.frame_of(model)
    obj = {"als": s.als, "tt": s.tt, "hybrid": s.h}[model]
    host = (s.call(model, "rank_of", data, exclude=s.train),
            s.call(model, "full_ranking_metrics", data, weight_col="w", exclude=s.train))
    try:
        obj.RANKING_HOST_ROWS = 0  # an instance attribute over the class constant
        dev_rank = s.call(model, "rank_of", data, exclude=s.train)
        dev_res = s.call(model, "full_ranking_metrics", data, weight_col="w", exclude=s.train)
    finally:
        del obj.RANKING_HOST_ROWS
    assert dev_rank.equals(host[0])
    assert dev_res == host[1]


def test_als_cold_start_strategies_and_unknown_ids(device):
    s = _setup(50)
    m = s.als.model
    unknown_item = int(next(i for i in range(N_ITEMS) if i not in set(np.asarray(m.item_ids).tolist())))
    known_item = int(np.asarray(m.item_ids)[3])
    data = pd.DataFrame({"userId": [0, 0, 55, 999, 999, 1], "itemId": [known_item, unknown_item, known_item,
                                                                        known_item, unknown_item, N_ITEMS + 50]})
    try:
        s.als.cold_start_strategy = "drop"
        out = s.als.rank_of(data)
        assert out.index.tolist() == [0, 1, 5] and out["rank"].tolist()[1:] == [-1, -1] and out["rank"].iloc[0] >= 0
        res = s.als.full_ranking_metrics(data)
        assert (res["dropped"], res["pairs"], res["unranked"], res["count"]) == (2, 1, 2, 1)
        s.als.cold_start_strategy = "nan"
        kept = s.als.rank_of(data)
        assert kept.index.tolist() == list(range(6)) and kept["rank"].tolist()[1:] == [-1] * 5
        assert kept["rank"].iloc[0] == out["rank"].iloc[0]
        res_nan = s.als.full_ranking_metrics(data)
        assert (res_nan["dropped"], res_nan["pairs"], res_nan["unranked"], res_nan["count"]) == (0, 1, 5, 1)
        for k in ("meanPercentileRank", "auc", "meanReciprocalRank"):
            assert res_nan[k] == res[k]
    finally:
        s.als.cold_start_strategy = "drop"


def test_two_tower_stale_candidates_raise(device):
    s = _setup(50)
    cand = s.tt.candidates(s.frame)
    fitted = s.tt.scaler
    try:
        other = s.frame[["price", "average_review_rating"]] * 2.0 + 1.0
        s.tt.scaler = MinMaxScaler().fit(other)
        for call in (s.tt.rank_of, s.tt.full_ranking_metrics, s.tt.evaluate_full_ranking, s.h.rank_of,
                     s.h.full_ranking_metrics):
            with pytest.raises(RuntimeError, match="candidates"):
                call(s.data, cand)
    finally:
        s.tt.scaler = fitted
    assert len(s.tt.rank_of(s.data, cand)) == len(s.data)
    with pytest.raises(IndexError):
        s.tt.rank_of(pd.DataFrame({"userId": [N_USERS], "itemId": [1]}), cand)


@pytest.mark.parametrize("model", ["als", "tt", "hybrid"])
def test_bad_weights_raise(device, model):
    s = _setup(50)
    for bad in (-1.0, math.nan, math.inf):
        data = s.frame_of(model).copy()
        data.loc[3, "w"] = bad
        with pytest.raises(ValueError, match="weights"):
            s.call(model, "full_ranking_metrics", data, weight_col="w")
