"""GPU: list_quality_metrics / evaluate_list_quality of the three models and
RecommenderEvaluator.evaluate_lists against the numpy oracle
(tests/list_quality_oracle.py) applied to each model's own public lists
(recommend_for_all_users(k, exclude=train)) and vectors.

Small models: 40 users x 60 items; ALS rank 8, two iterations, trained on
users 0 .. 35 and 54 of the items (users 36 .. 39 are cold, six items unknown
to the ALS model at least); two-tower embedding_size 50 and 64, freshly built. The
candidate frame is shuffled and holds every item.

Integer-derived quantities (coverage, Gini, personalization, counts) are
compared exactly. A mean over R lists: the largest per-list bound of
test_gpu_list_quality.py plus the two summations' 2 R 2^-53 max|v|. Entropy:
N 2^-53 plus two ulps of the largest |log2|."""
import numpy as np
import pandas as pd
import pytest
from sklearn.preprocessing import MinMaxScaler

import list_quality_oracle as lq

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, N_WARM, K = 40, 60, 36, 10
EXACT = ("catalogCoverage", "gini", "personalization", "count", "novelty_unseen")
MEANS = ("intraListDiversity", "unexpectedness", "novelty", "averagePopularity")


class Setup:
    def __init__(self, d, seed):
        from src.als_model import ALSModel
        from src.hybrid_system import HybridRecommendationSystem
        from src.two_tower_model import TwoTowerModel

        rng = np.random.default_rng(seed)
        ids = rng.permutation(N_ITEMS).astype(np.int64)  # shuffled: frame row != itemId order
        self.frame = pd.DataFrame({"itemId": ids, "manufacturer_id": rng.integers(0, 30, N_ITEMS),
                                   "category_id": rng.integers(0, 10, N_ITEMS), "price": rng.random(N_ITEMS) * 100,
                                   "average_review_rating": rng.integers(0, 11, N_ITEMS).astype(np.float64) / 2})
        self.ids = ids
        pool = np.sort(rng.choice(N_ITEMS, 54, replace=False))
        weights = 1.0 / (1.0 + np.arange(pool.size))  # skewed: popular items exist
        rows = [(u, int(i), float(rng.integers(1, 6))) for u in range(N_WARM)
                for i in rng.choice(pool, 7, False, p=weights / weights.sum())]
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

    def als_vectors(self):
        m = self.als.model
        return np.asarray(m.item_ids, np.int64), m.V[:, : m.k].cpu().numpy()

    def als_vectors_in_frame_order(self):
        item_ids, v = self.als_vectors()
        out = np.zeros((N_ITEMS, v.shape[1]), np.float32)
        pos = {int(i): r for r, i in enumerate(item_ids)}
        for r, i in enumerate(self.ids):
            if int(i) in pos:
                out[r] = v[pos[int(i)]]
        return out


_CACHE = {}


def _setup(device, d):
    if d not in _CACHE:
        _CACHE[d] = Setup(d, seed={50: 31, 64: 32}[d])
    return _CACHE[d]


def expected(df, item_ids, vectors, k, history):
    """The oracle over a lists frame: (summary dict, per-list values, counts)."""
    col = {int(i): c for c, i in enumerate(item_ids)}
    n = len(item_ids)
    width = max(len(r) for r in df["recommendations"])
    lists = np.full((len(df), width), -1, np.int64)
    lens = np.zeros(len(df), np.int64)
    for r, rec in enumerate(df["recommendations"]):
        lens[r] = len(rec)
        lists[r, : len(rec)] = [col.get(int(i), -1) for i, _ in rec]
    hist = tables = None
    if history is not None:
        hu, hi = history["userId"].to_numpy(), history["itemId"].to_numpy()
        assert all(int(i) in col for i in hi)  # every history item is a candidate here
        hc = np.array([col[int(i)] for i in hi])
        tables = lq.history_tables(hu, hc, n)
        hist = [np.unique(hc[hu == u]) for u in df["userId"]]
    res, vals, cnt, _ = lq.summary(lists, lens, vectors, k, history=hist, tables=tables)
    return res, vals, cnt, tables


def check(got, df, item_ids, vectors, k, history):
    want, vals, cnt, tables = expected(df, item_ids, vectors, k, history)
    d, n, rows = vectors.shape[1], len(item_ids), len(df)
    for name in EXACT:
        assert got[name] == want[name] or (np.isnan(got[name]) and np.isnan(want[name])), (name, got[name], want[name])
    total = int(cnt[:, 0].sum())
    tol = n * lq.U53 + 2 * np.spacing(np.log2(total))
    print("distributionalCoverage", got["distributionalCoverage"], "error",
          abs(got["distributionalCoverage"] - want["distributionalCoverage"]), "bound", tol)
    assert abs(got["distributionalCoverage"] - want["distributionalCoverage"]) <= tol
    m, g = cnt[:, 0].max(), cnt[:, 1].max()
    bounds = {"intraListDiversity": 8 * (d + m) * lq.U53, "unexpectedness": 8 * (d + m + g) * lq.U53}
    if tables is not None:
        bounds["novelty"] = 2 * m * lq.U53 * np.nanmax(np.abs(tables[0]))
        bounds["averagePopularity"] = 2 * m * lq.U53 * np.nanmax(np.abs(tables[1]))
    for c, name in enumerate(MEANS):
        if np.isnan(want[name]):
            assert np.isnan(got[name]), name
            continue
        tol = bounds[name] + 2 * rows * lq.U53 * np.nanmax(np.abs(vals[:, c]))
        print(name, got[name], "error", abs(got[name] - want[name]), "bound", tol)
        assert abs(got[name] - want[name]) <= tol, name
    return want


def same(a, b):
    assert set(a) == set(b)
    for key in a:
        assert a[key] == b[key] or (np.isnan(a[key]) and np.isnan(b[key])), (key, a[key], b[key])


def test_als(device):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, 50)
    item_ids, vec = s.als_vectors()
    before = s.als.recommend_for_all_users(K, exclude=s.train)
    before_plain = s.als.recommend_for_all_users(K)
    got = s.als.list_quality_metrics(K, exclude=s.train, history=s.train)
    assert got.pop("dropped") == 0 and got["count"] == N_WARM
    want = check(got, before, item_ids, vec, K, s.train)
    assert 0 < want["catalogCoverage"] <= 1 and want["novelty_unseen"] == 0
    # the internal keyword leaves every public return as it was
    assert s.als.recommend_for_all_users(K, exclude=s.train).equals(before)
    assert s.als.recommend_for_all_users(K).equals(before_plain)
    assert s.als.recommend_for_user_subset([3, 5], K, exclude=s.train).equals(
        before[before["userId"].isin([3, 5])].reset_index(drop=True))
    # any lists frame through the evaluator: the same numbers
    same(RecommenderEvaluator.evaluate_lists(before, item_ids, vec, history=s.train), got)
    # no exclusion, no history: three NaNs
    plain = s.als.list_quality_metrics(K)
    assert all(np.isnan(plain[name]) for name in ("novelty", "averagePopularity", "unexpectedness"))
    plain.pop("dropped")
    check(plain, before_plain, item_ids, vec, K, None)
    same(RecommenderEvaluator.evaluate_lists(before_plain, item_ids, vec), plain)
    # a subset with an unknown id
    sub = s.als.list_quality_metrics(K, users=[2, 7, 7, 11, 1000, 38], exclude=s.train, history=s.train)
    assert sub.pop("dropped") == 2 and sub["count"] == 3
    check(sub, before[before["userId"].isin([2, 7, 11])].reset_index(drop=True), item_ids, vec, K, s.train)
    assert s.als.evaluate_list_quality("gini", K, exclude=s.train) == got["gini"]
    with pytest.raises(ValueError):
        s.als.evaluate_list_quality("ndcgAtK")


@pytest.mark.parametrize("d", [50, 64])
def test_two_tower(device, d):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, d)
    vec = s.cand.vectors.cpu().numpy()
    before = s.tt.recommend_for_all_users(s.cand, K, exclude=s.train)
    before_plain = s.tt.recommend_for_all_users(s.frame, K)
    got = s.tt.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train)
    assert got.pop("dropped") == 0 and got["count"] == N_USERS
    check(got, before, s.ids, vec, K, s.train)
    assert s.tt.recommend_for_all_users(s.cand, K, exclude=s.train).equals(before)
    assert s.tt.recommend_for_all_users(s.frame, K).equals(before_plain)
    same(RecommenderEvaluator.evaluate_lists(before, s.ids, vec, history=s.train), got)
    plain = s.tt.list_quality_metrics(s.frame, K, users=np.arange(5, 25))
    assert plain.pop("dropped") == 0 and plain["count"] == 20
    assert all(np.isnan(plain[name]) for name in ("novelty", "averagePopularity", "unexpectedness"))
    check(plain, s.tt.recommend_for_users(np.arange(5, 25), s.frame, K), s.ids, vec, K, None)
    assert s.tt.evaluate_list_quality(s.cand, "personalization", K, exclude=s.train) == got["personalization"]


@pytest.mark.parametrize("d", [50, 64])
def test_hybrid(device, d):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, d)
    vec = s.cand.vectors.cpu().numpy()
    actual = s.train.iloc[::3]
    before = s.h.recommend_for_all_users(s.cand, K, exclude=s.train)
    before_actual = s.h.recommend_for_all_users(s.cand, K, exclude=s.train, actual=actual)
    got = s.h.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train)
    assert got.pop("dropped") == 0 and got["count"] == N_USERS
    check(got, before, s.ids, vec, K, s.train)
    assert s.h.recommend_for_all_users(s.cand, K, exclude=s.train).equals(before)
    assert s.h.recommend_for_all_users(s.cand, K, exclude=s.train, actual=actual).equals(before_actual)
    same(RecommenderEvaluator.evaluate_lists(before, s.ids, vec, history=s.train), got)
    # the per-user fused lists
    adaptive = s.h.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train, actual=actual)
    adaptive.pop("dropped")
    check(adaptive, before_actual, s.ids, vec, K, s.train)
    # cosines between ALS item factors; the items the ALS model does not know (six at least) are zero vectors
    avec = s.als_vectors_in_frame_order()
    assert (~avec.any(axis=1)).sum() == N_ITEMS - len(s.als.model.item_ids) >= 6
    als_sim = s.h.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train, similarity="als")
    als_sim.pop("dropped")
    check(als_sim, before, s.ids, avec, K, s.train)
    for name in EXACT + ("distributionalCoverage", "novelty", "averagePopularity"):
        assert als_sim[name] == got[name]  # the lists are the same: only the cosines differ
    plain = s.h.list_quality_metrics(s.frame, K)
    assert all(np.isnan(plain[name]) for name in ("novelty", "averagePopularity", "unexpectedness"))
    assert s.h.evaluate_list_quality(s.cand, "intraListDiversity", K, exclude=s.train,
                                     similarity="als") == als_sim["intraListDiversity"]
    with pytest.raises(ValueError):
        s.h.list_quality_metrics(s.cand, K, similarity="cooccurrence")
