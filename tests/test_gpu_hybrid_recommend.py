"""GPU: HybridRecommendationSystem.recommend_for_users / recommend_for_all_users
/ ranking_metrics / evaluate_ranking.

Small models: 60 users x 300 candidate items; ALS rank 8, two iterations,
trained on users 0 .. 49 and about nine tenths of the items (users 50 .. 59
are cold, the other items unknown to the ALS model, whose item_features then
give most of them a cold-start value of their own); two-tower embedding_size
50 and 64, freshly built. The candidate frame is shuffled.

Expected lists: per_user(u) = sorted(adaptive_fusion(als.predict_for_user(u,
ids), tt.predict_for_user(u, frame)), key=score, reverse=True) with the
excluded pairs removed, cut to n: itemIds and f64 score bits are compared
exactly. Every queried user's per_user scores are asserted distinct (the seeds
below give that), so the set order adaptive_fusion lists the union in does not
matter. The tie rule is tested on a frame of its own.

Ranking metrics: tests/ranking_oracle.mean_metrics over the lists
recommend_for_users returns, at rtol 1e-12 (f64 sums in another order)."""
import numpy as np
import pandas as pd
import pytest
from ranking_oracle import mean_metrics
from sklearn.preprocessing import MinMaxScaler

pytestmark = pytest.mark.gpu

ORACLE_ORDER = ("precisionAtK", "recallAtK", "meanAveragePrecision", "meanAveragePrecisionAtK", "ndcgAtK")
N_USERS, N_ITEMS, N_WARM = 60, 300, 50
WEIGHTS = {True: (0.5, 0.1), False: (0.1, 0.5)}  # als_wins -> (als_f1_score, twotower_f1_score)


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
        # training frame: users 0 .. 49, eight ratings each over ~270 items
        pool = np.sort(rng.choice(N_ITEMS, 270, replace=False))
        rows = [(u, int(i), float(rng.integers(1, 6))) for u in range(N_WARM) for i in rng.choice(pool, 8, False)]
        self.train = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
        self.als = ALSModel(rank=8, max_iter=2, reg_param=0.1, seed=seed)
        assert self.als.train(self.train) is True
        known = set(self.train["itemId"].tolist())
        self.unknown = [int(i) for i in ids if int(i) not in known]
        assert len(self.unknown) >= 20
        # the tie pair: two items the ALS model does not know and has no features for (global mean for both)
        self.tie = (self.unknown[0], self.unknown[1])
        feats = rng.random((N_ITEMS, 4))
        self.als.item_features = {int(i): {"features": feats[i], "rating": float(rng.integers(1, 11)) / 2}
                                  for i in range(N_ITEMS) if i not in self.tie}
        self.tt = TwoTowerModel(N_USERS, N_ITEMS + 8, 30, 10, embedding_size=d, seed=seed)
        self.tt.build_model()
        self.tt.scaler = MinMaxScaler().fit(self.frame[["price", "average_review_rating"]])
        self.h = HybridRecommendationSystem()
        self.h.als_model, self.h.twotower_model, self.h.models_loaded = self.als, self.tt, True
        self.cand = self.tt.candidates(self.frame)
        self._ranked = {}
        # exclusion frames: the training frame; and one with foreign users / items and repeats
        eu = np.concatenate([np.repeat(np.arange(N_USERS), 30), [N_USERS + 5, -3, 0, 4]])
        ei = np.concatenate([rng.choice(ids, 30 * N_USERS), [int(ids[0]), int(ids[1]), N_ITEMS + 100, -1]])
        eu, ei = np.concatenate([eu, eu[:80]]), np.concatenate([ei, ei[:80]])
        order = rng.permutation(len(eu))
        self.foreign = pd.DataFrame({"userId": eu[order], "itemId": ei[order]})

    def weights(self, als_wins):
        self.h.als_f1_score, self.h.twotower_f1_score = WEIGHTS[als_wins]

    def per_user(self, u, als_wins, frame=None):
        """The per-user call the lists are checked against (cached for the main frame)."""
        key = (u, als_wins)
        if frame is None and key in self._ranked:
            return self._ranked[key]
        f = self.frame if frame is None else frame
        self.weights(als_wins)
        a = self.als.predict_for_user(u, f["itemId"].to_numpy())
        t = self.tt.predict_for_user(u, f)
        fused = self.h.adaptive_fusion(a, t)
        assert len(a) == len(t) == len(fused) == len(f)
        ranked = sorted(fused, key=lambda x: x[1], reverse=True)
        if frame is None:
            assert len(set(s for _, s in ranked)) == len(ranked), f"user {u}: tied fused scores"
            self._ranked[key] = ranked
        return ranked

    def expected(self, u, n, als_wins, exclude=None):
        lst = self.per_user(u, als_wins)
        if exclude is not None:
            gone = set(exclude["itemId"][exclude["userId"] == u].tolist())
            lst = [p for p in lst if p[0] not in gone]
        return lst[:n]


_CACHE = {}


def _setup(device, d):
    if d not in _CACHE:
        _CACHE[d] = Setup(d, seed={50: 21, 64: 22}[d])
    return _CACHE[d]


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _assert_frame(df, users, s, n, als_wins, exclude=None):
    assert list(df.columns) == ["userId", "recommendations"]
    assert df["userId"].tolist() == list(users)
    for u, rec in zip(users, df["recommendations"]):
        exp = s.expected(u, n, als_wins, exclude)
        assert [i for i, _ in rec] == [i for i, _ in exp], f"user {u}"
        np.testing.assert_array_equal(_bits([r for _, r in rec]), _bits([r for _, r in exp]), err_msg=f"user {u}")


@pytest.mark.parametrize("als_wins", [True, False])
@pytest.mark.parametrize("d", [50, 64])
def test_lists_match_per_user(device, d, als_wins):
    s = _setup(device, d)
    users = list(range(N_USERS))
    m = s.als.model
    assert (m._lookup(m.user_ids, np.arange(N_USERS)) < 0).sum() == N_USERS - N_WARM  # cold users are queried
    assert (m._lookup(m.item_ids, s.ids) < 0).sum() == len(s.unknown)               # and unknown candidates
    query = np.array(users[::-1] + [3, 3, 0])  # unsorted, repeated: distinct and ascending in the result
    for u in users:
        s.per_user(u, als_wins)  # asserts the scores distinct, for every queried user
    for n in (5, 40, 1024):
        for exclude in (None, s.train):
            s.weights(als_wins)
            df = s.h.recommend_for_users(query if n != 40 else pd.DataFrame({"userId": query}),
                                         s.frame if n == 5 else s.cand, n, exclude=exclude)
            _assert_frame(df, users, s, n, als_wins, exclude)
            if n == 1024:
                want = N_ITEMS - (0 if exclude is None else 8)
                assert [len(r) for r in df["recommendations"]] == [want if u < N_WARM or exclude is None else N_ITEMS
                                                                   for u in users]
    s.weights(als_wins)
    _assert_frame(s.h.recommend_for_users([5, 55, 9], s.cand, 10, exclude=s.foreign), [5, 9, 55], s, 10, als_wins,
                  s.foreign)
    _assert_frame(s.h.recommend_for_users(users, s.cand, 40, exclude=s.foreign), users, s, 40, als_wins, s.foreign)


def test_tie_keeps_frame_order(device):
    """Two candidates with the same features and embedding row, both cold on
    the ALS side with the same cold-start value: the same fused score for
    every user, listed in frame order (not in the set order per_user gives)."""
    s = _setup(device, 64)
    a, b = s.tie
    frame = s.frame.copy()
    ra, rb = (int(np.flatnonzero(s.ids == x)[0]) for x in (a, b))
    for c in ("manufacturer_id", "category_id", "price", "average_review_rating"):
        frame.loc[rb, c] = frame.loc[ra, c]
    emb = s.tt.model.tensors["item_emb"]
    saved = emb[b].clone()
    try:
        emb[b] = emb[a]
        first, second = (a, b) if ra < rb else (b, a)
        for als_wins in (True, False):
            scores = dict(s.per_user(7, als_wins, frame))
            assert _bits(scores[a]) == _bits(scores[b])  # the tie is real
            s.weights(als_wins)
            df = s.h.recommend_for_users([7, 52], frame, N_ITEMS)
            for rec in df["recommendations"]:
                got = [i for i, _ in rec]
                assert got.index(second) == got.index(first) + 1
            rec = dict(df["recommendations"][0])
            assert _bits(rec[a]) == _bits(scores[a])
    finally:
        emb[b] = saved


@pytest.mark.parametrize("d", [50, 64])
def test_sub_batches_and_overflow_route(device, d, monkeypatch):
    from src import _hrec
    from src.hybrid_system import HybridRecommendationSystem

    s = _setup(device, d)
    s.weights(True)
    base = {e: s.h.recommend_for_all_users(s.cand, 40, exclude=x) for e, x in (("none", None), ("train", s.train))}
    _assert_frame(base["train"], list(range(N_USERS)), s, 40, True, s.train)
    calls = []
    real = _hrec.hybrid_lists

    def counting(als, tt, *a, **k):
        calls.append((als.shape[0], k.get("mode", 0)))
        return real(als, tt, *a, **k)

    monkeypatch.setattr(_hrec, "hybrid_lists", counting)
    monkeypatch.setattr(HybridRecommendationSystem, "RECOMMEND_SCORE_BYTES", 8 * N_ITEMS * 7)  # 7 users a sub-batch
    for e, x in (("none", None), ("train", s.train)):
        calls.clear()
        df = s.h.recommend_for_all_users(s.cand, 40, exclude=x)
        assert [c[0] for c in calls] == [7] * 8 + [4] and all(c[1] == 0 for c in calls)
        assert df["recommendations"].tolist() == base[e]["recommendations"].tolist()

    def overflowing(als, tt, *a, **k):
        calls.append((als.shape[0], k.get("mode", 0)))
        res = real(als, tt, *a, **k)
        if k.get("mode", 0) == 0:  # pretend the list was cut: scramble the answer and raise the flag
            res[0].zero_()
            res[3].fill_(1)
        return res

    monkeypatch.setattr(_hrec, "hybrid_lists", overflowing)
    for e, x in (("none", None), ("train", s.train)):
        calls.clear()
        df = s.h.recommend_for_all_users(s.cand, 40, exclude=x)
        # every sub-batch of 7 is redone in mode 1, in pieces of 3 (16 bytes a key)
        assert [c for c in calls if c[1] == 0] == [(7, 0)] * 8 + [(4, 0)]
        assert [c[0] for c in calls if c[1] == 1] == [3, 3, 1] * 8 + [3, 1]
        assert df["recommendations"].tolist() == base[e]["recommendations"].tolist()


def test_degenerate_cases(device):
    s = _setup(device, 50)
    s.weights(False)
    users = list(range(N_USERS))
    for excl in (None, s.train):
        a = s.h.recommend_for_all_users(s.frame, 10, exclude=excl)
        b = s.h.recommend_for_users(np.arange(N_USERS), s.cand, 10, exclude=excl)
        assert a["userId"].tolist() == b["userId"].tolist() == users
        assert a["recommendations"].tolist() == b["recommendations"].tolist()
    everything = pd.concat([s.train, pd.DataFrame({"userId": np.full(N_ITEMS, 1), "itemId": s.ids})],
                           ignore_index=True)
    df = s.h.recommend_for_users([2, 1, 1], s.cand, 10, exclude=everything)
    assert df["userId"].tolist() == [1, 2]
    assert df["recommendations"][0] == [] and len(df["recommendations"][1]) == 10
    _assert_frame(df.iloc[1:], [2], s, 10, False, s.train)
    empty = s.h.recommend_for_users([], s.cand, 10)
    assert list(empty.columns) == ["userId", "recommendations"] and len(empty) == 0
    assert len(s.h.recommend_for_users(pd.DataFrame({"userId": np.zeros(0, np.int64)}), s.frame, 10,
                                       exclude=s.train)) == 0


def test_errors(device):
    from src.hybrid_system import HybridRecommendationSystem

    s = _setup(device, 50)
    fresh = HybridRecommendationSystem()
    data = pd.DataFrame({"userId": [0], "itemId": [1]})
    for call in (lambda: fresh.recommend_for_users([0], s.frame, 5), lambda: fresh.recommend_for_all_users(s.frame, 5),
                 lambda: fresh.ranking_metrics(data, s.frame), lambda: fresh.evaluate_ranking(data, s.frame)):
        with pytest.raises(ValueError, match="Models not loaded"):
            call()
    for n in (0, 1025):
        with pytest.raises(ValueError, match="num_items must be in"):
            s.h.recommend_for_users([0], s.cand, n)
    for bad in ([0, N_USERS], [-1]):
        with pytest.raises(IndexError, match="user_in: id out of range"):
            s.h.recommend_for_users(bad, s.cand, 5)
    with pytest.raises(IndexError, match="user_in: id out of range"):
        s.h.ranking_metrics(pd.DataFrame({"userId": [0, N_USERS], "itemId": [1, 2]}), s.cand)
    dup = pd.concat([s.frame.iloc[:20], s.frame.iloc[5:6]], ignore_index=True)
    with pytest.raises(ValueError, match="repeats an itemId"):
        s.h.recommend_for_users([0], dup, 5)
    with pytest.raises(ValueError, match="metric_name"):
        s.h.evaluate_ranking(data, s.cand, metric_name="auc")
    # unknown ids and no fallback vector
    feats = s.als.item_features
    known_rows = s.frame[~s.frame["itemId"].isin(s.unknown)].reset_index(drop=True)
    try:
        s.als.item_features = None
        with pytest.raises(ValueError, match="unknown to the ALS model"):
            s.h.recommend_for_users([N_WARM + 1], known_rows, 5)     # a cold user
        with pytest.raises(ValueError, match="unknown to the ALS model"):
            s.h.recommend_for_users([0], s.frame, 5)                 # unknown candidates
        assert len(s.h.recommend_for_users([0, 1], known_rows, 5)) == 2  # everything known: no vector needed
    finally:
        s.als.item_features = feats


def _held_out(s, rng):
    """Per user (all but 6 and 7) two of its unfiltered top 10, two random
    items and, for user 0, an item absent from the catalogue; ratings 1 .. 5."""
    rows = []
    for u in range(N_USERS):
        if u in (6, 7):
            continue
        top = s.per_user(u, True)
        items = [top[1][0], top[7][0]] + rng.choice(s.ids, 2).tolist()
        if u == 0:
            items.append(N_ITEMS + 3)
        rows += [(u, int(i), float(rng.integers(1, 6))) for i in items]
    df = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
    return df.sample(frac=1.0, random_state=3).reset_index(drop=True)


@pytest.mark.parametrize("d", [50, 64])
def test_ranking_metrics(device, d):
    s = _setup(device, d)
    data = _held_out(s, np.random.default_rng(17))
    names = s.h.RANKING_METRIC_NAMES
    assert names == s.tt.RANKING_METRIC_NAMES
    s.weights(True)
    hit = False
    for k, exclude, min_rating in ((10, None, None), (10, s.train, None), (5, s.foreign, 3.0), (100, None, 2.0)):
        kept = data if min_rating is None else data[data["average_review_rating"] >= min_rating]
        users = sorted(set(kept["userId"].tolist()))
        lists = s.h.recommend_for_users(users, s.cand, k, exclude=exclude)
        assert lists["userId"].tolist() == users
        _assert_frame(lists, users, s, k, True, exclude)
        labs = [sorted(set(kept["itemId"][kept["userId"] == u].tolist())) for u in users]
        exp = mean_metrics([[i for i, _ in rec] for rec in lists["recommendations"]], labs, k)
        res = s.h.ranking_metrics(data, s.cand if k != 5 else s.frame, k=k, min_rating=min_rating, exclude=exclude)
        assert set(res) == set(names) | {"count"} and res["count"] == len(users)
        for name, e in zip(ORACLE_ORDER, exp):
            np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0, err_msg=f"{name} k={k}")
        hit = hit or exp[0] > 0
        for name in names:
            got = s.h.evaluate_ranking(data, s.cand, metric_name=name, k=k, min_rating=min_rating, exclude=exclude)
            assert isinstance(got, float) and got == res[name]
    assert hit  # the lists do hit the held-out items
    none = s.h.ranking_metrics(data, s.cand, min_rating=99.0)
    assert none["count"] == 0 and all(np.isnan(none[name]) for name in names)
