"""GPU: TwoTowerModel.recommend_for_users / recommend_for_all_users /
ranking_metrics / evaluate_ranking / candidates.

Models come straight from build_model() with a fixed seed (LayerNorm makes the
scores vary); the scaler is fitted on the item frame. Two configurations: d =
64 with 20,000 candidates and 40 users (the fused matrix-core top-k, sampled
path), d = 50 with 3,000 candidates and 12 users (the materialised
hrec_tt_score chain). The candidate frame is shuffled and holds two rows with
identical features and embedding rows but distinct itemIds (a tie).

Expected lists: for each user predict_for_user(u, frame), Python's
sorted(..., key=score, reverse=True), the excluded itemIds removed, cut to n.
itemIds and f32 score bits are compared exactly.

Ranking metrics: tests/ranking_oracle.mean_metrics over the expected lists, at
rtol 1e-12 as tests/test_gpu_als_recommend.py compares the same quantities
(means of a few dozen per-row values that are themselves exact; the oracle's
math.log gain table and the wrapper's numpy one may differ in the last bit)."""
import copy

import numpy as np
import pandas as pd
import pytest
from ranking_oracle import mean_metrics
from sklearn.preprocessing import MinMaxScaler

pytestmark = pytest.mark.gpu

ORACLE_ORDER = ("precisionAtK", "recallAtK", "meanAveragePrecision", "meanAveragePrecisionAtK", "ndcgAtK")


def _item_frame(rng, n_items, n_man, n_cat):
    ids = rng.permutation(n_items).astype(np.int64)  # shuffled: frame row != itemId order
    frame = pd.DataFrame({"itemId": ids, "manufacturer_id": rng.integers(0, n_man, n_items),
                          "category_id": rng.integers(0, n_cat, n_items), "price": rng.random(n_items) * 100,
                          "average_review_rating": rng.integers(0, 11, n_items).astype(np.float64) / 2})
    a, b = n_items // 3, n_items // 3 + 11  # the tied pair: identical features in two rows
    for c in ("manufacturer_id", "category_id", "price", "average_review_rating"):
        frame.loc[b, c] = frame.loc[a, c]
    return frame, (a, b)


class Setup:
    def __init__(self, device, d, n_items, n_users, seed):
        from src.two_tower_model import TwoTowerModel

        rng = np.random.default_rng(seed)
        self.n_users, self.n_items = n_users, n_items
        self.tt = TwoTowerModel(n_users, n_items + 8, 30, 10, embedding_size=d, seed=seed)
        self.tt.build_model()
        self.frame, (a, b) = _item_frame(rng, n_items, 30, 10)
        emb = self.tt.model.tensors["item_emb"]
        emb[int(self.frame["itemId"][b])] = emb[int(self.frame["itemId"][a])]  # same embedding row: a true tie
        self.tie = (int(self.frame["itemId"][a]), int(self.frame["itemId"][b]))
        self.tt.scaler = MinMaxScaler().fit(self.frame[["price", "average_review_rating"]])
        # the reference ranking of every user, computed once
        self.ranked = {}
        for u in range(n_users):
            preds = self.tt.predict_for_user(u, self.frame)
            self.ranked[u] = sorted(preds, key=lambda x: x[1], reverse=True)
        # exclusion pairs: a random 30 % per user (user 3: its own top 100 as well); user 2
        # nothing; plus users outside the table, items outside the frame, and repeated pairs.
        # Every user keeps far more than kk unseen sample items, so at d = 64 one fused call
        # answers. exclude_all adds every item for user 1: that user has no bound, its chunk
        # overflows in both rounds and the materialised chain answers it.
        ids = self.frame["itemId"].to_numpy()
        eu, ei = [], []
        for u in range(n_users):
            if u == 2:
                continue
            picks = ids[rng.random(n_items) < 0.3]
            if u == 3:
                picks = np.concatenate([picks, [i for i, _ in self.ranked[u][:100]]])
            eu.append(np.full(len(picks), u))
            ei.append(picks)
        eu.append(np.array([n_users + 5, -3, 0, 4]))
        ei.append(np.array([int(ids[0]), int(ids[1]), n_items + 100, -1]))
        eu, ei = np.concatenate(eu), np.concatenate(ei)
        eu, ei = np.concatenate([eu, eu[:50]]), np.concatenate([ei, ei[:50]])
        order = rng.permutation(len(eu))
        self.exclude = pd.DataFrame({"userId": eu[order], "itemId": ei[order]})
        self.gone = {u: set() for u in range(n_users)}
        for u, i in zip(eu.tolist(), ei.tolist()):
            if 0 <= u < n_users:
                self.gone[u].add(i)
        self.exclude_all = pd.concat([self.exclude, pd.DataFrame({"userId": np.full(n_items, 1), "itemId": ids})],
                                     ignore_index=True).sample(frac=1.0, random_state=9).reset_index(drop=True)
        self.gone_all = dict(self.gone)
        self.gone_all[1] = set(ids.tolist())

    def expected(self, u, n, exclude):
        """exclude: False, True (self.exclude) or "all" (self.exclude_all)."""
        lst = self.ranked[u]
        if exclude:
            gone = self.gone_all[u] if exclude == "all" else self.gone[u]
            lst = [p for p in lst if p[0] not in gone]
        return lst[:n]

    def frame_of(self, exclude):
        return {False: None, True: self.exclude, "all": self.exclude_all}[exclude]


_CACHE = {}


def _setup(device, d):
    if d not in _CACHE:
        _CACHE[d] = Setup(device, 64, 20_000, 40, seed=4) if d == 64 else Setup(device, 50, 3_000, 12, seed=5)
    return _CACHE[d]


def _assert_frame(df, users, s, n, exclude):
    assert list(df.columns) == ["userId", "recommendations"]
    assert df["userId"].tolist() == list(users)
    for u, rec in zip(users, df["recommendations"]):
        exp = s.expected(u, n, exclude)
        assert [i for i, _ in rec] == [i for i, _ in exp], f"user {u}"
        got_bits = np.asarray([r for _, r in rec], np.float32).view(np.int32)
        exp_bits = np.asarray([r for _, r in exp], np.float32).view(np.int32)
        np.testing.assert_array_equal(got_bits, exp_bits, err_msg=f"user {u}")


def _no_chain(monkeypatch):
    """The materialised chain's masking step raises: what passes under this
    came from hrec_dot_topk_excluding's fused output alone."""
    from src import _hrec

    def boom(*a, **k):
        raise AssertionError("the materialised chain ran")

    monkeypatch.setattr(_hrec, "mask_rows", boom)


@pytest.mark.parametrize("d", [64, 50])
def test_lists_match_predict_for_user(device, d, monkeypatch):
    s = _setup(device, d)
    t0, t1 = s.tie
    r0 = dict(s.ranked[0])
    assert np.float32(r0[t0]).view(np.int32) == np.float32(r0[t1]).view(np.int32)  # the tie is real
    cand = s.tt.candidates(s.frame)
    assert len(cand) == s.n_items and cand.vectors.shape == (s.n_items, d)
    users = list(range(s.n_users))
    query = np.array(users[::-1] + [3, 3, 0])  # unordered, repeated: distinct and ascending in the result
    with monkeypatch.context() as mp:
        if d == 64:  # every user keeps a bound: the fused entry answers, never the chain
            _no_chain(mp)
        for n in (1, 10, 100):
            _assert_frame(s.tt.recommend_for_users(query, s.frame, n), users, s, n, False)
            _assert_frame(s.tt.recommend_for_users(pd.DataFrame({"userId": query}), cand, n, exclude=s.exclude),
                          users, s, n, True)
        sub = [5, 3, 9]
        _assert_frame(s.tt.recommend_for_users(sub, cand, 10, exclude=s.exclude), sorted(sub), s, 10, True)
        for excl in (None, s.exclude):
            a = s.tt.recommend_for_all_users(cand, 10, exclude=excl)
            b = s.tt.recommend_for_users(np.arange(s.n_users), cand, 10, exclude=excl)
            assert a["userId"].tolist() == b["userId"].tolist() == users
            assert a["recommendations"].tolist() == b["recommendations"].tolist()
    # a user with everything excluded, in calls of its own: the row stays, empty
    df = s.tt.recommend_for_users([1, 2], cand, 10, exclude=s.exclude_all)
    assert df["recommendations"][0] == []
    assert len(df["recommendations"][1]) == 10       # nothing excluded
    for n in (1, 100):
        _assert_frame(s.tt.recommend_for_all_users(cand, n, exclude=s.exclude_all), users, s, n, "all")


@pytest.mark.parametrize("d", [64, 50])
def test_errors(device, d):
    s = _setup(device, d)
    cand = s.tt.candidates(s.frame)
    for bad in ([0, s.n_users], [-1]):
        with pytest.raises(IndexError, match="user_in: id out of range"):
            s.tt.recommend_for_users(bad, cand, 5)
    for n in (0, 1025):
        with pytest.raises(ValueError):
            s.tt.recommend_for_users([0], cand, n)
    dup = pd.concat([s.frame.iloc[:20], s.frame.iloc[5:6]], ignore_index=True)
    with pytest.raises(ValueError, match="repeats an itemId"):
        s.tt.recommend_for_users([0], dup, 5)
    with pytest.raises(ValueError, match="metric_name"):
        s.tt.evaluate_ranking(pd.DataFrame({"userId": [0], "itemId": [1]}), cand, metric_name="auc")
    with pytest.raises(IndexError, match="user_in: id out of range"):
        s.tt.ranking_metrics(pd.DataFrame({"userId": [0, s.n_users], "itemId": [1, 2]}), cand)


def test_stale_candidates_raise(device):
    from src.two_tower_model import TwoTowerModel

    rng = np.random.default_rng(8)
    tt = TwoTowerModel(10, 60, 5, 4, embedding_size=32, seed=1)
    tt.build_model()
    frame, _ = _item_frame(rng, 50, 5, 4)
    tt.scaler = MinMaxScaler().fit(frame[["price", "average_review_rating"]])
    cand = tt.candidates(frame)
    assert len(tt.recommend_for_users([0, 1], cand, 5)) == 2
    train = frame.iloc[:16].assign(userId=np.arange(16) % 10)
    fitted = copy.deepcopy(tt.scaler)  # _prepare_features refits the model's scaler object in place
    feats = tt._prepare_features(train)  # refits the scaler on 16 rows: predict_for_user's inputs change
    with pytest.raises(RuntimeError, match="another scaler fit"):
        tt.recommend_for_users([0, 1], cand, 5)
    tt.scaler = fitted
    assert len(tt.recommend_for_users([0, 1], cand, 5)) == 2  # the same parameters again: fine
    dev_in = tt._device_inputs(feats)
    import torch

    y = torch.as_tensor(train["average_review_rating"].to_numpy(np.float32), device=tt.model.device)
    tt.fit_batches(dev_in, y, [np.arange(16)])
    with pytest.raises(RuntimeError, match="other weights"):
        tt.recommend_for_users([0, 1], cand, 5)  # a training step moved the weights
    other = TwoTowerModel(10, 60, 5, 4, embedding_size=32, seed=1)
    other.build_model()
    other.scaler = tt.scaler
    with pytest.raises(RuntimeError, match="other weights"):
        other.candidates(cand)
    assert len(tt.recommend_for_users([0, 1], tt.candidates(frame), 5)) == 2  # rebuilt: fine


def _held_out(s, rng):
    """A held-out frame: per user (all but users 6 and 7) two of its top 10
    (unfiltered), two random items and, for user 0, an item absent from the
    catalogue; ratings 1 .. 5."""
    ids = s.frame["itemId"].to_numpy()
    rows = []
    for u in range(s.n_users):
        if u in (6, 7):
            continue
        items = [s.ranked[u][1][0], s.ranked[u][7][0]] + rng.choice(ids, 2).tolist()
        if u == 0:
            items.append(s.n_items + 3)
        rows += [(u, int(i), float(rng.integers(1, 6))) for i in items]
    df = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
    return df.sample(frac=1.0, random_state=3).reset_index(drop=True)


def _oracle(s, data, k, exclude, min_rating=None):
    """exclude as Setup.expected takes it."""
    if min_rating is not None:
        data = data[data["average_review_rating"] >= min_rating]
    users = sorted(set(data["userId"].tolist()))
    lists = [[i for i, _ in s.expected(u, k, exclude)] for u in users]
    labs = [sorted(set(data["itemId"][data["userId"] == u].tolist())) for u in users]
    return mean_metrics(lists, labs, k), len(users)


@pytest.mark.parametrize("d", [64, 50])
def test_ranking_metrics(device, d, monkeypatch):
    s = _setup(device, d)
    data = _held_out(s, np.random.default_rng(17))
    cand = s.tt.candidates(s.frame)
    names = s.tt.RANKING_METRIC_NAMES
    from src.als_model import ALSModel

    assert names == ALSModel.RANKING_METRIC_NAMES
    for k, exclude, min_rating in ((10, False, None), (10, True, None), (5, True, 3.0), (100, False, 2.0),
                                   (10, "all", None)):
        exp, count = _oracle(s, data, k, exclude, min_rating)
        with monkeypatch.context() as mp:
            if d == 64 and exclude != "all":  # the fused entry's lists, never the chain's
                _no_chain(mp)
            res = s.tt.ranking_metrics(data, cand if k != 5 else s.frame, k=k, min_rating=min_rating,
                                       exclude=s.frame_of(exclude))
            assert set(res) == set(names) | {"count"} and res["count"] == count
            for name, e in zip(ORACLE_ORDER, exp):
                np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0, err_msg=f"{name} k={k}")
            for name in names:
                got = s.tt.evaluate_ranking(data, cand, metric_name=name, k=k, min_rating=min_rating,
                                            exclude=s.frame_of(exclude))
                assert got == res[name]
    assert _oracle(s, data, 100, False, 2.0)[0][0] > 0  # the lists do hit the held-out items
    # the label CSR built on the device gives the same numbers
    host = s.tt.ranking_metrics(data, cand, k=10, exclude=s.exclude)
    old = s.tt.RANKING_HOST_ROWS
    try:
        type(s.tt).RANKING_HOST_ROWS = 0
        assert s.tt.ranking_metrics(data, cand, k=10, exclude=s.exclude) == host
    finally:
        type(s.tt).RANKING_HOST_ROWS = old


def test_exclusion_built_on_device_matches_host(device):
    s = _setup(device, 50)
    cand = s.tt.candidates(s.frame)
    host = s.tt.recommend_for_all_users(cand, 10, exclude=s.exclude)
    old = s.tt.EXCLUSION_HOST_PAIRS
    try:
        type(s.tt).EXCLUSION_HOST_PAIRS = 0
        devb = s.tt.recommend_for_all_users(cand, 10, exclude=s.exclude)
    finally:
        type(s.tt).EXCLUSION_HOST_PAIRS = old
    assert host["recommendations"].tolist() == devb["recommendations"].tolist()
