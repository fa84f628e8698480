"""GPU: the per-user F1-adaptive fusion of HybridRecommendationSystem's batched
methods (actual=, f1_k=), evaluate_models and fit_fusion_weights.

The models are test_gpu_hybrid_recommend's Setup (60 users x 300 shuffled
candidates, cold users, unknown items; d = 50 and 64). The expected list of
user u is the reference's per-user route: a = als.predict_for_user(u, ids),
t = tt.predict_for_user(u, frame); the instance's two scores set to
compute_f1_score(actual_u, dict(a)) and compute_f1_score(actual_u, dict(t))
(a user without rows in `actual` keeps the scores the instance had);
sorted(adaptive_fusion(a, t), by score, descending), the excluded pairs
removed, cut to n. Item ids and f64 score bits are compared exactly.

`actual`: users with u % 3 == 0 hold the ALS side's own top 10, users with
u % 3 == 1 the two-tower side's own top 10 — so the first kind is fused with
(0.8, 0.2) and the second with (0.2, 0.8) whatever the instance holds, which
the test asserts — and users with u % 3 == 2 have no rows. Some users also
hold items outside the candidate frame, pairs are repeated, a user outside
the user table and an extra column are present."""
import numpy as np
import pandas as pd
import pytest
import torch
from ranking_oracle import mean_metrics
from test_gpu_hybrid_recommend import N_ITEMS, N_USERS, ORACLE_ORDER, WEIGHTS, _assert_frame, _bits, _setup

pytestmark = pytest.mark.gpu

SUB = 7  # users per sub-batch


class Case:
    """Per Setup: both models' per-user predictions, the `actual` frame and
    each user's own F1 pair (computed once)."""

    def __init__(self, s):
        from src.als_model import compute_f1_score

        self.s = s
        self.preds, self.sets, self.f1 = {}, {}, {}
        rows = []
        for u in range(N_USERS):
            a = s.als.predict_for_user(u, s.frame["itemId"].to_numpy())
            t = s.tt.predict_for_user(u, s.frame)
            assert len(a) == len(t) == N_ITEMS
            self.preds[u] = (a, t)
            if u % 3 == 2:
                continue
            side = dict(a if u % 3 == 0 else t)
            items = [i for i, _ in sorted(side.items(), key=lambda x: x[1], reverse=True)[:10]]
            if u % 4 == 0:
                items += [N_ITEMS + 50 + u, N_ITEMS + 200]  # outside the candidate frame: recall's denominator only
            self.sets[u] = {int(i) for i in items}
            rows += [(u, int(i)) for i in items] + [(u, int(items[0]))]  # a repeated pair
        rows += [(N_USERS + 5, int(s.ids[0])), (N_USERS + 5, int(s.ids[1]))]  # a user outside the table
        df = pd.DataFrame(rows, columns=["userId", "itemId"])
        df["average_review_rating"] = 3.0
        self.actual = df.sample(frac=1.0, random_state=5).reset_index(drop=True)
        for u, items in self.sets.items():
            act = {i: 1.0 for i in items}
            a, t = self.preds[u]
            self.f1[u] = (compute_f1_score(act, dict(a)), compute_f1_score(act, dict(t)))
        self._ranked = {}

    def wins(self, u, default):
        return self.f1[u][0] > self.f1[u][1] if u in self.f1 else default

    def ranked(self, u, default):
        """The reference's route for user u with the instance at WEIGHTS[default]."""
        key = (u, self.wins(u, default))
        if key not in self._ranked:
            h = self.s.h
            saved = h.als_f1_score, h.twotower_f1_score
            h.als_f1_score, h.twotower_f1_score = self.f1.get(u, WEIGHTS[default])
            fused = h.adaptive_fusion(*self.preds[u])
            h.als_f1_score, h.twotower_f1_score = saved
            ranked = sorted(fused, key=lambda x: x[1], reverse=True)
            assert len(ranked) == N_ITEMS and len(set(x for _, x in ranked)) == N_ITEMS, f"user {u}: tied fused scores"
            self._ranked[key] = ranked
        return self._ranked[key]

    def expected(self, u, n, default, exclude=None):
        lst = self.ranked(u, default)
        if exclude is not None:
            gone = set(exclude["itemId"][exclude["userId"] == u].tolist())
            lst = [p for p in lst if p[0] not in gone]
        return lst[:n]


_CASES = {}


def _case(device, d):
    if d not in _CASES:
        _CASES[d] = Case(_setup(device, d))
    return _CASES[d]


def _assert_lists(df, users, c, n, default, exclude=None):
    assert list(df.columns) == ["userId", "recommendations"]
    assert df["userId"].tolist() == list(users)
    for u, rec in zip(users, df["recommendations"]):
        exp = c.expected(u, n, default, exclude)
        assert [i for i, _ in rec] == [i for i, _ in exp], f"user {u}"
        np.testing.assert_array_equal(_bits([r for _, r in rec]), _bits([r for _, r in exp]), err_msg=f"user {u}")


@pytest.mark.parametrize("d", [50, 64])
def test_batch_holds_all_three_kinds(device, d):
    c = _case(device, d)
    for u in range(N_USERS):
        if u % 3 == 0:
            assert c.f1[u][0] > c.f1[u][1], u      # its labels are the ALS side's own top 10
        elif u % 3 == 1:
            assert not c.f1[u][0] > c.f1[u][1], u  # the two-tower side's
            assert c.f1[u][1] > 0
        else:
            assert u not in c.f1                   # no rows: the instance's weights
    assert any(c.f1[u][0] < 1.0 for u in range(0, N_USERS, 12))  # items outside the frame lower recall
    # the fused lists do depend on the choice
    for u in (0, 1, 50, 52):
        s = c.s
        assert [i for i, _ in s.per_user(u, True)[:10]] != [i for i, _ in s.per_user(u, False)[:10]]


@pytest.mark.parametrize("default", [True, False])
@pytest.mark.parametrize("d", [50, 64])
def test_lists_match_per_user(device, d, default, monkeypatch):
    c = _case(device, d)
    s = c.s
    users = list(range(N_USERS))
    monkeypatch.setitem(s.h.__dict__, "RECOMMEND_SCORE_BYTES", 8 * N_ITEMS * SUB)  # several sub-batches
    for n, exclude, f1_k in ((5, None, 10), (40, s.train, 10), (1024, s.foreign, 10)):
        s.weights(default)
        df = s.h.recommend_for_users(users[::-1] + [3, 3], s.cand if n != 5 else s.frame, n, exclude=exclude,
                                     actual=c.actual, f1_k=f1_k)
        _assert_lists(df, users, c, n, default, exclude)
        assert (s.h.als_f1_score, s.h.twotower_f1_score) == WEIGHTS[default]  # untouched
    s.weights(default)
    _assert_lists(s.h.recommend_for_users([5, 55, 9, 30, 31], s.cand, 10, actual=c.actual), [5, 9, 30, 31, 55], c, 10,
                  default)
    a = s.h.recommend_for_all_users(s.cand, 10, exclude=s.train, actual=c.actual)
    _assert_lists(a, users, c, 10, default, s.train)
    # actual=None: what the parent gives
    _assert_frame(s.h.recommend_for_users(users, s.cand, 10, exclude=s.train), users, s, 10, default, s.train)
    _assert_frame(s.h.recommend_for_users(users, s.cand, 10, actual=None, f1_k=3), users, s, 10, default)
    # an `actual` without any queried user changes nothing
    other = pd.DataFrame({"userId": [N_USERS + 1, 58], "itemId": [int(s.ids[0]), int(s.ids[1])]})
    _assert_frame(s.h.recommend_for_users(users[:50], s.cand, 10, actual=other), users[:50], s, 10, default)


def test_other_f1_k(device):
    """f1_k = 3 and f1_k = 300 (= every candidate: both models find the same
    labels, so nobody's ALS F1 is strictly larger)."""
    from src.als_model import compute_f1_score

    c = _case(device, 64)
    s = c.s
    users = list(range(N_USERS))
    for f1_k in (3, N_ITEMS):
        s.weights(True)
        df = s.h.recommend_for_users(users, s.cand, 10, actual=c.actual, f1_k=f1_k)
        for u, rec in zip(users, df["recommendations"]):
            if u in c.sets:
                act = {i: 1.0 for i in c.sets[u]}
                a, t = c.preds[u]
                w = compute_f1_score(act, dict(a), k=f1_k) > compute_f1_score(act, dict(t), k=f1_k)
                assert f1_k != N_ITEMS or not w
            else:
                w = True
            exp = s.per_user(u, w)[:10]
            assert [i for i, _ in rec] == [i for i, _ in exp], f"user {u}"
            np.testing.assert_array_equal(_bits([r for _, r in rec]), _bits([r for _, r in exp]), err_msg=f"user {u}")


@pytest.mark.parametrize("d", [50, 64])
def test_redo_routes(device, d, monkeypatch):
    """A raised F1 flag redoes the sub-batch whole (F1 in mode 1, then the
    lists); a raised lists flag alone redoes the lists in mode 1."""
    from src import _hrec

    c = _case(device, d)
    s = c.s
    users = list(range(N_USERS))
    monkeypatch.setitem(s.h.__dict__, "RECOMMEND_SCORE_BYTES", 8 * N_ITEMS * SUB)
    real_f1, real_lists = _hrec.hybrid_model_f1, _hrec.hybrid_lists_rowwise
    calls = []

    def f1_over(als, tt, *a, **k):
        calls.append(("f1", als.shape[0], k.get("mode", 0)))
        res = real_f1(als, tt, *a, **k)
        if k.get("mode", 0) == 0 and len([x for x in calls if x[0] == "f1" and x[2] == 0]) % 2:  # every other sub-batch
            res[1].fill_(1 - int(res[1][0]))
            res[2].fill_(1)
        return res

    def lists_over(als, tt, *a, **k):
        calls.append(("lists", als.shape[0], k.get("mode", 0)))
        res = real_lists(als, tt, *a, **k)
        if k.get("mode", 0) == 0:
            res[0].zero_()
            res[3].fill_(1)
        return res

    s.weights(True)
    monkeypatch.setattr(_hrec, "hybrid_model_f1", f1_over)
    _assert_lists(s.h.recommend_for_users(users, s.cand, 40, exclude=s.train, actual=c.actual), users, c, 40, True,
                  s.train)
    first = [x for x in calls if x[2] == 0 and x[0] == "f1"]
    assert [x[1] for x in first[:9]] == [SUB] * 8 + [4]
    redo = [x for x in calls if x[0] == "f1" and x[2] == 1]
    assert [x[1] for x in redo] == [3, 3, 1] * 4 + [3, 1]        # sub-batches 0, 2, 4, 6, 8 in pieces of 3
    calls.clear()
    monkeypatch.setattr(_hrec, "hybrid_model_f1", real_f1)
    monkeypatch.setattr(_hrec, "hybrid_lists_rowwise", lists_over)
    _assert_lists(s.h.recommend_for_users(users, s.cand, 40, actual=c.actual), users, c, 40, True)
    assert [x[1:] for x in calls if x[2] == 0] == [(SUB, 0)] * 8 + [(4, 0)]
    assert [x[1] for x in calls if x[2] == 1] == [3, 3, 1] * 8 + [3, 1]


@pytest.mark.parametrize("d", [50, 64])
def test_evaluate_models_and_fit(device, d, monkeypatch):
    from src.als_model import compute_f1_score

    c = _case(device, d)
    s = c.s
    s.weights(True)
    data = c.actual[c.actual["userId"] < N_USERS]
    monkeypatch.setitem(s.h.__dict__, "RECOMMEND_SCORE_BYTES", 8 * N_ITEMS * SUB)
    for k in (10, 3):
        df = s.h.evaluate_models(data, s.cand if k == 10 else s.frame, k=k)
        assert list(df.columns) == ["userId", "als_f1", "twotower_f1", "als_wins"]
        assert df["userId"].tolist() == sorted(c.sets)
        assert [df[col].dtype for col in ("als_f1", "twotower_f1", "als_wins")] == [np.float64, np.float64, bool]
        for u, fa, ft, w in zip(df["userId"], df["als_f1"], df["twotower_f1"], df["als_wins"]):
            act = {i: 1.0 for i in c.sets[u]}
            ea, et = (compute_f1_score(act, dict(p), k=k) for p in c.preds[u])
            assert _bits(fa) == _bits(float(ea)) and _bits(ft) == _bits(float(et)), (u, k)
            assert bool(w) == (ea > et)
            if k == 10:
                assert (ea, et) == c.f1[u]
        assert (s.h.als_f1_score, s.h.twotower_f1_score) == WEIGHTS[True]  # untouched
    df = s.h.evaluate_models(data, s.cand)
    try:
        got = s.h.fit_fusion_weights(data, s.cand)
        exp = (np.mean(df["als_f1"].to_numpy()), np.mean(df["twotower_f1"].to_numpy()))
        assert _bits(got[0]) == _bits(exp[0]) and _bits(got[1]) == _bits(exp[1])
        assert (s.h.als_f1_score, s.h.twotower_f1_score) == got
        with pytest.raises(ValueError, match="holds no user"):
            s.h.fit_fusion_weights(data.iloc[:0], s.cand)
        assert (s.h.als_f1_score, s.h.twotower_f1_score) == got
    finally:
        s.weights(True)
    empty = s.h.evaluate_models(data.iloc[:0], s.cand)
    assert list(empty.columns) == ["userId", "als_f1", "twotower_f1", "als_wins"] and len(empty) == 0
    with pytest.raises(IndexError, match="user_in: id out of range"):
        s.h.evaluate_models(c.actual, s.cand)  # holds a user outside the table
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k must be in"):
            s.h.evaluate_models(data, s.cand, k=k)


@pytest.mark.parametrize("d", [50, 64])
def test_ranking_metrics(device, d):
    c = _case(device, d)
    s = c.s
    rng = np.random.default_rng(23)
    rows = []
    for u in range(N_USERS):
        if u in (6, 7):
            continue
        top = c.ranked(u, False)
        rows += [(u, int(i)) for i in [top[1][0], top[7][0]] + rng.choice(s.ids, 2).tolist()]
    data = pd.DataFrame(rows, columns=["userId", "itemId"]).sample(frac=1.0, random_state=3).reset_index(drop=True)
    names = s.h.RANKING_METRIC_NAMES
    s.weights(False)
    for k, exclude in ((10, None), (5, s.train)):
        users = sorted(set(data["userId"].tolist()))
        lists = s.h.recommend_for_users(users, s.cand, k, exclude=exclude, actual=c.actual)
        _assert_lists(lists, users, c, k, False, exclude)
        labs = [sorted(set(data["itemId"][data["userId"] == u].tolist())) for u in users]
        exp = mean_metrics([[i for i, _ in rec] for rec in lists["recommendations"]], labs, k)
        res = s.h.ranking_metrics(data, s.cand, k=k, exclude=exclude, actual=c.actual)
        assert set(res) == set(names) | {"count"} and res["count"] == len(users)
        for name, e in zip(ORACLE_ORDER, exp):
            np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0, err_msg=f"{name} k={k}")
        assert exp[0] > 0
        plain = s.h.ranking_metrics(data, s.cand, k=k, exclude=exclude)
        assert any(plain[name] != res[name] for name in names)  # the per-user weights do change the lists
        for name in names:
            got = s.h.evaluate_ranking(data, s.cand, metric_name=name, k=k, exclude=exclude, actual=c.actual)
            assert isinstance(got, float) and got == res[name]


def test_label_totals_host_and_device(device):
    """ranked_lists.distinct_counts: the host and the device route agree
    (repeated pairs once, rows outside the keys dropped, negative ids)."""
    from src import ranked_lists

    rng = np.random.default_rng(29)
    keys = np.array([-4, 0, 3, 7, 8, 1000], np.int64)
    rows = rng.choice([-4, -1, 0, 3, 5, 7, 1000, 2000], 500)
    items = rng.integers(-20, 20, 500)
    exp = [len({int(i) for r, i in zip(rows, items) if r == q}) for q in keys]
    assert exp[4] == 0 and min(exp[:4]) > 1
    for host_rows in (1 << 16, 0):
        got = ranked_lists.distinct_counts(keys, rows, items, device, host_rows)
        assert got.dtype == torch.int32 and got.tolist() == exp
    assert ranked_lists.distinct_counts(keys[:0], rows, items, device, 0).numel() == 0
    assert ranked_lists.distinct_counts(keys, rows[:0], items[:0], device, 0).tolist() == [0] * 6


def test_errors(device):
    c = _case(device, 50)
    s = c.s
    s.weights(True)
    data = pd.DataFrame({"userId": [0], "itemId": [1]})
    for f1_k in (0, -1, 1025):
        for call in (lambda: s.h.recommend_for_users([0], s.cand, 5, actual=c.actual, f1_k=f1_k),
                     lambda: s.h.recommend_for_all_users(s.cand, 5, actual=c.actual, f1_k=f1_k),
                     lambda: s.h.ranking_metrics(data, s.cand, actual=c.actual, f1_k=f1_k),
                     lambda: s.h.evaluate_ranking(data, s.cand, actual=c.actual, f1_k=f1_k)):
            with pytest.raises(ValueError, match="f1_k must be in"):
                call()
    with pytest.raises(IndexError, match="user_in: id out of range"):
        s.h.recommend_for_users([0, N_USERS], s.cand, 5, actual=c.actual)
    feats = s.als.item_features
    try:
        s.als.item_features = None
        with pytest.raises(ValueError, match="unknown to the ALS model"):
            s.h.recommend_for_users([0], s.frame, 5, actual=c.actual)
        with pytest.raises(ValueError, match="unknown to the ALS model"):
            s.h.evaluate_models(data, s.frame)
    finally:
        s.als.item_features = feats
    assert len(s.h.recommend_for_users([], s.cand, 5, actual=c.actual)) == 0
