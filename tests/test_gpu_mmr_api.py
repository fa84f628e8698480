"""GPU: the diversify= keyword (ranked_lists.MMR) of the three models' list and
metric methods and RecommenderEvaluator.diversify_lists, against the numpy
oracle (tests/mmr_oracle.py) applied to each model's own public top-40 frame.

The small fitted models of tests/test_gpu_list_quality_api.py (40 users x 60
items; ALS rank 8 trained on users 0 .. 35 and 54 items; two-tower
embedding_size 50 and 64). A list whose oracle gap is under 1e3 * tol is held
to the validity check of tests/test_gpu_mmr.py (a) instead of exact equality,
so every list is checked."""
import numpy as np
import pandas as pd
import pytest
from ranking_oracle import mean_metrics

import list_quality_oracle as lq
import mmr_oracle as mo
from test_gpu_list_quality_api import EXACT, K, MEANS, N_ITEMS, N_USERS, N_WARM, _setup, check

pytestmark = pytest.mark.gpu

POOL = 40
RANKING_ORDER = ("precisionAtK", "recallAtK", "meanAveragePrecision", "meanAveragePrecisionAtK", "ndcgAtK")


def _mmr(lam=0.5, pool=POOL):
    from src.ranked_lists import MMR

    return MMR(lam, pool)


def _inv(vectors):
    """The kernel's own inverse norms of the vectors, read back."""
    import torch
    from src import _hrec

    return _hrec.row_inv_norms(torch.as_tensor(np.ascontiguousarray(vectors, np.float32), device="cuda")).cpu().numpy()


def _bits(x):
    return np.float64(x).tobytes()


def check_lists(div, pool, item_ids, vectors, lam, num):
    """div: the diversified frame, pool: the model's plain frame of the pool
    (same users, same exclude). Subset, rating bits, and the oracle's lists."""
    assert div.iloc[:, 0].tolist() == pool.iloc[:, 0].tolist()
    col = {int(i): c for c, i in enumerate(item_ids)}
    recs = list(pool["recommendations"])
    width = max(len(r) for r in recs)
    cols = np.full((len(recs), width), -1, np.int64)
    scores = np.full((len(recs), width), np.nan)
    lens = np.array([len(r) for r in recs], np.int32)
    for r, rec in enumerate(recs):
        cols[r, : len(rec)] = [col.get(int(i), -1) for i, _ in rec]
        scores[r, : len(rec)] = [s for _, s in rec]
    vectors = np.ascontiguousarray(vectors, np.float32)
    inv = _inv(vectors)
    d = vectors.shape[1]
    want = mo.mmr(cols, scores, vectors, inv, lam, num, pool_len=lens)
    got_pos = np.full((len(recs), num), -1, np.int64)
    for r, (rec, out) in enumerate(zip(recs, div["recommendations"])):
        rating = {int(i): s for i, s in rec}
        place = {int(i): p for p, (i, _) in enumerate(rec)}
        assert len(out) == want.len[r] == min(num, len(rec)), r
        assert len({int(i) for i, _ in out}) == len(out)
        for i, s in out:
            assert int(i) in rating and _bits(s) == _bits(rating[int(i)]), (r, i)
        got_pos[r, : len(out)] = [place[int(i)] for i, _ in out]
    rep = mo.mmr(cols, scores, vectors, inv, lam, num, pool_len=lens, forced=got_pos)
    exact = want.gap > 1e3 * mo.tol(d)
    print("lists", len(recs), "compared exactly", int(exact.sum()), "max deficit", rep.deficit.max(), "tol", mo.tol(d))
    assert np.array_equal(got_pos[exact], want.pos[exact])
    assert rep.deficit.max() <= mo.tol(d)  # every list, the exact ones included
    return got_pos


def check_quality(got, ev, frame, item_ids, vectors, history):
    """list_quality_metrics(diversify=) against the oracle over the returned
    frame and against evaluate_lists of it: integers exactly, the float
    columns within the per-list bound plus the summations' (check's bounds)."""
    check(dict(got), frame, item_ids, vectors, K, history)
    check(dict(ev), frame, item_ids, vectors, K, history)
    for name in EXACT:
        assert got[name] == ev[name] or (np.isnan(got[name]) and np.isnan(ev[name])), name
    d, rows = vectors.shape[1], len(frame)
    for name in MEANS + ("distributionalCoverage",):
        if np.isnan(ev[name]):
            assert np.isnan(got[name])
            continue
        bound = (8 * (d + 2 * K + 64) + 2 * rows + N_ITEMS) * lq.U53 * max(1.0, abs(ev[name]))
        assert abs(got[name] - ev[name]) <= bound, (name, got[name], ev[name])


def _held_out(users, rng):
    rows = [(int(u), int(i), float(rng.integers(1, 6))) for u in users for i in rng.choice(N_ITEMS, 6, replace=False)]
    return pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])


def check_ranking(res, frame, data, count):
    users = frame.iloc[:, 0].tolist()
    assert users == sorted(set(data["userId"].tolist())) and res["count"] == count == len(users)
    lists = [[int(i) for i, _ in rec] for rec in frame["recommendations"]]
    labs = [sorted(set(data["itemId"][data["userId"] == u].tolist())) for u in users]
    exp = mean_metrics(lists, labs, K)
    assert exp[0] > 0  # the lists do hit held-out items
    for name, e in zip(RANKING_ORDER, exp):
        np.testing.assert_allclose(res[name], e, rtol=1e-12, atol=0, err_msg=name)


def test_als(device):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, 50)
    item_ids, vec = s.als_vectors()
    plain, plain_x = s.als.recommend_for_all_users(K), s.als.recommend_for_all_users(K, exclude=s.train)
    # lambda 1 over a pool of num: the plain frames
    assert s.als.recommend_for_all_users(K, diversify=_mmr(1.0, K)).equals(plain)
    assert s.als.recommend_for_all_users(K, exclude=s.train, diversify=_mmr(1.0, K)).equals(plain_x)
    assert s.als.recommend_for_user_subset([3, 5, 1000], K, diversify=_mmr(1.0, K)).equals(
        plain[plain["userId"].isin([3, 5])].reset_index(drop=True))
    mmr = _mmr()
    for exclude in (None, s.train):
        div = s.als.recommend_for_all_users(K, exclude=exclude, diversify=mmr)
        check_lists(div, s.als.recommend_for_all_users(POOL, exclude=exclude), item_ids, vec, 0.5, K)
        sub = s.als.recommend_for_user_subset(pd.DataFrame({"userId": [7, 2, 7, 39]}), K, exclude=exclude,
                                              diversify=mmr)
        assert sub.equals(div[div["userId"].isin([2, 7])].reset_index(drop=True))
    assert not div.equals(plain_x)  # lambda 0.5 does change lists
    got = s.als.list_quality_metrics(K, exclude=s.train, history=s.train, diversify=mmr)
    assert got.pop("dropped") == 0 and got["count"] == N_WARM
    check_quality(got, RecommenderEvaluator.evaluate_lists(div, item_ids, vec, history=s.train), div, item_ids, vec,
                  s.train)
    assert s.als.evaluate_list_quality("intraListDiversity", K, exclude=s.train, history=s.train,
                                       diversify=mmr) == got["intraListDiversity"]
    base = s.als.list_quality_metrics(K, exclude=s.train, history=s.train)
    print("ALS intraListDiversity plain", base["intraListDiversity"], "MMR(0.5, 40)", got["intraListDiversity"])
    assert got["intraListDiversity"] > base["intraListDiversity"]
    data = _held_out(range(N_WARM), np.random.default_rng(3))
    res = s.als.ranking_metrics(data, k=K, exclude=s.train, diversify=mmr)
    assert res.pop("dropped") == 0
    check_ranking(res, s.als.recommend_for_user_subset(data, K, exclude=s.train, diversify=mmr), data, N_WARM)
    assert s.als.evaluate_ranking(data, "ndcgAtK", k=K, exclude=s.train, diversify=mmr) == res["ndcgAtK"]
    # num above the pool: the model ranks num, the selection reorders them
    small = s.als.recommend_for_all_users(K, diversify=_mmr(0.5, 5))
    for a, b in zip(small["recommendations"], plain["recommendations"]):
        assert sorted(a) == sorted(b) and a[0] == b[0]
    # the item side is not diversified; anything but an MMR is refused
    for call in (lambda: s.als.recommend_for_all_items(5, diversify=mmr),
                 lambda: s.als.recommend_for_item_subset([1, 2], 5, diversify=mmr)):
        with pytest.raises(ValueError):
            call()
    assert s.als.recommend_for_all_items(5).equals(s.als.recommend_for_all_items(5, diversify=None))
    for call in (lambda: s.als.recommend_for_all_users(K, diversify=0.5),
                 lambda: s.als.ranking_metrics(data, k=K, diversify="mmr"),
                 lambda: s.als.list_quality_metrics(K, diversify=(0.5, 40))):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        _mmr(0.5, 1025)


@pytest.mark.parametrize("d", [50, 64])
def test_two_tower(device, d):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, d)
    vec = s.cand.vectors.cpu().numpy()
    plain, plain_x = s.tt.recommend_for_all_users(s.cand, K), s.tt.recommend_for_all_users(s.cand, K, exclude=s.train)
    assert s.tt.recommend_for_all_users(s.cand, K, diversify=_mmr(1.0, K)).equals(plain)
    assert s.tt.recommend_for_all_users(s.frame, K, exclude=s.train, diversify=_mmr(1.0, K)).equals(plain_x)
    mmr = _mmr()
    for exclude in (None, s.train):
        div = s.tt.recommend_for_all_users(s.cand, K, exclude=exclude, diversify=mmr)
        check_lists(div, s.tt.recommend_for_all_users(s.cand, POOL, exclude=exclude), s.ids, vec, 0.5, K)
        sub = s.tt.recommend_for_users([9, 4, 9], s.frame, K, exclude=exclude, diversify=mmr)
        assert sub.equals(div[div["userId"].isin([4, 9])].reset_index(drop=True))
    assert not div.equals(plain_x)
    got = s.tt.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train, diversify=mmr)
    assert got.pop("dropped") == 0 and got["count"] == N_USERS
    check_quality(got, RecommenderEvaluator.evaluate_lists(div, s.ids, vec, history=s.train), div, s.ids, vec, s.train)
    assert s.tt.evaluate_list_quality(s.cand, "gini", K, exclude=s.train, diversify=mmr) == got["gini"]
    data = _held_out(range(0, N_USERS, 2), np.random.default_rng(4))
    res = s.tt.ranking_metrics(data, s.cand, k=K, exclude=s.train, diversify=mmr)
    check_ranking(res, s.tt.recommend_for_users(data, s.cand, K, exclude=s.train, diversify=mmr), data, N_USERS // 2)
    assert s.tt.evaluate_ranking(data, s.cand, "recallAtK", k=K, exclude=s.train, diversify=mmr) == res["recallAtK"]
    with pytest.raises(TypeError):
        s.tt.recommend_for_all_users(s.cand, K, diversify=0.7)


@pytest.mark.parametrize("d", [50, 64])
def test_hybrid(device, d):
    from src.evaluation import RecommenderEvaluator

    s = _setup(device, d)
    vec = s.cand.vectors.cpu().numpy()
    avec = s.als_vectors_in_frame_order()
    actual = s.train.iloc[::3]
    plain, plain_x = s.h.recommend_for_all_users(s.cand, K), s.h.recommend_for_all_users(s.cand, K, exclude=s.train)
    assert s.h.recommend_for_all_users(s.cand, K, diversify=_mmr(1.0, K)).equals(plain)
    assert s.h.recommend_for_all_users(s.cand, K, exclude=s.train, diversify=_mmr(1.0, K), similarity="als").equals(
        plain_x)
    assert s.h.recommend_for_all_users(s.cand, K, exclude=s.train, actual=actual, diversify=_mmr(1.0, K)).equals(
        s.h.recommend_for_all_users(s.cand, K, exclude=s.train, actual=actual))
    mmr = _mmr()
    for exclude in (None, s.train):
        pool = s.h.recommend_for_all_users(s.cand, POOL, exclude=exclude)
        div = s.h.recommend_for_all_users(s.cand, K, exclude=exclude, diversify=mmr)
        check_lists(div, pool, s.ids, vec, 0.5, K)
        div_als = s.h.recommend_for_all_users(s.cand, K, exclude=exclude, diversify=mmr, similarity="als")
        check_lists(div_als, pool, s.ids, avec, 0.5, K)
        sub = s.h.recommend_for_users([9, 4, 9], s.frame, K, exclude=exclude, diversify=mmr)
        assert sub.equals(div[div["userId"].isin([4, 9])].reset_index(drop=True))
    # the per-user fused lists
    check_lists(s.h.recommend_for_all_users(s.cand, K, exclude=s.train, actual=actual, diversify=mmr),
                s.h.recommend_for_all_users(s.cand, POOL, exclude=s.train, actual=actual), s.ids, vec, 0.5, K)
    assert not div.equals(plain_x)
    got = s.h.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train, diversify=mmr)
    assert got.pop("dropped") == 0 and got["count"] == N_USERS
    check_quality(got, RecommenderEvaluator.evaluate_lists(div, s.ids, vec, history=s.train), div, s.ids, vec, s.train)
    got_als = s.h.list_quality_metrics(s.cand, K, exclude=s.train, history=s.train, diversify=mmr, similarity="als")
    got_als.pop("dropped")
    check_quality(got_als, RecommenderEvaluator.evaluate_lists(div_als, s.ids, avec, history=s.train), div_als, s.ids,
                  avec, s.train)
    assert s.h.evaluate_list_quality(s.cand, "intraListDiversity", K, exclude=s.train, history=s.train,
                                     diversify=mmr) == got["intraListDiversity"]
    data = _held_out(range(0, N_USERS, 2), np.random.default_rng(5))
    res = s.h.ranking_metrics(data, s.cand, k=K, exclude=s.train, diversify=mmr)
    check_ranking(res, s.h.recommend_for_users(data, s.cand, K, exclude=s.train, diversify=mmr), data, N_USERS // 2)
    res_als = s.h.ranking_metrics(data, s.cand, k=K, exclude=s.train, diversify=mmr, similarity="als")
    check_ranking(res_als, s.h.recommend_for_users(data, s.cand, K, exclude=s.train, diversify=mmr, similarity="als"),
                  data, N_USERS // 2)
    assert s.h.evaluate_ranking(data, s.cand, "precisionAtK", k=K, exclude=s.train, diversify=mmr) == \
        res["precisionAtK"]
    with pytest.raises(ValueError):
        s.h.recommend_for_all_users(s.cand, K, diversify=mmr, similarity="cooccurrence")
    with pytest.raises(TypeError):
        s.h.ranking_metrics(data, s.cand, k=K, diversify=0.5)


def test_diversify_lists_on_a_hand_made_frame(device):
    """Items 10 and 20 point the same way, 30 is orthogonal, 40 is a zero
    vector, 99 is outside item_ids. Scores 3, 2, 1 of user 1: rel 1, 0.5, 0;
    lambda 0.5: 10 (0.5), then 30 (0 against 0.25 - 0.5), then 20."""
    from src.evaluation import RecommenderEvaluator
    from src.ranked_lists import MMR

    item_ids = [10, 20, 30, 40]
    vectors = np.array([[2, 0], [3, 0], [0, 1], [0, 0]], np.float32)
    lists = pd.DataFrame({"userId": [1, 2, 3, 4], "recommendations": [
        [(99, 9.0), (10, 3.0), (20, 2.0), (30, 1.0)],
        [(30, 1.0)],
        [],
        [(10, 2.0), (20, 2.0), (40, 2.0)]]})
    out = RecommenderEvaluator.diversify_lists(lists, item_ids, vectors, MMR(0.5), 3)
    assert list(out.columns) == ["userId", "recommendations"] and out["userId"].tolist() == [1, 2, 3, 4]
    # user 4: equal scores (rel 1): 10 first; then the zero vector 40 (0.5 - 0) beats 20 (0.5 - 0.5)
    assert out["recommendations"].tolist() == [[(10, 3.0), (30, 1.0), (20, 2.0)], [(30, 1.0)], [],
                                               [(10, 2.0), (40, 2.0), (20, 2.0)]]
    # num above the longest list is clipped; lambda 1 keeps each list's own order
    same = RecommenderEvaluator.diversify_lists(lists, item_ids, vectors, MMR(1.0), 50)
    assert same["recommendations"].tolist() == [[(10, 3.0), (20, 2.0), (30, 1.0)], [(30, 1.0)], [],
                                                [(10, 2.0), (20, 2.0), (40, 2.0)]]
    assert RecommenderEvaluator.diversify_lists(lists, item_ids, vectors, MMR(0.5), 1)["recommendations"].tolist() == \
        [[(10, 3.0)], [(30, 1.0)], [], [(10, 2.0)]]
    with pytest.raises(ValueError):
        RecommenderEvaluator.diversify_lists(lists, [10, 10, 30, 40], vectors, MMR(0.5), 3)
    with pytest.raises(TypeError):
        RecommenderEvaluator.diversify_lists(lists, item_ids, vectors, 0.5, 3)
    with pytest.raises(ValueError):
        RecommenderEvaluator.diversify_lists(lists, item_ids, vectors, MMR(0.5), 0)
