"""GPU: similar_items / similar_users of the models and
RecommenderEvaluator.similar_rows against the numpy oracle
(tests/cosine_oracle.py) applied to each model's own factors or vectors, read
back, with the kernel's own inv_norm. Ids and the bits of the similarities
must match.

The small models of tests/test_gpu_list_quality_api.py: 40 users x 60 items;
ALS rank 8 trained on 54 of the items at most; two-tower embedding_size 50 and
64, freshly built; the candidate frame is shuffled and holds every item."""
import numpy as np
import pandas as pd
import pytest

import cosine_oracle as co
import test_gpu_list_quality_api as models

pytestmark = pytest.mark.gpu

N_ITEMS = models.N_ITEMS


def expected(ids, vectors, d, rows, num, min_similarity=None):
    """The oracle's lists [(id, similarity)] for the query rows of `vectors`
    (numpy [n, >= d]), ids[j] naming row j."""
    import torch
    from src import _hrec

    v = np.ascontiguousarray(vectors[:, :d], np.float32)
    inv = _hrec.row_inv_norms(torch.as_tensor(v, device="cuda")).cpu().numpy()
    idx, val, ln = co.topk(v, d, inv, rows, num, True, -np.inf if min_similarity is None else min_similarity)
    return [[(int(ids[j]), float(s)) for j, s in zip(idx[b, :m], val[b, :m])] for b, m in enumerate(ln)]


def check_frame(df, key, keys, want):
    assert list(df.columns) == [key, "recommendations"]
    assert df[key].tolist() == [int(k) for k in keys]
    got = df["recommendations"].tolist()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert [i for i, _ in g] == [i for i, _ in w]
        assert np.array_equal(np.array([s for _, s in g], np.float64).view(np.int64),
                              np.array([s for _, s in w], np.float64).view(np.int64))
        assert all(type(i) is int and type(s) is float for i, s in g)


def setup(device, d=50):
    return models._setup(device, d)


@pytest.mark.parametrize("side", ["item", "user"])
def test_als(device, side):
    s = setup(device)
    m = s.als.model
    ids, F = (m.item_ids, m.V) if side == "item" else (m.user_ids, m.U)
    ids = np.asarray(ids, np.int64)
    vec = F.cpu().numpy()
    call = s.als.similar_items if side == "item" else s.als.similar_users
    key = side + "Id"
    n = ids.size
    assert (np.diff(ids) > 0).all()
    # every row, ids ascending
    check_frame(call(), key, ids, expected(ids, vec, m.k, np.arange(n), 10))
    # a subset: repeated and unknown ids; a DataFrame works too
    sub = [int(ids[7]), int(ids[2]), 100000, int(ids[7]), -4]
    rows = np.array([2, 7])
    want = expected(ids, vec, m.k, rows, 3, 0.5)
    check_frame(call(sub, num=3, min_similarity=0.5), key, ids[rows], want)
    check_frame(call(pd.DataFrame({key: sub}), num=3, min_similarity=0.5), key, ids[rows], want)
    # num larger than the catalogue: every other row, once
    full = call(num=1024)
    check_frame(full, key, ids, expected(ids, vec, m.k, np.arange(n), 1024))
    for k, rec in zip(full[key], full["recommendations"]):
        assert len(rec) == n - 1 and sorted(i for i, _ in rec) == sorted(set(ids.tolist()) - {k})
        assert all(a[1] >= b[1] for a, b in zip(rec, rec[1:]))
    # a cut nothing passes; a second call gives the same frame
    assert all(r == [] for r in call(num=5, min_similarity=1.5)["recommendations"])
    assert call(sub, num=3).equals(call(sub, num=3))
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            call(num=bad)
    assert call([100000], num=3).shape == (0, 2)


def test_als_nonnegative_and_implicit_and_wide_rank(device):
    from src.als_model import ALSModel

    s = setup(device)
    for kw in (dict(nonnegative=True), dict(implicit_prefs=True, alpha=2.0), dict(rank=96)):
        kw = dict(dict(rank=8, max_iter=2, reg_param=0.1, seed=5), **kw)
        als = ALSModel(**kw)
        assert als.train(s.train) is True
        m = als.model
        ids = np.asarray(m.item_ids, np.int64)
        check_frame(als.similar_items(num=4), "itemId", ids,
                    expected(ids, m.V.cpu().numpy(), m.k, np.arange(ids.size), 4))


@pytest.mark.parametrize("d", [50, 64])
def test_two_tower(device, d):
    from src.evaluation import RecommenderEvaluator
    from src.ranked_lists import MMR

    s = setup(device, d)
    vec = s.cand.vectors.cpu().numpy()
    assert vec.shape == (N_ITEMS, d)
    # every candidate, in frame order (the frame is shuffled)
    got = s.tt.similar_items(s.cand)
    check_frame(got, "itemId", s.ids, expected(s.ids, vec, d, np.arange(N_ITEMS), 10))
    assert got.equals(s.tt.similar_items(s.frame))
    # a subset: its distinct ids ascending, an id outside the frame left out
    sub = [int(s.ids[5]), int(s.ids[0]), 5000, int(s.ids[5])]
    keys = np.unique([int(s.ids[5]), int(s.ids[0])])
    rows = np.array([int(np.flatnonzero(s.ids == k)[0]) for k in keys])
    check_frame(s.tt.similar_items(s.cand, sub, num=7, min_similarity=0.0), "itemId", keys,
                expected(s.ids, vec, d, rows, 7, 0.0))
    # the lists frame goes through the evaluator as it is
    res = RecommenderEvaluator.evaluate_lists(got, s.ids, vec)
    assert res["count"] == N_ITEMS and 0 < res["catalogCoverage"] <= 1
    picked = RecommenderEvaluator.diversify_lists(got, s.ids, vec, MMR(0.5), 5)
    assert picked["itemId"].tolist() == got["itemId"].tolist() and all(len(r) == 5 for r in picked["recommendations"])


def test_hybrid(device):
    s = setup(device)
    vec = s.cand.vectors.cpu().numpy()
    got = s.h.similar_items(s.cand, num=6)
    check_frame(got, "itemId", s.ids, expected(s.ids, vec, 50, np.arange(N_ITEMS), 6))
    assert got.equals(s.tt.similar_items(s.cand, num=6))
    # ALS factors in frame order; an item the ALS model does not know is the zero vector
    avec = s.als_vectors_in_frame_order()
    unknown = np.flatnonzero(~avec.any(axis=1))
    assert unknown.size >= 6
    k = s.als.model.k
    als = s.h.similar_items(s.cand, num=N_ITEMS, similarity="als")
    check_frame(als, "itemId", s.ids, expected(s.ids, avec, k, np.arange(N_ITEMS), N_ITEMS))
    for r in unknown:
        rec = als["recommendations"][r]
        # similarity +0.0 to everything: every other candidate in frame order
        assert [i for i, _ in rec] == [int(i) for j, i in enumerate(s.ids) if j != r]
        assert all(sim == 0.0 and not np.signbit(sim) for _, sim in rec)
    cut = s.h.similar_items(s.cand, [int(s.ids[unknown[0]])], num=5, min_similarity=0.0, similarity="als")
    assert cut["recommendations"].tolist() == [[]]
    with pytest.raises(ValueError):
        s.h.similar_items(s.cand, similarity="cooccurrence")


def test_similar_rows_of_any_matrix(device):
    from src.evaluation import RecommenderEvaluator

    import torch

    s = setup(device)
    users = np.arange(models.N_USERS, dtype=np.int64)
    uvec = s.tt.model.user_vectors(torch.as_tensor(users.astype(np.int32), device="cuda"))  # user-tower outputs
    ids = users * 10 + 3
    vec = uvec.cpu().numpy()
    got = RecommenderEvaluator.similar_rows(uvec, ids)
    check_frame(got, "id", ids, expected(ids, vec, vec.shape[1], users, 10))
    # host vectors, shuffled ids, a query list with an unknown and a repeated id
    rng = np.random.default_rng(3)
    perm = rng.permutation(ids.size)
    sub = RecommenderEvaluator.similar_rows(vec[perm], ids[perm], queries=[ids[4], 7, ids[1], ids[4]], num=1024,
                                            min_similarity=-0.25)
    keys = np.array(sorted([int(ids[4]), int(ids[1])]))
    rows = np.array([int(np.flatnonzero(ids[perm] == k)[0]) for k in keys])
    check_frame(sub, "id", keys, expected(ids[perm], vec[perm], vec.shape[1], rows, 1024, -0.25))
    with pytest.raises(ValueError):
        RecommenderEvaluator.similar_rows(vec, np.zeros(ids.size, np.int64))
    with pytest.raises(ValueError):
        RecommenderEvaluator.similar_rows(vec[:, :0], ids)
