"""GPU: ALSModel.explain and explain_recommendations.

Small models: 40 users x 30 items, 8 distinct items per user, ratings in
{1, 1.5, .., 5}; rank 8 and rank 20, max_iter 3, explicit and implicit_prefs.
The fit ends with the user half-sweep, so every stored user row is the f32
rounding of A^-1 b against the stored item factors, and
  |explained - prediction| <= 2 (k + 2) 2^-24 sum_c |U_uc V_ic|:
the f32 rounding of the stored row (2^-24 per component) and of transform's
k-term f32 chain ((k + 1) 2^-24 of the sum of magnitudes at the most), with a
factor 2 of margin. max_refit_gap stays within the project's ALS tolerance,
rtol 1e-5 of the row (tests/test_gpu_als_conditioning.py), and exceeds 100 x
that first value once half of every user's history is taken away."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, PER_USER = 40, 30, 8
CONFIGS = {"rank8": dict(rank=8), "rank20": dict(rank=20),
           "rank8_implicit": dict(rank=8, implicit_prefs=True, alpha=2.0),
           "rank20_implicit": dict(rank=20, implicit_prefs=True, alpha=0.5)}
_CACHE = {}


def _train():
    if "train" not in _CACHE:
        rng = np.random.default_rng(21)
        rows = [(10 + 3 * u, 100 + 7 * int(i), float(rng.integers(2, 11)) / 2) for u in range(N_USERS)
                for i in rng.choice(N_ITEMS, PER_USER, replace=False)]
        _CACHE["train"] = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
    return _CACHE["train"]


def _model(name):
    if name not in _CACHE:
        from src.als_model import ALSModel

        m = ALSModel(max_iter=3, reg_param=0.1, seed=17, **CONFIGS[name])
        assert m.train(_train()) is True
        _CACHE[name] = m
    return copy.copy(_CACHE[name])


def _bound(m, frame):
    """2 (k + 2) 2^-24 sum_c |U_uc V_ic| per row of frame (f64)."""
    mod = m.model
    u = mod._lookup(mod.user_ids, frame["userId"].to_numpy(np.int64))
    i = mod._lookup(mod.item_ids, frame["itemId"].to_numpy(np.int64))
    U = mod.U.cpu().numpy().astype(np.float64)[u]
    V = mod.V.cpu().numpy().astype(np.float64)[i]
    return 2 * (mod.k + 2) * 2.0 ** -24 * np.abs(U * V).sum(axis=1)


def _check_invariant(m, out, what):
    err = np.abs(out["explained"].to_numpy() - out["prediction"].to_numpy().astype(np.float64))
    bound = _bound(m, out)
    print("%s: largest |explained - prediction| / bound = %.3f" % (what, float((err / bound).max())))
    assert np.isfinite(err).all() and (err <= bound).all()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_contributions_add_up_to_the_prediction(device, name):
    m = _model(name)
    train = _train()
    out = m.explain(train, history=train)
    assert list(out.columns) == list(train.columns) + ["prediction", "explained", "contributions"]
    assert len(out) == len(train) and out["explained"].dtype == np.float64
    assert out["prediction"].to_numpy().tobytes() == m.transform(train)["prediction"].to_numpy().tobytes()
    _check_invariant(m, out, name)
    info = out.attrs["explain"]
    assert info["ratings_used"] == len(train) and info["ratings_dropped"] == 0 and info["users_without_history"] == 0
    row_scale = float(m.model.U.abs().max().item())
    print("%s: max_refit_gap = %.3e (row scale %.3f)" % (name, info["max_refit_gap"], row_scale))
    assert 0 <= info["max_refit_gap"] <= 1e-5 * row_scale
    # half of each user's rows removed: the rows were not fitted on that history
    half = train[train.groupby("userId").cumcount() % 2 == 0]
    other = m.explain(train, history=half)
    assert other.attrs["explain"]["max_refit_gap"] > 100 * max(info["max_refit_gap"], 2.0 ** -30 * row_scale)
    # contributions: the user's own history, descending, at most top
    own = train.groupby("userId")["itemId"].apply(set).to_dict()
    for u, contrib in zip(out["userId"], out["contributions"]):
        assert 1 <= len(contrib) <= 5
        assert all(i in own[u] for i, _ in contrib)
        v = [c for _, c in contrib]
        assert v == sorted(v, reverse=True)
    assert all(len(c) == 1 for c in m.explain(train.iloc[:9], history=train, top=1)["contributions"])
    full = m.explain(train.iloc[:9], history=train, top=32)["contributions"]
    if "implicit" not in name:
        assert all(len(c) == PER_USER for c in full)  # top above the history: all of it


@pytest.mark.parametrize("name", ["rank8", "rank20_implicit"])
def test_explanations_equal_a_direct_kernel_call(device, name):
    from src import _hrec

    m = _model(name)
    train, mod = _train(), m.model
    pairs = train.iloc[[3, 50, 51, 200, 319]]
    out = m.explain(pairs, history=train, top=4)
    yty = _hrec.als_gramian(mod.V, mod.k) if m.implicit_prefs else None
    for (_, p), explained, contrib in zip(pairs.iterrows(), out["explained"], out["contributions"]):
        h = train[train["userId"] == p["userId"]]
        cols = mod._lookup(mod.item_ids, h["itemId"].to_numpy(np.int64))
        hist = (torch.zeros(1, dtype=torch.int64, device=device),
                torch.tensor([0, len(h)], dtype=torch.int64, device=device),
                torch.as_tensor(cols.astype(np.int32), device=device),
                torch.as_tensor(h["average_review_rating"].to_numpy(np.float32), device=device))
        irow = mod._lookup(mod.item_ids, np.array([p["itemId"]], np.int64))
        total, pos, val, ln, _ = _hrec.als_explain(
            torch.as_tensor(irow.reshape(1, 1), device=device), hist, mod.V, mod.k, 0.1, 4,
            implicit=bool(m.implicit_prefs), alpha=float(m.alpha), yty=yty)
        n = int(ln[0, 0].item())
        assert n == len(contrib)
        assert np.float64(explained).tobytes() == total[0, 0].cpu().numpy().tobytes()
        assert np.array([c for _, c in contrib]).tobytes() == val[0, 0, :n].cpu().numpy().tobytes()
        assert [i for i, _ in contrib] == h["itemId"].to_numpy()[pos[0, 0, :n].cpu().numpy()].tolist()


@pytest.mark.parametrize("name", ["rank20", "rank8_implicit"])
def test_the_invariant_holds_for_folded_users(device, name):
    m = _model(name)
    train = _train()
    new = train[train["userId"].isin([10, 13, 40, 100])].copy()
    new["userId"] += 5000
    res = m.fold_in_users(new)
    assert res["users_added"] == 4
    out = m.explain(new, history=new)
    _check_invariant(m, out, name + " folded")
    assert out.attrs["explain"]["max_refit_gap"] <= 1e-5 * float(m.model.U.abs().max().item())
    assert out.attrs["explain"]["users_without_history"] == 0


@pytest.mark.parametrize("name", ["rank8", "rank20_implicit"])
def test_explain_recommendations(device, name):
    m = _model(name)
    train = _train()
    users = [10, 13, 16, 127, 99999]  # 99999: unknown, left out
    plain = m.recommend_for_user_subset(users, 5, exclude=train)
    out = m.explain_recommendations(users, 5, history=train, exclude=train)
    assert out["userId"].tolist() == plain["userId"].tolist() == [10, 13, 16, 127]
    assert list(out.columns) == ["userId", "recommendations", "explained"]
    for a, b, e in zip(out["recommendations"], plain["recommendations"], out["explained"]):
        assert [(i, np.float32(s).tobytes()) for i, s, _ in a] == [(i, np.float32(s).tobytes()) for i, s in b]
        assert len(e) == len(a) == 5
    # the same explanations as explain on the exploded pairs, bit for bit
    pairs = pd.DataFrame([(u, i) for u, recs in zip(out["userId"], out["recommendations"]) for i, _, _ in recs],
                         columns=["userId", "itemId"])
    flat = m.explain(pairs, history=train)
    assert flat["contributions"].tolist() == [c for recs in out["recommendations"] for _, _, c in recs]
    assert flat["explained"].to_numpy().tobytes() == np.array([x for e in out["explained"] for x in e]).tobytes()
    assert flat["prediction"].to_numpy().tobytes() == np.array(
        [s for recs in out["recommendations"] for _, s, _ in recs], np.float32).tobytes()
    assert out.attrs["explain"]["max_refit_gap"] == flat.attrs["explain"]["max_refit_gap"]
    _check_invariant(m, flat, name + " recommended")
    # without an exclusion the lists are the plain ones too
    free = m.explain_recommendations(users, 3, history=train)
    assert [[i for i, _, _ in r] for r in free["recommendations"]] == [
        [i for i, _ in r] for r in m.recommend_for_user_subset(users, 3)["recommendations"]]
    # a user absent from history: the list stays, without reasons
    part = m.explain_recommendations([10, 13], 5, history=train[train["userId"] != 13], exclude=train)
    assert all(c == [] for _, _, c in part["recommendations"][1]) and np.isnan(part["explained"][1]).all()
    assert all(len(c) > 0 for _, _, c in part["recommendations"][0])
    assert part.attrs["explain"]["users_without_history"] == 1


def test_unknown_ids_and_missing_history(device):
    m = _model("rank8")
    train = _train()
    hist = pd.concat([train[train["userId"] != 13],
                      pd.DataFrame({"userId": [10, 777], "itemId": [424242, 100], "average_review_rating": [3.0, 4.0]})])
    pairs = pd.DataFrame({"userId": [10, 99999, 10, 13, 16], "itemId": [100, 100, 55555, 100, 107]})
    out = m.explain(pairs, history=hist)
    assert len(out) == 5
    ok = [True, False, False, False, True]
    assert [bool(np.isfinite(x)) for x in out["explained"]] == ok
    assert [len(c) > 0 for c in out["contributions"]] == ok
    pred = out["prediction"].to_numpy()
    assert np.isnan(pred[[1, 2]]).all() and np.isfinite(pred[[0, 3, 4]]).all()
    info = out.attrs["explain"]
    assert info["ratings_dropped"] == 1 and info["ratings_used"] == len(hist) - 1
    assert info["users_without_history"] == 1  # user 13
    empty = m.explain(pairs.iloc[:0], history=hist)
    assert len(empty) == 0 and list(empty.columns)[-3:] == ["prediction", "explained", "contributions"]
    none = m.explain(pairs, history=hist.iloc[:0])
    assert np.isnan(none["explained"]).all() and none.attrs["explain"]["ratings_used"] == 0


def test_what_cannot_be_explained_raises(device):
    from src.als_model import ALSModel

    train = _train()
    with pytest.raises(RuntimeError, match="not trained"):
        ALSModel(rank=8).explain(train, history=train)
    with pytest.raises(RuntimeError, match="not trained"):
        ALSModel(rank=8).explain_recommendations([10], 5, history=train)
    nn = ALSModel(rank=8, max_iter=1, reg_param=0.1, seed=17, nonnegative=True)
    assert nn.train(train) is True
    with pytest.raises(ValueError, match="nonnegative"):
        nn.explain(train, history=train)
    wide = ALSModel(rank=100, max_iter=1, reg_param=0.1, seed=17)
    assert wide.train(train) is True
    with pytest.raises(ValueError, match="rank <= 64"):
        wide.explain(train, history=train)
    with pytest.raises(ValueError, match="rank <= 64"):
        wide.explain_recommendations([10], 5, history=train)
    m = _model("rank8")
    for top in (0, 33):
        with pytest.raises(ValueError, match="top"):
            m.explain(train, history=train, top=top)
