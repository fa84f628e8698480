"""GPU: fold_in_users on ALSModel, TwoTowerModel and HybridRecommendationSystem.

One rated frame: 300 users x 120 items, 12 distinct items per user, ratings
in {1, 1.5, .., 5} (exact in f32). ALS models of four configurations are fitted
on it (max_iter 3) once; the two-tower models (embedding_size 50 and 64) get
one epoch of training first, so Adam slots and `iterations` are not at their
initial values. Every test folds into a copy of its own (_als, _tt), so the
tests do not depend on their order or on running once.

Bit identity (ALS): a user's ratings copied under a new id give, through the
same half-sweep launch against the same item factors, the row the fit gave the
original. The independent solve is numpy's f64 solve of the ALS-WR normal
equations at the project's fit tolerance (rtol 1e-4).

Two-tower tolerances follow tests/test_gpu_tt_fold_in.py: 8 x the f32-vs-f64 gap
of tests/fold_in_oracle.py on the same inputs, never below 2e-6."""
import copy

import numpy as np
import pandas as pd
import pytest
import torch

import fold_in_oracle as fo
import hybrid_lists_oracle as hlo

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, PER_USER = 300, 120, 12
ALS_CONFIGS = {"rank10": dict(rank=10), "rank20_implicit": dict(rank=20, implicit_prefs=True, alpha=2.0),
               "rank64_nonneg": dict(rank=64, nonnegative=True), "rank100": dict(rank=100)}
_CACHE = {}


def _ratings():
    if "ratings" not in _CACHE:
        rng = np.random.default_rng(5)
        rows = [(u, int(i), float(rng.integers(2, 11)) / 2) for u in range(N_USERS)
                for i in rng.choice(N_ITEMS, PER_USER, replace=False)]
        _CACHE["ratings"] = pd.DataFrame(rows, columns=["userId", "itemId", "average_review_rating"])
    return _CACHE["ratings"]


def _items():
    if "items" not in _CACHE:
        rng = np.random.default_rng(6)
        _CACHE["items"] = pd.DataFrame({
            "itemId": rng.permutation(N_ITEMS).astype(np.int64), "manufacturer_id": rng.integers(0, 30, N_ITEMS),
            "category_id": rng.integers(0, 10, N_ITEMS), "price": rng.random(N_ITEMS) * 100,
            "average_review_rating": rng.integers(0, 11, N_ITEMS).astype(np.float64) / 2})
    return _CACHE["items"]


def _als(name):
    """A copy of the fitted ALSModel for one test to fold users into. fold_in_users
    puts a new DeviceALSFactors on the instance it is called on and writes to no
    tensor of the old one, so the fitted model in the cache stays as it was fitted."""
    if name not in _CACHE:
        from src.als_model import ALSModel

        m = ALSModel(max_iter=3, reg_param=0.1, seed=17, **ALS_CONFIGS[name])
        assert m.train(_ratings()) is True
        _CACHE[name] = (m, m.model.user_ids.copy(), m.model.U.clone())
    m, ids, U = _CACHE[name]
    assert np.array_equal(m.model.user_ids, ids) and torch.equal(m.model.U, U)  # no test has changed it
    return copy.copy(m)


def _copy_of(users, offset):
    """The rows of `users` in the rated frame, frame order kept, under ids + offset."""
    r = _ratings()
    c = r[r["userId"].isin(users)].copy()
    c["userId"] += offset
    return c


def _rows(model, ids):
    rows = model._lookup(model.user_ids, np.asarray(ids, np.int64))
    assert (rows >= 0).all()
    return model.U[torch.as_tensor(rows, device=model.U.device)].cpu().numpy()


# ------------------------------------------------------------------- ALS
@pytest.mark.parametrize("name", list(ALS_CONFIGS))
def test_als_folded_rows_have_the_fits_bits(device, name):
    als = _als(name)
    orig = np.arange(3, N_USERS, 7)[:40]
    new = orig + 1_000_000
    copy = _copy_of(orig, 1_000_000)
    before_ids, before_U = als.model.user_ids.copy(), als.model.U.clone()
    V = als.model.V
    res = als.fold_in_users(copy)
    assert res == {"users_added": 40, "users_replaced": 0, "users_skipped": 0, "ratings_used": 40 * PER_USER,
                   "ratings_dropped": 0}
    m = als.model
    assert m.V is V and (np.diff(m.user_ids) > 0).all() and len(m.user_ids) == len(before_ids) + 40
    assert _rows(m, new).tobytes() == _rows(m, orig).tobytes()
    assert _rows(m, before_ids).tobytes() == before_U.cpu().numpy().tobytes()  # old users still hit their old rows
    # the lists and the predictions of a copy are the original's
    mine = _ratings()[_ratings()["userId"].isin(orig)]
    a = als.recommend_for_user_subset(new, 10, exclude=copy)
    b = als.recommend_for_user_subset(orig, 10, exclude=mine)
    assert a["userId"].tolist() == new.tolist() and b["userId"].tolist() == orig.tolist()
    assert a["recommendations"].tolist() == b["recommendations"].tolist()
    assert all(len(r) == 10 for r in a["recommendations"])
    pa = als.transform(copy)["prediction"].to_numpy()
    pb = als.transform(mine)["prediction"].to_numpy()
    assert pa.dtype == np.float32 and len(pa) == 40 * PER_USER and pa.tobytes() == pb.tobytes()


def test_als_row_matches_an_independent_solve(device):
    als = _als("rank10")
    items = [int(i) for i in als.model.item_ids[[4, 50, 99]]]
    r = np.array([4.5, 2.0, 3.5])
    data = pd.DataFrame({"userId": [2_000_001] * 4, "itemId": items[:2] + [N_ITEMS + 77] + items[2:],
                         "average_review_rating": [r[0], r[1], 5.0, r[2]]})
    res = als.fold_in_users(data)
    assert res == {"users_added": 1, "users_replaced": 0, "users_skipped": 0, "ratings_used": 3, "ratings_dropped": 1}
    V = als.model.V[torch.as_tensor([4, 50, 99], device=als.model.V.device), :10].cpu().numpy().astype(np.float64)
    want = np.linalg.solve(V.T @ V + 0.1 * 3 * np.eye(10), V.T @ r)
    got = _rows(als.model, [2_000_001])[0]
    np.testing.assert_allclose(got[:10], want, rtol=1e-4, atol=0)
    assert not got[10:].any()  # the padding columns stay zero


def test_als_error_paths_and_bookkeeping(device):
    als = _als("rank10")
    m0 = als.model
    ids0, U0 = m0.user_ids.copy(), m0.U.clone()
    known = _copy_of([8], 0)
    with pytest.raises(ValueError, match="already in the model"):
        als.fold_in_users(known)
    assert als.model is m0
    # replace=True: the row becomes the solution from the given ratings alone
    some = known.iloc[:5]
    fresh = some.copy()
    fresh["userId"] = 3_000_000
    only_unknown = pd.DataFrame({"userId": [3_000_005, 3_000_005], "itemId": [N_ITEMS + 1, N_ITEMS + 2],
                                 "average_review_rating": [3.0, 4.0]})
    res = als.fold_in_users(pd.concat([some, fresh, only_unknown]), replace=True)
    assert res == {"users_added": 1, "users_replaced": 1, "users_skipped": 1, "ratings_used": 10, "ratings_dropped": 2}
    m = als.model
    assert _rows(m, [8]).tobytes() == _rows(m, [3_000_000]).tobytes()
    assert _rows(m, [8]).tobytes() != _rows(m0, [8]).tobytes()
    assert m._lookup(m.user_ids, [3_000_005])[0] == -1
    assert (np.diff(m.user_ids) > 0).all()
    others = ids0[ids0 != 8]
    assert _rows(m, others).tobytes() == U0[torch.as_tensor(ids0 != 8, device=U0.device)].cpu().numpy().tobytes()
    # caches keyed on the user side see the new users
    assert int(m._lookup_device(np.array([3_000_000]), "user")[0]) == int(m._lookup(m.user_ids, [3_000_000])[0])
    assert len(als.recommend_for_all_users(3)) == len(m.user_ids)


def test_als_singular_row_raises_and_leaves_the_model(device):
    """reg_param 0, 2 ratings at rank 10. The half-sweep reports a singular
    row as NaN when a pivot is exactly zero (tests/test_gpu_als_conditioning.py);
    rounding noise in a Gramian that is singular only in exact arithmetic gives
    finite garbage, in train as here. So the two ratings are of one item whose
    factors are small integers: the Gramian 2 v v^T and its elimination are
    exact, the second pivot is 0."""
    from src.als_model import ALSModel, DeviceALSFactors

    rng = np.random.default_rng(9)
    V = np.zeros((6, 16), np.float32)
    V[:, :10] = rng.normal(size=(6, 10)).astype(np.float32)
    V[4, :10] = np.array([2, 1, 0, 1, 2, 2, 0, 1, 2, 1], np.float32)
    U = np.zeros((3, 16), np.float32)
    U[:, :10] = rng.normal(size=(3, 10)).astype(np.float32)
    als = ALSModel(rank=10, reg_param=0.0)
    als.model = m = DeviceALSFactors(np.array([5, 6, 9]), np.arange(100, 106), torch.as_tensor(U, device=device),
                                     torch.as_tensor(V, device=device), 10)
    two = pd.DataFrame({"userId": [7, 7], "itemId": [104, 104], "average_review_rating": [4.0, 2.5]})
    with pytest.raises(ValueError, match="singular"):
        als.fold_in_users(two)
    assert als.model is m and m.user_ids.tolist() == [5, 6, 9] and m.U.cpu().numpy().tobytes() == U.tobytes()
    # the same ratings fold in once the equations are regularised
    als.reg_param = 0.1
    assert als.fold_in_users(two)["users_added"] == 1 and als.model.user_ids.tolist() == [5, 6, 7, 9]
    assert np.isfinite(_rows(als.model, [7])).all()


# ------------------------------------------------------------- two-tower
def _tt(d):
    """(a TwoTowerModel of its own for one test, its candidates): the trained
    weights, Adam slots, `iterations` and scaler of one cached training run on
    a fresh engine, as load_model restores them."""
    from src.two_tower_model import TwoTowerModel

    def new():
        return TwoTowerModel(N_USERS, N_ITEMS + 8, 30, 10, embedding_size=d, learning_rate=1e-3, seed=23)

    key = ("tt", d)
    if key not in _CACHE:
        tt = new()
        train = _ratings().merge(_items()[["itemId", "manufacturer_id", "category_id", "price"]], on="itemId")
        tt.train(train, batch_size=256, epochs=1)
        assert tt.model.iterations > 0
        state = tt.model.state_dict()
        state.update(tt.model.optimizer_state())
        _CACHE[key] = (state, tt.scaler)
    state, scaler = _CACHE[key]
    tt = new()
    tt.build_model(init={k: v for k, v in state.items() if not k.startswith("__")})
    tt.model.iterations = int(state["__iterations__"])
    assert tt.model.load_optimizer_state(state)
    tt.scaler, tt.is_trained = scaler, True
    return tt, tt.candidates(_items())


def _fold_data(first_user):
    """Five users from first_user on: histories of 12, 12, 3 (one item outside
    the candidate frame), 1 and 2 (both outside the frame) rows, interleaved in
    the frame."""
    rng = np.random.default_rng(first_user)
    rows = []
    for q, n in enumerate((12, 12, 3, 1, 2)):
        items = rng.choice(N_ITEMS, n, replace=False).tolist()
        if q == 2:
            items[1] = N_ITEMS + 300
        if q == 4:
            items = [N_ITEMS + 301, N_ITEMS + 302]
        rows += [(first_user + q, int(i), float(rng.integers(2, 11)) / 2) for i in items]
    order = rng.permutation(len(rows))
    return pd.DataFrame([rows[i] for i in order], columns=["userId", "itemId", "average_review_rating"])


def _operands(tt, cand, data, steps, lr):
    """hrec_tt_fold_in_users' operands for `data`, grouped here in Python."""
    dev = tt.model.device
    users = np.unique(data["userId"].to_numpy())
    groups = [data[data["userId"] == u] for u in users]
    items = np.concatenate([g["itemId"].to_numpy() for g in groups]).astype(np.int64)
    ratings = np.concatenate([g["average_review_rating"].to_numpy() for g in groups]).astype(np.float32)
    indptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    rows = cand.rows_of(torch.as_tensor(items, device=dev))
    return (users, torch.as_tensor(indptr, device=dev), rows, torch.as_tensor(ratings, device=dev),
            torch.as_tensor(fo.step_sizes(lr, steps), device=dev))


def _restatement(tt, cand, emb0, ops, steps, dtype):
    _, indptr, rows, ratings, lr = ops
    t = tt.model.tensors
    return fo.fold_in(emb0, t["ln_user_gamma"].cpu().numpy(), t["ln_user_beta"].cpu().numpy(),
                      cand.vectors.cpu().numpy(), indptr.cpu().numpy(), rows.cpu().numpy(), ratings.cpu().numpy(),
                      steps, lr.cpu().numpy(), dtype)


@pytest.mark.parametrize("d", [50, 64])
def test_two_tower_moves_only_the_folded_rows(device, d):
    from src import _hrec

    tt, cand = _tt(d)
    eng = tt.model
    data = _fold_data(40)
    steps, lr = 30, 1e-2
    ops = _operands(tt, cand, data, steps, lr)
    users = ops[0]
    snap = {n: t.clone() for n, t in eng.tensors.items()}
    slots = {n: (eng.m_tab[n].clone(), eng.v_tab[n].clone()) for n in eng.m_tab}
    dense, its = (eng.dense.clone(), eng.m_dense.clone(), eng.v_dense.clone()), eng.iterations
    # the direct call on the same operands
    emb = snap["user_emb"][torch.as_tensor(users, device=device)].clone()
    direct = _hrec.tt_fold_in_users(emb, snap["ln_user_gamma"], snap["ln_user_beta"], cand.vectors, *ops[1:],
                                    fo.BETA_1, np.float32(1) - fo.BETA_1, fo.BETA_2, np.float32(1) - fo.BETA_2,
                                    fo.EPSILON)
    out = tt.fold_in_users(data, cand, steps=steps, learning_rate=lr)
    assert list(out.columns) == ["userId", "n_ratings", "loss_before", "loss_after"]
    assert out["userId"].tolist() == users.tolist() and out["n_ratings"].tolist() == [12, 12, 2, 1, 0]
    assert out.attrs["ratings_dropped"] == 3
    folded = torch.as_tensor(users, device=device)
    now = eng.tensors["user_emb"]
    assert torch.equal(now[folded].view(torch.int32), emb.view(torch.int32))
    np.testing.assert_array_equal(out[["loss_before", "loss_after"]].to_numpy(np.float32).view(np.int32),
                                  direct.cpu().numpy().view(np.int32))
    moved = (now != snap["user_emb"]).any(1).cpu().numpy()
    assert moved[users[:4]].all() and not moved[users[4]] and moved.sum() == 4  # the user without a usable rating stays
    assert np.isnan(out["loss_after"].iloc[4]) and np.isfinite(out["loss_after"].iloc[:4]).all()
    for n, t in eng.tensors.items():
        if n != "user_emb":
            assert torch.equal(t, snap[n]), n
    for n in slots:
        assert torch.equal(eng.m_tab[n], slots[n][0]) and torch.equal(eng.v_tab[n], slots[n][1]), n
    assert all(torch.equal(a, b) for a, b in zip((eng.dense, eng.m_dense, eng.v_dense), dense))
    assert eng.iterations == its and tt.candidates(cand) is cand


@pytest.mark.parametrize("d", [50, 64])
def test_two_tower_loss_falls_and_transform_reports_it(device, d):
    tt, cand = _tt(d)
    data = _fold_data(80)
    steps, lr = 200, 1e-2
    ops = _operands(tt, cand, data, steps, lr)
    users = ops[0]
    emb0 = tt.model.tensors["user_emb"][torch.as_tensor(users, device=device)].cpu().numpy()
    _, _, l64 = _restatement(tt, cand, emb0, ops, steps, np.float64)
    _, _, l32 = _restatement(tt, cand, emb0, ops, steps, np.float32)
    has = ~np.isnan(l64[:, 0])
    assert has.tolist() == [True, True, True, True, False] and (l64[has, 1] < l64[has, 0]).all()
    out = tt.fold_in_users(data, cand, steps=steps, learning_rate=lr)
    before, after = out["loss_before"].to_numpy(), out["loss_after"].to_numpy()
    assert (after[has] < before[has]).all()
    assert np.abs(after[has] - l64[has, 1]).max() <= max(8 * np.abs(l32[has, 1] - l64[has, 1]).max(), 2e-6)
    # the pointwise API sees the fitted rows: its mse over a user's rows is the kernel's loss_after. Other
    # users and 20 steps, where the loss is still O(1) and the comparison says something.
    data, steps = _fold_data(120), 20
    ops = _operands(tt, cand, data, steps, lr)
    users = ops[0]
    emb0 = tt.model.tensors["user_emb"][torch.as_tensor(users, device=device)].cpu().numpy()
    l64, l32 = (_restatement(tt, cand, emb0, ops, steps, dt)[2][:, 1] for dt in (np.float64, np.float32))
    out = tt.fold_in_users(data, cand, steps=steps, learning_rate=lr)
    after = out["loss_after"].to_numpy()
    tol = max(8 * float(np.abs(l32[has].astype(np.float64) - l64[has]).max()), 2e-6)
    for q in np.flatnonzero(has):
        mine = data[data["userId"] == users[q]]
        res = tt.regression_metrics(mine, candidates=cand)
        pred = tt.transform(mine, candidates=cand)["prediction"].to_numpy()
        ok = ~np.isnan(pred)
        y = mine["average_review_rating"].to_numpy()
        print(f"d {d} user {users[q]}: loss_after {after[q]:.6g}, mse {res['mse']:.6g}, f64 restatement "
              f"{l64[q]:.6g}, allowed {tol:.3g}")
        assert res["count"] == out["n_ratings"].iloc[q] == ok.sum()
        assert abs(res["mse"] - float(after[q])) <= tol
        assert abs(float(np.mean((pred[ok].astype(np.float64) - y[ok]) ** 2)) - float(after[q])) <= tol
        assert abs(float(after[q]) - l64[q]) <= tol


def test_two_tower_grows_the_user_table(device, tmp_path):
    tt, cand = _tt(50)
    eng = tt.model
    old = eng.sizes["user_emb"]
    frame = _items()
    pred_before = [tt.predict_for_user(u, frame) for u in (0, 7, old - 1)]
    data = _fold_data(old + 20)
    with pytest.raises(IndexError):
        tt.predict_for_user(old + 20, frame)
    out = tt.fold_in_users(data, cand, steps=20, learning_rate=1e-2)
    new = old + 25
    assert eng.sizes["user_emb"] == tt.num_users == new == out["userId"].max() + 1
    assert tuple(eng.tensors["user_emb"].shape) == tuple(eng.m_tab["user_emb"].shape) == (new, 50)
    assert tuple(eng.mark["user_emb"].shape) == (new,) and bool((eng.mark["user_emb"][old:] == -1).all())
    assert not eng.m_tab["user_emb"][old:].any() and not eng.v_tab["user_emb"][old:].any()
    grown = eng.tensors["user_emb"][old: old + 20].cpu().numpy()  # rows nobody folded: the seeded Keras init
    want = np.random.default_rng([eng.seed, old]).uniform(-0.05, 0.05, size=(25, 50)).astype(np.float32)[:20]
    assert grown.tobytes() == want.tobytes()
    assert [tt.predict_for_user(u, frame) for u in (0, 7, old - 1)] == pred_before
    assert tt.candidates(cand) is cand  # built before the call, still accepted
    assert len(tt.predict_for_user(old + 20, frame)) == N_ITEMS
    assert len(tt.recommend_for_users([old + 20, 3], cand, 5, exclude=data)) == 2
    with pytest.raises(IndexError):
        tt.fold_in_users(pd.DataFrame({"userId": [1 << 24], "itemId": [1], "average_review_rating": [3.0]}), cand)
    # the seed the grown rows are drawn from survives save / load: the same call grows the same rows
    from src.two_tower_model import TwoTowerModel

    tt.save_model(str(tmp_path / "tt.keras"))
    again = TwoTowerModel.load_model(str(tmp_path / "tt.keras"))
    assert again.model.seed == eng.seed == 23 and again.num_users == new
    for m in (tt, again):
        m.model.grow_users(new + 3)
    assert torch.equal(again.model.tensors["user_emb"], eng.tensors["user_emb"])


# ---------------------------------------------------------------- hybrid
def test_hybrid_serves_folded_users_as_known_users(device):
    from src import _hrec
    from src.als_model import ALSModel
    from src.hybrid_system import HybridRecommendationSystem

    als = ALSModel(rank=10, max_iter=3, reg_param=0.1, seed=29)
    assert als.train(_ratings()) is True
    tt, cand = _tt(64)
    h = HybridRecommendationSystem()
    h.als_model, h.twotower_model, h.models_loaded = als, tt, True
    h.als_f1_score, h.twotower_f1_score = 0.5, 0.1
    first = max(tt.model.sizes["user_emb"], N_USERS) + 100
    data = _fold_data(first)
    data = data[data["userId"] != first + 4]  # without the user whose items nobody knows
    users = np.unique(data["userId"].to_numpy())
    assert (als.model._lookup(als.model.user_ids, users) < 0).all()
    res = h.fold_in_users(data, cand, steps=50, learning_rate=1e-2)
    assert res["als"]["users_added"] == 4 and res["als"]["ratings_dropped"] == 1
    assert res["twotower"]["userId"].tolist() == users.tolist()
    assert h._als_fallback(users, cand.item_ids) is None  # nothing is substituted for these users
    a = als.model.score(users, cand.item_ids)
    t = _hrec.tt_score(tt.model.user_vectors(torch.as_tensor(users.astype(np.int32), device=device)), cand.vectors)
    assert bool(torch.isfinite(a).all())
    pos = {int(i): r for r, i in enumerate(cand.item_ids)}
    cols = [sorted({pos[int(i)] for i in data["itemId"][data["userId"] == u] if int(i) in pos}) for u in users]
    excl = (np.arange(len(users)), np.concatenate([[0], np.cumsum([len(c) for c in cols])]), np.concatenate(cols))
    want, lens, _ = hlo.lists(a.cpu().numpy(), t.cpu().numpy(), 5, True, None, excl)
    df = h.recommend_for_users(users, cand, 5, exclude=data)
    assert df["userId"].tolist() == users.tolist()
    for rec, (idx, val), n in zip(df["recommendations"], want, lens):
        assert n == 5 and [i for i, _ in rec] == cand.item_ids[idx].tolist()
        assert np.array([s for _, s in rec], np.float64).tobytes() == val.tobytes()
