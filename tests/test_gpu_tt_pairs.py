"""GPU: two-tower scores for (user row, item row) pairs (hrec_tt_predict_pairs),
the fused regression sums (hrec_tt_pair_metrics) and TwoTowerModel.transform /
regression_metrics / evaluate.

Bit references, both older than the pair kernel: hrec_tt_pair_score on the
rows torch gathers, and the [u, i] entry of hrec_tt_score over the two tables
(7 user rows, 5 item rows, N(0, 1) in f32). The widths cover both chain
orders (32 / 64 / 128 / 256 permuted, the rest sequential), the three load
widths (d % 4 == 0, d % 2 == 0, odd) and a last chunk that is not full.

Sums: the expected value is numpy's f64 sum over the kernel's own f32
predictions; a sum of n f64 terms in any order is within n 2^-52 sum |terms|
of it (the bound of test_gramian_matches_f64), counts are exact.

API metrics: the formulas in numpy f64 over transform's predictions at rtol
1e-12. Only the summation order differs (and 1 - r2 / var subtract): the error
is at most n 2^-53 times the cancellation factors sum y^2 / sum (y - ybar)^2
and (sum p^2 + n ybar^2) / sum (p - ybar)^2, which the test asserts stay under
1e-12 / (n 2^-53)."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

pytestmark = pytest.mark.gpu

N_USER_ROWS, N_ITEM_ROWS = 7, 5
DS = [1, 3, 4, 16, 31, 32, 33, 50, 64, 65, 128, 255, 256]
NS = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
_TABLES = {}


def _hrec():
    from src import _hrec

    return _hrec


def _tables(device, d):
    """(U [7, d], V [5, d]) f32 on the device; built once per d, never written."""
    if d not in _TABLES:
        rng = np.random.default_rng(100 + d)
        _TABLES[d] = tuple(torch.as_tensor(rng.standard_normal((r, d)).astype(np.float32), device=device)
                           for r in (N_USER_ROWS, N_ITEM_ROWS))
    return _TABLES[d]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pairs(rng, n, device, last=False):
    ur = rng.integers(0, N_USER_ROWS, n).astype(np.int64)
    ir = rng.integers(0, N_ITEM_ROWS, n).astype(np.int64)
    if last:  # most pairs ask for the last row of each matrix: the read that ends at the allocation's end
        ur[rng.random(n) < 0.8] = N_USER_ROWS - 1
        ir[rng.random(n) < 0.8] = N_ITEM_ROWS - 1
    return torch.as_tensor(ur, device=device), torch.as_tensor(ir, device=device)


def _gathered(h, U, V, ur, ir):
    return h.tt_pair_score(U[ur].contiguous(), V[ir].contiguous())


# -------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("d", DS)
def test_pairs_have_the_bits_of_pair_score_and_score(device, d):
    h = _hrec()
    U, V = _tables(device, d)
    full = h.tt_score(U, V)
    assert full.shape == (N_USER_ROWS, N_ITEM_ROWS)
    rng = np.random.default_rng(7 * d)
    for n, last in [(n, False) for n in NS] + [(257, True)]:
        ur, ir = _pairs(rng, n, device, last)
        big = torch.full((n + 5,), 7.0, dtype=torch.float32, device=device)
        out = h.tt_predict_pairs(U, ur, V, ir, out=big[:n])
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and out.shape == (n,)
        assert torch.equal(big[n:], torch.full((5,), 7.0, device=device)), "rows beyond n are untouched"
        if n == 0:
            continue
        assert not torch.isnan(out).any()
        assert torch.equal(_bits(out), _bits(_gathered(h, U, V, ur, ir))), (d, n, "hrec_tt_pair_score")
        assert torch.equal(_bits(out), _bits(full[ur, ir])), (d, n, "hrec_tt_score")
        fresh = h.tt_predict_pairs(U, ur, V, ir)
        assert torch.equal(_bits(fresh), _bits(out))


def test_grid_stride_past_the_block_cap(device):
    h = _hrec()
    d, n = 16, 2048 * 256 + 257
    U, V = _tables(device, d)
    ur, ir = _pairs(np.random.default_rng(3), n, device)
    out = h.tt_predict_pairs(U, ur, V, ir)
    assert torch.equal(_bits(out), _bits(_gathered(h, U, V, ur, ir)))


# ------------------------------------------------------------- 2. bad indices
@pytest.mark.parametrize("d", [50, 64])
def test_bad_row_indices_give_nan_and_are_counted(device, d):
    h = _hrec()
    U, V = _tables(device, d)
    n = 130
    rng = np.random.default_rng(11 + d)
    ur, ir = _pairs(rng, n, device)
    good = _gathered(h, U, V, ur, ir)
    bad = [-1, None, 2 ** 62, -2 ** 63]
    where = {}
    for side, rows, n_rows, at in (("u", ur, N_USER_ROWS, 3), ("i", ir, N_ITEM_ROWS, 70)):
        for j, b in enumerate(bad):
            rows[at + 2 * j] = n_rows if b is None else b  # every other pair: each bad pair has good neighbours
            where[at + 2 * j] = side
    ur[127], ir[127] = -1, 2 ** 62  # bad on both sides
    where[127] = "ui"
    mask = torch.zeros(n, dtype=torch.bool, device=device)
    mask[list(where)] = True
    out = h.tt_predict_pairs(U, ur, V, ir)
    assert torch.equal(torch.isnan(out), mask), "NaN exactly at the bad pairs"
    assert torch.equal(_bits(out[~mask]), _bits(good[~mask])), "the neighbours keep their bits"
    y = torch.as_tensor(rng.random(n), device=device)
    pred = torch.empty(n, dtype=torch.float32, device=device)
    s = dict(zip(h.PAIR_SUMS, h.tt_pair_sums(U, ur, V, ir, y, pred_out=pred).tolist()))
    assert s["n_nan"] == len(where) and s["n_ok"] == n - len(where)
    assert torch.equal(_bits(pred[~mask]), _bits(good[~mask])) and torch.isnan(pred[mask]).all()
    assert all(math.isfinite(v) for v in s.values())


def test_a_nan_vector_row_is_counted_and_enters_no_sum(device):
    h = _hrec()
    d, n = 50, 300
    U, V = (t.clone() for t in _tables(device, d))
    U[2, 37] = float("nan")
    rng = np.random.default_rng(5)
    ur, ir = _pairs(rng, n, device)
    y = torch.as_tensor(rng.random(n) * 5, device=device)
    pred = torch.empty(n, dtype=torch.float32, device=device)
    s = dict(zip(h.PAIR_SUMS, h.tt_pair_sums(U, ur, V, ir, y, pred_out=pred).tolist()))
    hit = ur == 2
    assert 0 < int(hit.sum()) < n
    assert torch.equal(torch.isnan(pred), hit)
    assert s["n_nan"] == int(hit.sum()) and s["n_ok"] == n - int(hit.sum())
    p, yy = pred[~hit].cpu().numpy().astype(np.float64), y[~hit].cpu().numpy()
    for name, terms in _terms(p, yy).items():
        assert abs(s[name] - terms.sum()) <= n * 2.0 ** -52 * np.abs(terms).sum(), name


# -------------------------------------------------------------------- 3. sums
def _terms(p, y):
    e = y - p
    return {"sum_e": e, "sum_abs_e": np.abs(e), "sum_e2": e * e, "sum_y": y, "sum_y2": y * y, "sum_p": p,
            "sum_p2": p * p, "sum_yp": y * p}


@pytest.mark.parametrize("n", [0, 1, 257, 70001])
@pytest.mark.parametrize("d", [50, 64])
def test_fused_sums(device, d, n):
    h = _hrec()
    U, V = _tables(device, d)
    rng = np.random.default_rng(13 * n + d)
    ur, ir = _pairs(rng, n, device)
    if n > 1:
        ur[n // 2] = -1  # one pair without a prediction
    y = torch.as_tensor(rng.integers(0, 11, n).astype(np.float64) / 2.0, device=device)
    pred = torch.full((n,), 9.0, dtype=torch.float32, device=device)
    a = h.tt_pair_sums(U, ur, V, ir, y, pred_out=pred)
    b = h.tt_pair_sums(U, ur, V, ir, y, pred_out=pred)
    c = h.tt_pair_sums(U, ur, V, ir, y)
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and a.shape == (len(h.PAIR_SUMS),)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two calls give equal bits"
    assert torch.equal(a.view(torch.int64), c.view(torch.int64)), "pred_out=None gives the same sums"
    assert torch.equal(_bits(pred), _bits(h.tt_predict_pairs(U, ur, V, ir))), "the stored predictions are predict's"
    got = dict(zip(h.PAIR_SUMS, a.tolist()))
    p_all, y_all = pred.cpu().numpy(), y.cpu().numpy()
    ok = ~np.isnan(p_all)
    assert got["n_ok"] == int(ok.sum()) and got["n_nan"] == int((~ok).sum()) == int(n > 1)
    for name, terms in _terms(p_all[ok].astype(np.float64), y_all[ok]).items():
        bound = n * 2.0 ** -52 * np.abs(terms).sum()
        print(name, got[name], terms.sum(), bound)
        assert abs(got[name] - terms.sum()) <= bound, name


# --------------------------------------------------------------------- 4. API
N_USERS, N_ITEMS = 60, 40
ITEM_COLS = ["itemId", "manufacturer_id", "category_id", "price", "average_review_rating"]


class Setup:
    """A TwoTowerModel at its initial weights, an item table of 40 shuffled
    ids, and a frame of (user, item) rows with the items' columns: users
    repeat, one (user, item) row appears twice, the index is not the default.
    predict_for_user's score of every (user, position) over the frame and of
    every (user, itemId) over the candidate frame are computed once."""

    def __init__(self, device, d):
        from sklearn.preprocessing import MinMaxScaler
        from src.two_tower_model import TwoTowerModel

        rng = np.random.default_rng(d)
        self.tt = TwoTowerModel(N_USERS, N_ITEMS + 8, 6, 4, embedding_size=d, seed=d)
        self.tt.build_model()
        self.items = pd.DataFrame({"itemId": rng.permutation(N_ITEMS).astype(np.int64),
                                   "manufacturer_id": rng.integers(0, 6, N_ITEMS),
                                   "category_id": rng.integers(0, 4, N_ITEMS), "price": rng.random(N_ITEMS) * 100,
                                   "average_review_rating": rng.integers(0, 11, N_ITEMS).astype(np.float64) / 2})
        self.tt.scaler = MinMaxScaler().fit(self.items[["price", "average_review_rating"]])
        n = 240
        rows = rng.integers(0, N_ITEMS, n)
        frame = self.items.iloc[rows].reset_index(drop=True)
        frame.insert(0, "userId", rng.integers(0, N_USERS, n).astype(np.int64))
        frame = pd.concat([frame, frame.iloc[[17]]], ignore_index=True)  # the duplicate (user, item) row
        frame.index = np.arange(len(frame)) * 3 + 2
        self.frame = frame
        self.missing = int(self.items["itemId"].iloc[9])
        self.cand_frame = self.items[self.items["itemId"] != self.missing].reset_index(drop=True)
        self.by_position, self.by_item = {}, {}
        for u in np.unique(frame["userId"]).tolist():
            self.by_position[u] = np.array([s for _, s in self.tt.predict_for_user(u, frame)], np.float32)
            self.by_item[u] = dict(self.tt.predict_for_user(u, self.cand_frame))


_SETUPS = {}


@pytest.fixture(params=[50, 64])
def setup(request, device):
    if request.param not in _SETUPS:
        _SETUPS[request.param] = Setup(device, request.param)
    return _SETUPS[request.param]


def test_transform_has_predict_for_user_bits(setup):
    tt, frame = setup.tt, setup.frame
    out = tt.transform(frame)
    assert "prediction" not in frame.columns, "transform returns a copy"
    assert list(out.index) == list(frame.index) and list(out.columns) == list(frame.columns) + ["prediction"]
    p = out["prediction"].to_numpy()
    assert p.dtype == np.float32 and not np.isnan(p).any()
    exp = np.array([setup.by_position[u][pos] for pos, u in enumerate(frame["userId"].tolist())], np.float32)
    assert np.array_equal(p.view(np.uint32), exp.view(np.uint32))
    assert p[17].view(np.uint32) == p[-1].view(np.uint32), "the duplicate row"
    named = tt.transform(frame, prediction_col="p")
    assert np.array_equal(named["p"].to_numpy().view(np.uint32), p.view(np.uint32))


def test_transform_over_candidates(setup):
    tt = setup.tt
    data = setup.frame[["userId", "itemId"]]
    gone = (data["itemId"] == setup.missing).to_numpy()
    assert 0 < gone.sum() < len(data)
    for cand in (setup.cand_frame, tt.candidates(setup.cand_frame)):
        out = tt.transform(data, candidates=cand)
        p = out["prediction"].to_numpy()
        assert p.dtype == np.float32 and np.array_equal(np.isnan(p), gone), "NaN exactly at the missing item"
        exp = np.array([setup.by_item[u].get(i, np.float32("nan"))
                        for u, i in zip(data["userId"].tolist(), data["itemId"].tolist())], np.float32)
        assert np.array_equal(p[~gone].view(np.uint32), exp[~gone].view(np.uint32))
        res = tt.regression_metrics(setup.frame, candidates=cand)
        assert res["dropped"] == int(gone.sum()) and res["count"] == len(data) - int(gone.sum())
        _check_formulas(res, p[~gone], setup.frame["average_review_rating"].to_numpy(np.float64)[~gone])


def _check_formulas(res, p, y, rtol=1e-12):
    p = p.astype(np.float64)
    n, e, ybar = len(y), y - p, y.mean()
    ss_tot, ss_reg = ((y - ybar) ** 2).sum(), ((p - ybar) ** 2).sum()
    factors = ((y * y).sum() / ss_tot, ((p * p).sum() + n * ybar * ybar) / ss_reg)
    print("cancellation factors of r2 / var:", factors, "metrics:", res)
    assert max(factors) * n * 2.0 ** -53 <= rtol, "rtol assumes smaller cancellation factors"
    exp = {"mse": (e * e).mean(), "rmse": math.sqrt((e * e).mean()), "mae": np.abs(e).mean(),
           "r2": 1.0 - (e * e).sum() / ss_tot, "var": ss_reg / n}
    for name, v in exp.items():
        np.testing.assert_allclose(res[name], v, rtol=rtol, atol=0, err_msg=name)


def test_regression_metrics_and_evaluate(setup):
    tt, frame = setup.tt, setup.frame
    res = tt.regression_metrics(frame)
    assert set(res) == {"rmse", "mse", "mae", "r2", "var", "count", "dropped"}
    assert res["count"] == len(frame) and res["dropped"] == 0
    p = tt.transform(frame)["prediction"].to_numpy()
    _check_formulas(res, p, frame["average_review_rating"].to_numpy(np.float64))
    assert tt.evaluate(frame, "mae") == res["mae"]
    assert tt.evaluate(frame) == res["rmse"]
    other = frame.assign(stars=frame["average_review_rating"] * 2 - 1)
    res2 = tt.regression_metrics(other, label_col="stars")
    _check_formulas(res2, p, other["stars"].to_numpy(np.float64))
    assert tt.evaluate(other, "mse", label_col="stars") == res2["mse"]
    with pytest.raises(ValueError, match="rmse, mse, mae, r2, var"):
        tt.evaluate(frame, "f1")


def test_api_errors_and_empty_frames(setup):
    from src.two_tower_model import TwoTowerModel

    tt, frame = setup.tt, setup.frame
    with pytest.raises(RuntimeError):
        TwoTowerModel(5, 5, 2, 2).transform(frame)
    twice = pd.concat([setup.cand_frame, setup.cand_frame.iloc[[3]]], ignore_index=True)
    with pytest.raises(ValueError, match="repeats an itemId"):
        tt.transform(frame[["userId", "itemId"]], candidates=twice)
    for bad_user in (N_USERS, -1):
        bad = frame.copy()
        bad.iloc[5, bad.columns.get_loc("userId")] = bad_user
        with pytest.raises(IndexError):
            tt.transform(bad)
        with pytest.raises(IndexError):
            tt.regression_metrics(bad[["userId", "itemId", "average_review_rating"]], candidates=setup.cand_frame)
    for cand in (None, setup.cand_frame):
        empty = tt.transform(frame.iloc[:0], candidates=cand)
        assert len(empty) == 0 and empty["prediction"].dtype == np.float32
        res = tt.regression_metrics(frame.iloc[:0], candidates=cand)
        assert res["count"] == 0 and res["dropped"] == 0 and all(math.isnan(res[m]) for m in tt.METRIC_NAMES)


def test_engine_runs_the_user_tower_once_per_distinct_user(setup, monkeypatch):
    tt, frame = setup.tt, setup.frame
    seen = []
    real = tt.model.user_vectors
    monkeypatch.setattr(tt.model, "user_vectors", lambda user: (seen.append(int(user.numel())), real(user))[1])
    tt.transform(frame)
    assert seen == [int(frame["userId"].nunique())]


# ------------------------------------------- 5. the ALS metrics keep their values
@pytest.mark.parametrize("strategy", ["drop", "nan"])
def test_als_regression_metrics_unchanged_by_the_shared_helper(device, strategy):
    from src.als_model import ALSModel, DeviceALSFactors, DeviceSession

    rng = np.random.default_rng(2)
    k, kp, nu, ni, n = 10, 16, 37, 29, 97
    U, V = np.zeros((nu, kp), np.float32), np.zeros((ni, kp), np.float32)
    U[:, :k], V[:, :k] = rng.standard_normal((nu, k)) * 0.5, rng.standard_normal((ni, k)) * 0.5
    m = ALSModel(rank=k)
    m.spark = DeviceSession()
    m.model = DeviceALSFactors(100 + 3 * np.arange(nu), 50 + 2 * np.arange(ni), torch.as_tensor(U, device=device),
                               torch.as_tensor(V, device=device), k)
    m.cold_start_strategy = strategy
    frame = pd.DataFrame({"userId": 100 + 3 * rng.integers(0, nu, n), "itemId": 50 + 2 * rng.integers(0, ni, n),
                          "average_review_rating": rng.integers(2, 11, n) / 2.0})
    m.cold_start_strategy = "nan"
    p = m.transform(frame)["prediction"].to_numpy()
    m.cold_start_strategy = strategy
    res = m.regression_metrics(frame)
    assert res["count"] == n and res["dropped"] == 0
    _check_formulas(res, p, frame["average_review_rating"].to_numpy(np.float64), rtol=1e-9)
    cold = pd.concat([frame, pd.DataFrame({"userId": [7, 100], "itemId": [50, 51],
                                           "average_review_rating": [1.0, 2.0]})], ignore_index=True)
    res = m.regression_metrics(cold)
    if strategy == "nan":
        assert res["count"] == n + 2 and res["dropped"] == 0 and all(math.isnan(res[x]) for x in m.METRIC_NAMES)
    else:
        assert res["count"] == n and res["dropped"] == 2
        _check_formulas(res, p, frame["average_review_rating"].to_numpy(np.float64), rtol=1e-9)
    assert m.evaluate(frame, "mae") == m.regression_metrics(frame)["mae"]
