"""GPU: ALS predictions for (user, item) pairs (hrec_als_predict_pairs), the
fused regression sums (hrec_als_pair_metrics) and ALSModel.transform /
regression_metrics / evaluate.

Model: 37 users x 29 items, factors 0.3 N(0, 1) in f32 from a fixed seed, a
few entries set to 0, -0.0, a subnormal and 1e30 (never in the same column on
both sides, so no chain reaches inf - inf); the padding columns c >= k hold
7.0, so a chain that runs to kp is caught.

Reference: numpy on the host, vectorised over pairs and looped over c,
acc = f32(acc + f32(u[:, c] * v[:, c])): separate f32 operations round as the
JVM loop does. Predictions are compared bit for bit (uint32 views).

Metric tolerances. A sum of n positive f64 terms carries at most n 2^-53
relative error in any order (8e-12 at n = 70 000): sum e^2, sum |e|, sum y^2,
sum p^2, hence mse / rmse / mae, at rtol 1e-10; signed sums at 1e-10 of the
sum of their terms' magnitudes. 1 - r2 and var subtract: their error is that
of the sums times sum y^2 / sum (y - ybar)^2 and (sum p^2 + n ybar^2) / sum
(p - ybar)^2, asserted <= 10 on the host reference wherever at least two
rows are kept, so rtol 1e-9. (One row kept: sum (y - ybar)^2 is exactly 0 on
both sides, r2 is -inf or NaN on both sides, and var is compared as is.) The
API test's fitted model predicts near the labels, its var factor is about 20
at n = 97: the same rtol 1e-9 holds while factor * n 2^-53 <= 1e-10, which is
what that test asserts instead. The
expected values are math.fsum over the host reference, never the device's
own output. The rows holding 1e30 are left out of the metric pairs (one
prediction of 1e29 would be the whole of every sum and hide all others);
they are covered by the prediction tests."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS = 37, 29
KKP = [(1, 16), (10, 16), (17, 32), (64, 64), (65, 96), (128, 128), (256, 256)]
NS = [1, 63, 64, 65, 1000, 4097]
HUGE_USER, HUGE_ITEM = 11, 9
_MODELS = {}


def _hrec():
    from src import _hrec

    return _hrec


def _model(k, kp):
    """(U [37, kp], V [29, kp]) f32 on the host; built once per (k, kp)."""
    if (k, kp) not in _MODELS:
        rng = np.random.default_rng(1000 * k + kp)
        U = np.full((N_USERS, kp), 7.0, np.float32)
        V = np.full((N_ITEMS, kp), 7.0, np.float32)
        U[:, :k] = (0.3 * rng.standard_normal((N_USERS, k))).astype(np.float32)
        V[:, :k] = (0.3 * rng.standard_normal((N_ITEMS, k))).astype(np.float32)
        U[3, 0], U[5, 0], U[7, 0], U[HUGE_USER, 0] = 0.0, -0.0, 1e-40, 1e30
        V[2, 0], V[4, 0], V[6, 0] = -0.0, 0.0, 1e-41
        V[HUGE_ITEM, min(1, k - 1)] = 1e30 if k > 1 else 3.0
        U.setflags(write=False)
        V.setflags(write=False)
        _MODELS[(k, kp)] = (U, V)
    return _MODELS[(k, kp)]


def _chain(U, V, ur, ir, k):
    """The JVM chain of every pair on the host; NaN where a row is < 0."""
    ok = (ur >= 0) & (ir >= 0)
    u, v = U[np.where(ok, ur, 0)], V[np.where(ok, ir, 0)]
    acc = np.zeros(len(ur), np.float32)
    with np.errstate(all="ignore"):
        for c in range(k):
            acc = (acc + (u[:, c] * v[:, c]).astype(np.float32)).astype(np.float32)
    acc[~ok] = np.nan
    return acc


def _pairs(rng, n, users=N_USERS, items=N_ITEMS, unknown=0.1, marker=-1, skip_huge=False):
    ur = rng.integers(0, users, n).astype(np.int64)
    ir = rng.integers(0, items, n).astype(np.int64)
    if skip_huge:
        ur[ur == HUGE_USER] = 0
        ir[ir == HUGE_ITEM] = 0
    ur[rng.random(n) < unknown] = marker
    ir[rng.random(n) < unknown] = marker
    if n >= 1000:
        ur[5] = ir[5] = marker  # unknown on both sides
    return ur, ir


def _predict(h, device, U, V, ur, ir, k):
    out = h.als_predict_pairs(torch.as_tensor(U, device=device), torch.as_tensor(V, device=device),
                              torch.as_tensor(ur, device=device), torch.as_tensor(ir, device=device), k)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_bits(got, exp, ur, ir):
    assert got.dtype == np.float32 and got.shape == exp.shape
    unknown = (ur < 0) | (ir < 0)
    assert np.array_equal(np.isnan(got), unknown), "NaN exactly where a row is unknown"
    assert np.array_equal(got.view(np.uint32)[~unknown], exp.view(np.uint32)[~unknown])


# ------------------------------------------------------------- 1. predictions
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k,kp", KKP)
def test_predictions_are_bit_exact(device, k, kp, n):
    h = _hrec()
    U, V = _model(k, kp)
    ur, ir = _pairs(np.random.default_rng(7 * n + k), n)
    if n >= 1000:
        assert ((ur < 0) & (ir < 0)).any() and (ur >= 0).any()
    _assert_bits(_predict(h, device, U, V, ur, ir, k), _chain(U, V, ur, ir, k), ur, ir)


@pytest.mark.parametrize("case", ["one_user", "sorted_users", "int64_min_marker"])
def test_prediction_orders_and_markers(device, case):
    h = _hrec()
    k, kp = 64, 64
    U, V = _model(k, kp)
    rng = np.random.default_rng(11)
    ur, ir = _pairs(rng, 1000, marker=np.iinfo(np.int64).min if case == "int64_min_marker" else -1)
    if case == "one_user":
        ur[:] = 17
    elif case == "sorted_users":
        ur = np.sort(ur)
    _assert_bits(_predict(h, device, U, V, ur, ir, k), _chain(U, V, ur, ir, k), ur, ir)


# ------------------------------------------------- 2. the matrix path's bits
@pytest.mark.parametrize("k,kp", [(10, 16), (64, 64), (256, 256)])
def test_pairs_equal_the_score_matrix(device, k, kp):
    h = _hrec()
    U, V = (torch.as_tensor(a, device=device) for a in _model(k, kp))
    rows = torch.arange(N_USERS, device=device, dtype=torch.int64)
    full = h.als_score(U, rows, h.transpose(V), None, N_ITEMS, k)
    ur = rows.repeat_interleave(N_ITEMS)
    ir = torch.arange(N_ITEMS, device=device, dtype=torch.int64).repeat(N_USERS)
    got = h.als_predict_pairs(U, V, ur, ir, k).reshape(N_USERS, N_ITEMS)
    assert torch.equal(got.view(torch.int32), full.view(torch.int32))


# ------------------------------------------------------------------ 3. metrics
def _expected(pred, y, max_factor=10.0):
    """Counts, sums and metrics over the rows with a prediction, by fsum.
    max_factor: the largest cancellation factor the tolerances may assume."""
    ok = ~np.isnan(pred)
    p, yy = pred[ok].astype(np.float64), y[ok]
    e = yy - p
    n = int(ok.sum())
    s = {"n_ok": n, "n_nan": int((~ok).sum()), "sum_e": math.fsum(e), "sum_abs_e": math.fsum(np.abs(e)),
         "sum_e2": math.fsum(e * e), "sum_y": math.fsum(yy), "sum_y2": math.fsum(yy * yy), "sum_p": math.fsum(p),
         "sum_p2": math.fsum(p * p), "sum_yp": math.fsum(yy * p)}
    mag = {"sum_e": math.fsum(np.abs(e)), "sum_p": math.fsum(np.abs(p)), "sum_yp": math.fsum(np.abs(yy * p))}
    m = {}
    if n:
        ybar = s["sum_y"] / n
        ss_tot, ss_reg = math.fsum((yy - ybar) ** 2), math.fsum((p - ybar) ** 2)
        with np.errstate(all="ignore"):  # one row kept: ss_tot is 0
            m = {"mse": s["sum_e2"] / n, "rmse": math.sqrt(s["sum_e2"] / n), "mae": s["sum_abs_e"] / n,
                 "one_minus_r2": np.float64(s["sum_e2"]) / np.float64(ss_tot), "var": ss_reg / n}
        if n >= 2:
            assert ss_tot > 0 and ss_reg > 0
            factors = (s["sum_y2"] / ss_tot, (s["sum_p2"] + n * ybar * ybar) / ss_reg)
            print("cancellation factors of r2 / var:", factors)
            assert max(factors) <= max_factor, "the r2 / var tolerances assume smaller cancellation factors"
    return s, mag, m


def _check_metrics(got, m):
    for name in ("mse", "rmse", "mae"):
        np.testing.assert_allclose(got[name], m[name], rtol=1e-10, atol=0)
    with np.errstate(all="ignore"):
        np.testing.assert_allclose(1.0 - np.float64(got["r2"]), m["one_minus_r2"], rtol=1e-9, atol=0, equal_nan=True)
    np.testing.assert_allclose(got["var"], m["var"], rtol=1e-9, atol=0)


def _api_model(device, U, V, k):
    """An ALSModel over given factors; raw ids 100 + 3 row / 50 + 2 row."""
    from src.als_model import ALSModel, DeviceALSFactors, DeviceSession

    m = ALSModel(rank=k)
    m.spark = DeviceSession()
    m.model = DeviceALSFactors(100 + 3 * np.arange(N_USERS), 50 + 2 * np.arange(N_ITEMS),
                               torch.as_tensor(U, device=device), torch.as_tensor(V, device=device), k)
    return m


@pytest.mark.parametrize("n", [1, 65, 70000])
@pytest.mark.parametrize("k,kp", [(10, 16), (64, 64), (65, 96)])
def test_fused_metrics(device, k, kp, n):
    import pandas as pd

    h = _hrec()
    U, V = _model(k, kp)
    rng = np.random.default_rng(13 * n + k)
    ur, ir = _pairs(rng, n, skip_huge=True)
    if n == 1:
        ur[:], ir[:] = 4, 8  # the single pair is a known one
    y = rng.integers(2, 11, n).astype(np.float64) / 2.0  # 1.0, 1.5, ..., 5.0
    pred = _chain(U, V, ur, ir, k)
    s, mag, m = _expected(pred, y)
    dU, dV = torch.as_tensor(U, device=device), torch.as_tensor(V, device=device)
    dur, dir_, dy = (torch.as_tensor(a, device=device) for a in (ur, ir, y))
    pred_out = torch.full((n,), 5.0, device=device)
    a = h.als_pair_metrics(dU, dV, dur, dir_, k, dy, pred_out=pred_out)
    b = h.als_pair_metrics(dU, dV, dur, dir_, k, dy)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "two calls must give the same bits in every slot"
    got = dict(zip(h.PAIR_SUMS, a.tolist()))
    print("sums device / host:", {name: (got[name], s[name]) for name in h.PAIR_SUMS})
    assert got["n_ok"] == s["n_ok"] and got["n_nan"] == s["n_nan"] and got["n_ok"] + got["n_nan"] == n
    for name in ("sum_abs_e", "sum_e2", "sum_y", "sum_y2", "sum_p2"):
        np.testing.assert_allclose(got[name], s[name], rtol=1e-10, atol=0)
    for name in ("sum_e", "sum_p", "sum_yp"):
        assert abs(got[name] - s[name]) <= 1e-10 * mag[name]
    _assert_bits(pred_out.cpu().numpy(), pred, ur, ir)
    # the same through ALSModel.regression_metrics (raw ids; unknown ids -> rows of -1)
    model = _api_model(device, U, V, k)
    frame = pd.DataFrame({"userId": np.where(ur >= 0, 100 + 3 * ur, 7), "itemId": np.where(ir >= 0, 50 + 2 * ir, 51),
                          "rating": y})
    res = model.regression_metrics(frame, label_col="rating")
    print("metrics device / host:", res, m)
    assert res["count"] == s["n_ok"] and res["dropped"] == s["n_nan"]
    _check_metrics(res, m)
    for name in ("rmse", "mse", "mae", "r2", "var"):
        assert model.evaluate(frame, name, label_col="rating") == res[name] or math.isnan(res[name])


# ---------------------------------------------------------------------- 4. API
@pytest.fixture(scope="module")
def trained(device):
    import pandas as pd
    from src.als_model import ALSModel

    rng = np.random.default_rng(5)
    users = np.repeat(np.arange(20), 15) * 7 + 3
    items = np.tile(np.arange(15), 20) * 5 + 11
    keep = np.sort(rng.permutation(300)[:290])
    train = pd.DataFrame({"userId": users[keep], "itemId": items[keep],
                          "average_review_rating": rng.integers(2, 11, 290) / 2.0,
                          "rating": 3.0, "price": 1.0, "number_of_reviews": 2.0})
    model = ALSModel(rank=10, max_iter=2, seed=3)
    assert model.train(train)
    ev = train.iloc[::3].copy()
    extra = pd.DataFrame({"userId": [1000, 1001, 1000, 3, 10], "itemId": [11, 16, 21, 999, 998],
                          "average_review_rating": [4.0, 2.5, 1.0, 5.0, 3.5], "rating": 3.0, "price": 1.0,
                          "number_of_reviews": 2.0})
    ev = pd.concat([ev.iloc[:40], extra.iloc[:3], ev.iloc[40:], extra.iloc[3:]])
    ev.index = np.arange(len(ev)) * 2 + 5  # a non-default index
    return model, ev


def test_transform_and_cold_start_strategies(trained, device):
    model, ev = trained
    cold = ((ev["userId"] >= 1000) | (ev["itemId"] >= 998)).to_numpy()
    assert cold.sum() == 5
    model.cold_start_strategy = "nan"
    kept = model.transform(ev)
    assert list(kept.index) == list(ev.index) and kept["prediction"].dtype == np.float32
    assert np.array_equal(np.isnan(kept["prediction"].to_numpy()), cold)
    assert math.isnan(model.evaluate(ev))
    res = model.regression_metrics(ev)
    assert res["count"] == len(ev) and res["dropped"] == 0 and all(math.isnan(res[m]) for m in model.METRIC_NAMES)
    assert "prediction" not in ev.columns, "transform returns a copy"

    model.cold_start_strategy = "drop"
    out = model.transform(ev, prediction_col="p")
    assert list(out.index) == list(ev.index[~cold]) and list(out["userId"]) == list(ev["userId"][~cold])
    p = out["p"].to_numpy()
    assert p.dtype == np.float32 and not np.isnan(p).any()
    assert np.array_equal(p.view(np.uint32), kept["prediction"].to_numpy()[~cold].view(np.uint32))
    direct = model.model.predict_pairs(ev["userId"].to_numpy(), ev["itemId"].to_numpy()).cpu().numpy()
    assert np.array_equal(direct.view(np.uint32), kept["prediction"].to_numpy().view(np.uint32))
    res = model.regression_metrics(ev)
    assert res["dropped"] == 5 and res["count"] == len(ev) - 5
    # a fitted model predicts near the labels, so sum (p - ybar)^2 is small and var's factor passes 10;
    # the rtol 1e-9 of 1 - r2 and var needs factor * n 2^-53 <= 1e-10, i.e. a factor <= 1e-10 2^53 / n
    _, _, m = _expected(kept["prediction"].to_numpy(), ev["average_review_rating"].to_numpy(np.float64),
                        max_factor=1e-10 * 2.0 ** 53 / len(ev))
    _check_metrics(res, m)
    assert model.evaluate(ev, "mae") == res["mae"]
    # one known user: the ALS part of the score matrix, bit for bit
    u = int(ev["userId"].iloc[0])
    items = np.unique(ev["itemId"].to_numpy())
    row = model.model.score([u], items)[0].cpu().numpy()
    pairs = model.model.predict_pairs(np.full(len(items), u), items).cpu().numpy()
    assert np.array_equal(row.view(np.uint32), pairs.view(np.uint32)) and np.isnan(row).sum() == 2


def test_loaded_model_transforms_the_same_bits(trained, device, tmp_path):
    from src.als_model import ALSModel

    model, ev = trained
    model.cold_start_strategy = "drop"
    path = str(tmp_path / "als")
    model.save_model(path)
    loaded = ALSModel().load_model(path)
    assert loaded is not None
    a, b = model.transform(ev), loaded.transform(ev)
    assert list(a.index) == list(b.index)
    assert np.array_equal(a["prediction"].to_numpy().view(np.uint32), b["prediction"].to_numpy().view(np.uint32))
    assert loaded.regression_metrics(ev) == model.regression_metrics(ev)


def test_api_errors_and_empty_results(trained, device):
    import pandas as pd
    from src.als_model import ALSModel

    model, ev = trained
    model.cold_start_strategy = "drop"
    with pytest.raises(RuntimeError):
        ALSModel().transform(ev)
    with pytest.raises(RuntimeError):
        ALSModel().evaluate(ev)
    bad = ev.copy()
    bad["userId"] = bad["userId"] + 0.5
    with pytest.raises(ValueError):
        model.transform(bad)
    with pytest.raises(ValueError, match="rmse, mse, mae, r2, var"):
        model.evaluate(ev, "f1")
    model.cold_start_strategy = "keep"
    with pytest.raises(ValueError):
        model.transform(ev)
    model.cold_start_strategy = "drop"
    unknown = pd.DataFrame({"userId": [9001, 9002], "itemId": [11, 16], "average_review_rating": [1.0, 2.0]})
    res = model.regression_metrics(unknown)
    assert res["count"] == 0 and res["dropped"] == 2 and all(math.isnan(res[m]) for m in model.METRIC_NAMES)
    assert len(model.transform(unknown)) == 0
    empty = model.transform(ev.iloc[:0])
    assert len(empty) == 0 and "prediction" in empty.columns
    assert model.regression_metrics(ev.iloc[:0])["count"] == 0
