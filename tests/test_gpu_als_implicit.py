"""GPU: implicit-feedback ALS (Spark implicitPrefs / alpha) — the source
Gramian, one half-sweep, the engine fit and the ALSModel API against the f64
numpy restatement in tests/implicit_oracle.py. YtY's summation order differs
from the oracle's, so these are tolerance checks (the project's ALS
tolerances: one sweep rtol 1e-5 / atol 1e-6, a fit rtol 1e-4 / atol 1e-5)."""
import numpy as np
import pytest
import torch

import implicit_oracle as io

pytestmark = pytest.mark.gpu

KKP = [(10, 16), (16, 16), (20, 32), (33, 64), (64, 64)]
RATINGS = np.array([-2, -0.5, 0, 0.5, 1, 1.5, 2, 2.5, 3, 3.5, 4, 4.5, 5], np.float32)


def _hrec():
    from src import _hrec

    return _hrec


def _src(rng, n_src, k, kp):
    src = np.zeros((n_src, kp), np.float32)
    src[:, :k] = (rng.normal(size=(n_src, k)) / np.sqrt(k)).astype(np.float32)
    return src


# ---------------------------------------------------------------- Gramian
@pytest.mark.parametrize("k,kp", KKP)
@pytest.mark.parametrize("n_src", [1, 3, 63, 64, 65, 1000, 4099])
def test_gramian_matches_f64(device, n_src, k, kp):
    h = _hrec()
    S = _src(np.random.default_rng(n_src + k), n_src, k, kp)
    d = torch.as_tensor(S, device=device)
    got_t = h.als_gramian(d, k)
    again = h.als_gramian(d, k)
    assert got_t.dtype == torch.float64 and tuple(got_t.shape) == (kp, kp)
    assert torch.equal(got_t, again), "two calls must give the same bits"
    got = got_t.cpu().numpy()
    S64 = S.astype(np.float64)
    exp = S64.T @ S64
    bound = n_src * 2.0 ** -52 * (np.abs(S64).T @ np.abs(S64))
    err = np.abs(got - exp)
    print("gramian max err / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    assert (got[k:, :] == 0).all() and (got[:, k:] == 0).all(), "padding rows and columns must be zero"
    assert np.array_equal(got, got.T)


# ------------------------------------------------------------- half-sweep
DEG = [0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 200, 6, 6]


def _sweep_problem(k, kp):
    rng = np.random.default_rng(100 + k)
    n_src = max(2 * k, 140)
    indptr = np.concatenate([[0], np.cumsum(DEG)]).astype(np.int64)
    indices = rng.integers(0, n_src, indptr[-1]).astype(np.int32)
    indices[::7] = n_src - 1
    indices[3::11] = 0
    values = rng.choice(RATINGS, indptr[-1]).astype(np.float32)
    r = len(DEG) - 2  # a row whose ratings are all <= 0
    values[indptr[r]: indptr[r + 1]] = np.array([-2, -0.5, 0, 0, -2, -0.5], np.float32)
    r += 1            # a row with duplicate column entries
    indices[indptr[r]: indptr[r + 1]] = np.array([5, 5, 9, 5, 9, 11], np.int32)
    values[indptr[r]: indptr[r + 1]] = np.array([1, 3, -2, 1, 0.5, 4], np.float32)
    return indptr, indices, values, _src(rng, n_src, k, kp)


@pytest.mark.parametrize("alpha", [0.0, 1.0, 40.0])
@pytest.mark.parametrize("k,kp", KKP)
def test_implicit_half_sweep_matches_oracle(device, k, kp, alpha):
    h = _hrec()
    indptr, indices, values, src = _sweep_problem(k, kp)
    d_ip = torch.as_tensor(indptr, device=device)
    d_ix = torch.as_tensor(indices, device=device)
    d_v = torch.as_tensor(values, device=device)
    d_src = torch.as_tensor(src, device=device)
    yty = h.als_gramian(d_src, k)
    dst = torch.full((len(DEG), kp), 3.0, device=device)
    h.als_half_sweep_implicit(d_ip, d_ix, d_v, d_src, k, 0.1, alpha, yty, dst)
    got = dst.cpu().numpy()
    exp = io.half_sweep(indptr, indices, values, src, k, 0.1, alpha)
    print("half-sweep max abs err:", float(np.abs(got[:, :k] - exp).max()))
    np.testing.assert_allclose(got[:, :k], exp, rtol=1e-5, atol=1e-6)
    assert (got[:, k:] == 0).all(), "padding columns must stay zero"
    assert (got[0] == 0).all(), "a row without ratings has no factor"
    assert (got[len(DEG) - 2] == 0).all(), "ratings all <= 0: the factor is exactly zero"
    # not a pass-through to the explicit kernel
    exp_dst = torch.zeros((len(DEG), kp), device=device)
    h.als_half_sweep(d_ip, d_ix, d_v, d_src, k, 0.1, exp_dst)
    assert not np.allclose(got[:, :k], exp_dst.cpu().numpy()[:, :k], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------- engine fit
def _host_csr(c):
    return c.indptr.cpu().numpy(), c.indices.cpu().numpy(), c.values.cpu().numpy()


@pytest.mark.parametrize("n_users,n_items,dens,k,alpha", [(400, 300, 0.05, 16, 1.0), (300, 200, 0.05, 64, 40.0)])
def test_engine_implicit_fit_matches_oracle(device, n_users, n_items, dens, k, alpha):
    from src import synthetic
    from src.als_engine import DeviceALS

    csr = synthetic.generate(n_users, n_items, dens, False)
    csc = synthetic.generate(n_users, n_items, dens, True)
    eng = DeviceALS(n_users, n_items, k, 0.1, csr, csc, implicit=True, alpha=alpha)
    eng.init_user_factors(synthetic.SEED_INIT)
    U0 = eng.user_factors.cpu().numpy().copy()
    eng.fit(3)
    assert eng._s64 is None  # the f64-source shortcut is off
    U, V = io.fit(_host_csr(csr), _host_csr(csc), U0, k, 0.1, alpha, 3)
    np.testing.assert_allclose(eng.item_factors.cpu().numpy(), V, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(eng.user_factors.cpu().numpy(), U, rtol=1e-4, atol=1e-5)


def test_engine_implicit_limits():
    from src.als_engine import DeviceALS
    from src.synthetic import DeviceCSR

    z = torch.zeros(2, dtype=torch.int64)
    e = DeviceCSR(z, torch.zeros(0, dtype=torch.int32), torch.zeros(0), 0, 1, 1)
    with pytest.raises(ValueError, match="rank <= 64"):
        DeviceALS(1, 1, 100, 0.1, e, e, implicit=True)
    with pytest.raises(ValueError, match="accum_mode 0"):
        DeviceALS(1, 1, 8, 0.1, e, e, implicit=True, accum_mode=1)
    with pytest.raises(ValueError, match="alpha >= 0"):
        DeviceALS(1, 1, 8, 0.1, e, e, implicit=True, alpha=-1.0)


# -------------------------------------------------------------------- API
def _frame():
    import pandas as pd

    rng = np.random.default_rng(21)
    n_u, n_i, nnz = 60, 40, 600
    u = rng.integers(0, n_u, nnz)
    i = rng.integers(0, n_i, nnz)
    r = rng.choice(RATINGS[3:], nnz).astype(np.float64)
    u[:n_u], i[:n_i] = np.arange(n_u), np.arange(n_i)  # every id present
    u[100], i[100] = u[101], i[101]                    # a duplicate (u, i) pair
    r[102], r[103] = 0.0, -2.0
    order = np.argsort(u, kind="stable")
    u, i, r = u[order], i[order], r[order]
    return pd.DataFrame({"userId": u * 3 + 7, "itemId": i * 2 + 100, "average_review_rating": r,
                         "manufacturer": "m", "amazon_category_and_sub_category": "c", "price": 1.0,
                         "number_of_reviews": 1.0}), u, i, r, n_u, n_i


def test_alsmodel_implicit_prefs(device, tmp_path, capsys):
    from src.als_model import ALSModel

    frame, u, i, r, n_u, n_i = _frame()
    k, alpha = 10, 40.0
    U0 = (np.random.default_rng(3).normal(size=(n_u, k)) / np.sqrt(k)).astype(np.float32)
    model = ALSModel(rank=k, max_iter=3, implicit_prefs=True, alpha=alpha)
    assert model.train(frame, initial_user_factors=U0), capsys.readouterr().out
    U, V = io.fit(io.coo_to_csr(u, i, r, n_u), io.coo_to_csr(i, u, r, n_i), U0, k, 0.1, alpha, 3)
    Ug, Vg = model.model.U[:, :k].cpu().numpy(), model.model.V[:, :k].cpu().numpy()
    np.testing.assert_allclose(Vg, V, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(Ug, U, rtol=1e-4, atol=1e-5)
    items = [int(x) for x in np.arange(n_i) * 2 + 100]
    preds = model.predict_for_user(7 + 3 * 5, items)
    assert [p[0] for p in preds] == items
    want = U[5].astype(np.float64) @ V.T.astype(np.float64)
    np.testing.assert_allclose([p[1] for p in preds], want, rtol=1e-4, atol=1e-6 * np.abs(want).max())
    path = str(tmp_path / "als")
    model.save_model(path)
    back = ALSModel().load_model(path)
    assert back is not None and back.implicit_prefs is True and back.alpha == alpha
    assert torch.equal(back.model.U[:, :k], model.model.U[:, :k])
    assert torch.equal(back.model.V[:, :k], model.model.V[:, :k])
    capsys.readouterr()
    assert ALSModel(rank=100, implicit_prefs=True).train(frame) is False
    assert "rank <= 64" in capsys.readouterr().out


def test_alsmodel_explicit_default_unchanged(device):
    from src.als_model import ALSModel

    frame = _frame()[0]
    a, b = ALSModel(rank=10, max_iter=2, seed=5), ALSModel(rank=10, max_iter=2, seed=5, implicit_prefs=False)
    assert a.train(frame) and b.train(frame)
    assert torch.equal(a.model.U, b.model.U) and torch.equal(a.model.V, b.model.V)
