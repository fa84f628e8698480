"""GPU: non-negative ALS (Spark nonnegative=True) — one half-sweep, the engine
fit and the ALSModel API against the f64 numpy restatement of Spark's NNLS in
tests/nnls_oracle.py (itself checked against exact NNLS in
tests/test_nnls_oracle.py).

Tolerances. One sweep: per row |got - exp| <= 1e-5 max|exp_row| + 1e-6 (the
solver stops on a norm, ||dir||^2 < 1e-12 ||x||^2, so the small entries of a
row carry the row's absolute error). A fit: the project's rtol 1e-4 / atol
1e-5. Two summation orders of the oracle stay within a tenth of both."""
import numpy as np
import pytest
import torch

import nnls_oracle as no

pytestmark = pytest.mark.gpu

REG, ALPHA = 0.1, 40.0
LONG = [r for r, d in enumerate(no.DEG) if d >= 63]


def _hrec():
    from src import _hrec

    return _hrec


def _row_bound(exp):
    return 1e-5 * np.abs(exp).max(axis=1, keepdims=True) + 1e-6


def _run(h, device, prob, k, kp, imp):
    """(nonneg result [rows, kp], iterations, Cholesky result [rows, kp]) on the device."""
    indptr, indices, values, src = prob
    d_ip = torch.as_tensor(indptr, device=device)
    d_ix = torch.as_tensor(indices, device=device)
    d_v = torch.as_tensor(values, device=device)
    d_src = torch.as_tensor(src, device=device)
    n = len(no.DEG)
    yty = h.als_gramian(d_src, k) if imp else None
    outs = []
    for _ in range(2):
        dst = torch.full((n, kp), 3.0, device=device)
        iters = torch.full((n,), -1, dtype=torch.int32, device=device)
        h.als_half_sweep_nonneg(d_ip, d_ix, d_v, d_src, k, REG, dst, implicit=imp, alpha=ALPHA if imp else 0.0,
                                yty=yty, iters=iters)
        outs.append((dst, iters))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), \
        "two calls must give the same bits"
    chol = torch.zeros((n, kp), device=device)
    if imp:
        h.als_half_sweep_implicit(d_ip, d_ix, d_v, d_src, k, REG, ALPHA, yty, chol)
    else:
        h.als_half_sweep(d_ip, d_ix, d_v, d_src, k, REG, chol)
    no_iters = torch.full((n, kp), 3.0, device=device)  # iters_out is optional
    h.als_half_sweep_nonneg(d_ip, d_ix, d_v, d_src, k, REG, no_iters, implicit=imp, alpha=ALPHA if imp else 0.0,
                            yty=yty)
    assert torch.equal(no_iters, outs[0][0])
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy(), chol.cpu().numpy()


def _check_against_oracle(got, iters, exp, exp_iters, k):
    err = np.abs(got[:, :k] - exp)
    print("half-sweep worst err / bound:", float((err / _row_bound(exp)).max()),
          "iterations gpu / oracle:", iters.tolist(), exp_iters.tolist())
    assert (got >= 0).all(), "every factor is >= 0, exactly"
    assert (got[:, k:] == 0).all(), "padding columns must stay zero"
    assert (got[0] == 0).all() and iters[0] == 0, "a row without ratings has no factor"
    assert (err <= _row_bound(exp)).all()
    assert (iters >= 0).all() and (iters <= max(400, 20 * k)).all()
    assert (iters[exp_iters > 0] > 0).all(), "solved rows take iterations"
    assert (iters[exp_iters == 0] == 0).all()


@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("k,kp", no.KKP)
def test_nonneg_half_sweep_signed_sources(device, k, kp, imp):
    """About half of every row's entries sit at the bound; the Cholesky
    half-sweep of the same rows has negative entries."""
    h = _hrec()
    prob = no.sweep_problem(k, kp, True)
    got, iters, chol = _run(h, device, prob, k, kp, imp)
    exp, exp_iters = no.half_sweep(*prob, k, REG, imp, ALPHA, return_iters=True)
    _check_against_oracle(got, iters, exp, exp_iters, k)
    solved = np.flatnonzero(exp_iters > 0)
    assert len(solved) >= 10 and all((exp[r] == 0).any() for r in solved), "the oracle has exact zeros in these rows"
    assert (got[solved, :k] == 0).mean() > 0.25
    if imp:
        assert (got[no.ROW_NONPOS] == 0).all() and iters[no.ROW_NONPOS] == 0, "ratings all <= 0: exactly zero"
    # the solver swap is real: the unconstrained solution is signed and differs
    assert (chol[:, :k] < 0).any()
    assert not np.allclose(got[:, :k], chol[:, :k], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("k,kp", no.KKP)
def test_nonneg_half_sweep_nonnegative_sources(device, k, kp, imp):
    """|Gaussian| sources, positive ratings: where no bound is active NNLS is
    the Cholesky solution. Explicit: every long row; implicit: the long rows
    in which the oracle has no entry at the bound (implicit solutions of long
    rows do touch it)."""
    h = _hrec()
    prob = no.sweep_problem(k, kp, False)
    got, iters, chol = _run(h, device, prob, k, kp, imp)
    exp, exp_iters = no.half_sweep(*prob, k, REG, imp, ALPHA, return_iters=True)
    _check_against_oracle(got, iters, exp, exp_iters, k)
    # all ratings < 0 over sources >= 0: b <= 0 (implicit: no rating > 0), exactly zero after 0 iterations
    assert (got[no.ROW_NONPOS] == 0).all() and iters[no.ROW_NONPOS] == 0
    assert iters[no.ROW_DUP] > 0
    free = [r for r in LONG if (exp[r] > 0).all()]
    print("long rows without an active bound:", free)
    if not imp:
        assert free == LONG
    if free:
        err = np.abs(got[free, :k] - chol[free, :k])
        assert (err <= _row_bound(chol[free, :k])).all(), "unconstrained rows: NNLS agrees with Cholesky"


# ------------------------------------------------------------- engine fit
@pytest.mark.parametrize("n_users,n_items,dens,k,imp", [(400, 300, 0.05, 16, False), (300, 200, 0.05, 64, True),
                                                        (300, 200, 0.05, 64, False)])
def test_engine_nonneg_fit_matches_oracle(device, n_users, n_items, dens, k, imp):
    from src import synthetic
    from src.als_engine import DeviceALS

    csr = synthetic.generate(n_users, n_items, dens, False)
    csc = synthetic.generate(n_users, n_items, dens, True)
    eng = DeviceALS(n_users, n_items, k, REG, csr, csc, implicit=imp, alpha=ALPHA, nonnegative=True)
    eng.init_user_factors(synthetic.SEED_INIT)
    ucsr, _, U0, U, V = no.synthetic_fit(n_users, n_items, dens, k, imp, ALPHA)
    assert np.array_equal(eng.user_factors.cpu().numpy(), U0)
    assert np.array_equal(csr.indptr.cpu().numpy(), ucsr[0]) and np.array_equal(csr.indices.cpu().numpy(), ucsr[1])
    eng.fit(3)
    assert eng._s64 is None  # the f64-source shortcut is off
    Ug, Vg = eng.user_factors.cpu().numpy(), eng.item_factors.cpu().numpy()
    for g, e in ((Vg, V), (Ug, U)):
        print("fit worst err / tol:", float((np.abs(g - e.astype(np.float64)) / (1e-5 + 1e-4 * np.abs(e))).max()),
              "share of zeros:", float((g == 0).mean()))
    np.testing.assert_allclose(Vg, V, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(Ug, U, rtol=1e-4, atol=1e-5)
    assert (eng.U >= 0).all() and (eng.V >= 0).all(), "no factor is negative"
    assert (Ug == 0).mean() > 0.05 and (Vg == 0).mean() > 0.05, "a real share of the factors is at the bound"


def test_engine_nonneg_limits():
    from src.als_engine import DeviceALS
    from src.synthetic import DeviceCSR

    z = torch.zeros(2, dtype=torch.int64)
    e = DeviceCSR(z, torch.zeros(0, dtype=torch.int32), torch.zeros(0), 0, 1, 1)
    with pytest.raises(ValueError, match="nonnegative supports rank <= 64"):
        DeviceALS(1, 1, 100, 0.1, e, e, nonnegative=True)
    with pytest.raises(ValueError, match="nonnegative supports accum_mode 0"):
        DeviceALS(1, 1, 8, 0.1, e, e, nonnegative=True, accum_mode=1)


# -------------------------------------------------------------------- API
def _frame():
    """The 60 x 40 frame of the implicit API test."""
    import pandas as pd

    rng = np.random.default_rng(21)
    n_u, n_i, nnz = 60, 40, 600
    u = rng.integers(0, n_u, nnz)
    i = rng.integers(0, n_i, nnz)
    r = rng.choice(no.RATINGS[3:], nnz).astype(np.float64)
    u[:n_u], i[:n_i] = np.arange(n_u), np.arange(n_i)  # every id present
    u[100], i[100] = u[101], i[101]                    # a duplicate (u, i) pair
    r[102], r[103] = 0.0, -2.0
    order = np.argsort(u, kind="stable")
    u, i, r = u[order], i[order], r[order]
    return pd.DataFrame({"userId": u * 3 + 7, "itemId": i * 2 + 100, "average_review_rating": r,
                         "manufacturer": "m", "amazon_category_and_sub_category": "c", "price": 1.0,
                         "number_of_reviews": 1.0}), u, i, r, n_u, n_i


@pytest.mark.parametrize("imp", [False, True])
def test_alsmodel_nonnegative(device, tmp_path, capsys, imp):
    from src.als_model import ALSModel

    frame, u, i, r, n_u, n_i = _frame()
    k = 10
    U0 = (np.random.default_rng(3).normal(size=(n_u, k)) / np.sqrt(k)).astype(np.float32)
    model = ALSModel(rank=k, max_iter=3, implicit_prefs=imp, alpha=ALPHA, nonnegative=True)
    assert model.train(frame, initial_user_factors=U0), capsys.readouterr().out
    U, V = no.fit(no.coo_to_csr(u, i, r, n_u), no.coo_to_csr(i, u, r, n_i), U0, k, 0.1, 3, imp, ALPHA)
    Ug, Vg = model.model.U[:, :k].cpu().numpy(), model.model.V[:, :k].cpu().numpy()
    np.testing.assert_allclose(Vg, V, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(Ug, U, rtol=1e-4, atol=1e-5)
    assert (Ug >= 0).all() and (Vg >= 0).all() and (Ug == 0).any() and (Vg == 0).any()
    items = [int(x) for x in np.arange(n_i) * 2 + 100]
    for user in range(0, n_u, 7):
        preds = model.predict_for_user(7 + 3 * user, items)
        assert [p[0] for p in preds] == items
        assert all(p[1] >= 0 for p in preds), "non-negative factors give non-negative scores"
    want = U[5].astype(np.float64) @ V.T.astype(np.float64)
    preds = model.predict_for_user(7 + 3 * 5, items)
    # factors within the fit tolerance (rtol 1e-4, atol 1e-5), all terms >= 0:
    # |d(u.v)| <= 2 rtol u.v + atol (|u|_1 + |v|_1), plus the f32 dot's rounding (k 2^-24 u.v)
    tol = 2.1e-4 * want + 1e-5 * (U[5].sum(dtype=np.float64) + V.sum(axis=1, dtype=np.float64))
    assert (np.abs(np.array([p[1] for p in preds]) - want) <= tol).all()
    path = str(tmp_path / "als")
    model.save_model(path)
    back = ALSModel().load_model(path)
    assert back is not None and back.nonnegative is True and back.implicit_prefs is imp
    assert torch.equal(back.model.U[:, :k], model.model.U[:, :k])
    assert torch.equal(back.model.V[:, :k], model.model.V[:, :k])


def test_alsmodel_nonnegative_rank_limit(device, capsys):
    from src.als_model import ALSModel

    capsys.readouterr()
    assert ALSModel(rank=100, nonnegative=True).train(_frame()[0]) is False
    assert "rank <= 64" in capsys.readouterr().out


def test_alsmodel_nonnegative_false_is_the_default(device):
    from src.als_model import ALSModel

    frame = _frame()[0]
    a, b = ALSModel(rank=10, max_iter=2, seed=5), ALSModel(rank=10, max_iter=2, seed=5, nonnegative=False)
    assert a.train(frame) and b.train(frame)
    assert torch.equal(a.model.U, b.model.U) and torch.equal(a.model.V, b.model.V)
    assert a.nonnegative is False and (a.model.U < 0).any()
