"""CPU: tests/fold_in_oracle.py, the numpy restatement of
hrec_tt_fold_in_users the GPU tests compare the kernel with, against
torch.autograd and its own specification; and its f32-vs-f64 gap, which sets
the GPU tests' tolerance."""
import numpy as np
import pytest
import torch

import fold_in_oracle as fo

GAP_GRID = [(d, hist, steps, lr) for d in (7, 50, 64, 256) for hist in (1, 5, 40)
            for steps, lr in ((50, 1e-3), (200, 1e-2), (100, 5e-2))]


@pytest.mark.parametrize("d", [7, 50])
def test_gradient_matches_autograd_in_f64(d):
    c = fo.random_case(d, [9], seed=3)
    vecs = c["item_vec"][c["item_rows"]].astype(np.float64)
    y = c["ratings"].astype(np.float64)
    gamma, beta = c["gamma"].astype(np.float64), c["beta"].astype(np.float64)
    loss, g, u = fo.loss_and_gradient(c["emb"][0].astype(np.float64), gamma, beta, vecs, y, np.float64)
    e = torch.tensor(c["emb"][0].astype(np.float64), requires_grad=True)
    mean = e.mean()
    var = ((e - mean) ** 2).mean()  # biased
    ut = (e - mean) / torch.sqrt(var + 1e-3) * torch.tensor(gamma) + torch.tensor(beta)
    lt = ((torch.tensor(vecs) @ ut - torch.tensor(y)) ** 2).mean()
    lt.backward()
    ref = e.grad.numpy()
    assert abs(loss - lt.item()) <= 1e-12 * abs(lt.item())
    np.testing.assert_allclose(u, ut.detach().numpy(), rtol=1e-12, atol=0)
    assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max()


def test_step_sizes_are_the_train_steps():
    from src.tt_engine import AdamConfig

    for lr in (1e-3, 1e-2):
        cfg = AdamConfig(lr)
        got = fo.step_sizes(lr, 30)
        assert got.dtype == np.float32
        assert [x.tobytes() for x in got] == [cfg.coefficients(t)["sparse_lr"].tobytes() for t in range(30)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_steps_and_no_history(dtype):
    c = fo.random_case(7, [3, 0, 2], seed=1)
    c["item_rows"][3:5] = (-1, 40)  # the third row's entries: below and past the item vectors
    before = c["emb"].astype(dtype)
    # no step: rows as they were, the same loss twice
    emb, u, loss = fo.fold_in(c["emb"], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"],
                              c["ratings"], 0, np.zeros(0, np.float32), dtype)
    assert emb.dtype == dtype and emb.tobytes() == before.tobytes()
    assert loss[0, 0] == loss[0, 1] and np.isfinite(loss[0]).all()
    assert np.isnan(loss[1:]).all()
    # steps: a row without a usable entry keeps its bits and has NaN losses
    emb, u, loss = fo.fold_in(c["emb"], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"],
                              c["ratings"], 5, fo.step_sizes(1e-2, 5), dtype)
    assert emb[1:].tobytes() == before[1:].tobytes() and np.isnan(loss[1:]).all()
    assert emb[0].tobytes() != before[0].tobytes() and loss[0, 1] < loss[0, 0]
    np.testing.assert_array_equal(u[1], fo.layer_norm(before[1], c["gamma"].astype(dtype), c["beta"].astype(dtype),
                                                      dtype)[0])


def test_duplicates_are_separate_terms():
    c = fo.random_case(7, [2], seed=2)
    c["item_rows"][:] = 5
    _, _, loss = fo.fold_in(c["emb"], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"], c["ratings"],
                            0, np.zeros(0, np.float32))
    u = fo.layer_norm(c["emb"][0].astype(np.float64), c["gamma"].astype(np.float64), c["beta"].astype(np.float64),
                      np.float64)[0]
    s = c["item_vec"][5].astype(np.float64) @ u
    assert loss[0, 0] == pytest.approx(((s - c["ratings"].astype(np.float64)) ** 2).mean(), rel=1e-14)


def test_f32_gap_of_the_restatement():
    """The distance between the f32 and the f64 restatement on the final user
    vector u = LN(e), values O(1): what f32 rounding alone moves the result
    by. The GPU tests allow the kernel 8 x its case's own gap (floor 2e-6).
    Printed per case; the bound asserted here only keeps that allowance (8 x
    1.25e-4 = 1e-3) under the smallest effect a wrong step has, one step of
    size lr >= 1e-3 on an O(0.05) row entering u through 1/std ~ 30."""
    worst = 0.0
    for d, hist, steps, lr in GAP_GRID:
        c = fo.random_case(d, [hist], seed=7)
        args = (c["emb"], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"], c["ratings"], steps,
                fo.step_sizes(lr, steps))
        _, u32, l32 = fo.fold_in(*args, np.float32)
        _, u64, l64 = fo.fold_in(*args, np.float64)
        gap = float(np.abs(u32.astype(np.float64) - u64).max())
        print(f"d {d:3d} history {hist:2d} steps {steps:3d} lr {lr:g}: |u32 - u64| {gap:.3g}, "
              f"loss {l64[0, 0]:.4g} -> {l64[0, 1]:.4g} (f32 {l32[0, 1]:.4g})")
        worst = max(worst, gap)
    print(f"largest gap {worst:.3g}")
    assert worst < 1.25e-4
