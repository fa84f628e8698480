"""GPU: hrec_tt_fold_in_users against tests/fold_in_oracle.py in f64.

Grid: d in {7, 50, 64, 200, 256} (1 to 4 registers per lane, full and partial
last 64-column group, the three alignment classes) x steps in {0, 1, 25} x
launches of 1 row and of 5 rows (not a multiple of the 4 waves of a block, two
blocks). The 5-row launch holds histories of 0, 1, 2, 65 and 130 entries (an
empty row, less than / more than one 64-entry walk, a group of four that is
not full); the 2-entry history repeats one item, the 130-entry one holds an
item row of -1 and one of n_items. emb has two rows beyond n_rows.

Tolerance, per launch (the oracle's own error sets it, never the kernel's
output): the final u = LN(e) is compared absolutely, values O(1), within
max(8 x max |u_f32 - u_f64| of the restatement on that launch, 2e-6); the
kernel's butterfly sums and fused multiply-adds are a third rounding sequence
beside the two restatements, hence the factor 8, and 2e-6 is ~30 ulp of an
O(1) f32. The losses follow the same rule with the gap taken between the
restatements' losses: max(8 x max |loss_f32 - loss_f64| on that launch, 2e-6),
absolutely, with no allowance for the losses' size (they reach the hundreds)."""
import functools

import numpy as np
import pytest
import torch

import fold_in_oracle as fo

pytestmark = pytest.mark.gpu

DS = [7, 50, 64, 200, 256]
STEPS = [0, 1, 25]
LR = 1e-2
N_ITEMS, EXTRA = 40, 2


def _hrec():
    from src import _hrec

    return _hrec


@functools.lru_cache(maxsize=None)
def _case(d, rows):
    lens = [0, 1, 2, 65, 130] if rows == 5 else [65]
    c = fo.random_case(d, lens, n_items=N_ITEMS, seed=11, extra_rows=EXTRA)
    ip = c["indptr"]
    if rows == 5:
        c["item_rows"][ip[2] + 1] = c["item_rows"][ip[2]]  # the same item twice: two terms
        c["item_rows"][ip[4] + 3] = -1
        c["item_rows"][ip[4] + 70] = N_ITEMS
    else:
        c["item_rows"][1] = c["item_rows"][0]
        c["item_rows"][5], c["item_rows"][64] = -1, N_ITEMS
    return c


@functools.lru_cache(maxsize=None)
def _reference(d, rows, steps):
    """(f64 u, f64 loss, u tolerance, loss tolerance, the two gaps) of a case; computed once."""
    c = _case(d, rows)
    args = (c["emb"][: len(c["indptr"]) - 1], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"],
            c["ratings"], steps, fo.step_sizes(LR, steps))
    _, u32, l32 = fo.fold_in(*args, np.float32)
    _, u64, l64 = fo.fold_in(*args, np.float64)
    gap_u = float(np.abs(u32.astype(np.float64) - u64).max())
    gap_l = float(np.nanmax(np.abs(l32.astype(np.float64) - l64)))
    return u64, l64, max(8 * gap_u, 2e-6), max(8 * gap_l, 2e-6), gap_u, gap_l


def _run(device, d, rows, steps):
    h, c = _hrec(), _case(d, rows)
    t = {k: torch.as_tensor(v, device=device) for k, v in c.items()}
    emb = t["emb"].clone()
    loss = h.tt_fold_in_users(emb, t["gamma"], t["beta"], t["item_vec"], t["indptr"], t["item_rows"], t["ratings"],
                              torch.as_tensor(fo.step_sizes(LR, steps), device=device), fo.BETA_1,
                              np.float32(1) - fo.BETA_1, fo.BETA_2, np.float32(1) - fo.BETA_2, fo.EPSILON)
    torch.cuda.synchronize()
    return emb.cpu().numpy(), loss.cpu().numpy()


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("d", DS)
def test_fitted_rows_and_losses_match_the_f64_restatement(device, d, steps, rows):
    c = _case(d, rows)
    u64, l64, tol_u, tol_l, gap_u, gap_l = _reference(d, rows, steps)
    emb, loss = _run(device, d, rows, steps)
    g64, b64 = c["gamma"].astype(np.float64), c["beta"].astype(np.float64)
    u = np.stack([fo.layer_norm(e.astype(np.float64), g64, b64, np.float64)[0] for e in emb[:rows]])
    err_u = float(np.abs(u - u64).max())
    has = ~np.isnan(l64[:, 0])
    err_l = float(np.abs(loss[has].astype(np.float64) - l64[has]).max())
    print(f"d {d} steps {steps} rows {rows}: |u - u64| {err_u:.3g} (restatement gap {gap_u:.3g}, allowed {tol_u:.3g}); "
          f"|loss - loss64| {err_l:.3g} (gap {gap_l:.3g}, allowed {tol_l:.3g}); "
          f"RATIO of 8 used: u {8 * err_u / tol_u:.2f} loss {8 * err_l / tol_l:.2f}")
    assert err_u <= tol_u
    assert err_l <= tol_l
    assert np.isnan(loss[~has]).all() and np.isfinite(loss[has]).all()
    # a row without a usable entry, and every row when there is no step, keeps its bits
    same = ~has if steps else np.ones(rows, bool)
    assert emb[:rows][same].tobytes() == c["emb"][:rows][same].tobytes()
    if steps:
        assert not np.array_equal(emb[:rows][has], c["emb"][:rows][has])
    else:
        assert np.array_equal(loss[has, 0], loss[has, 1])
    # rows of emb beyond n_rows are not touched
    assert emb[rows:].tobytes() == c["emb"][rows:].tobytes()


@pytest.mark.parametrize("d", DS)
def test_two_calls_give_equal_bits(device, d):
    a, b = _run(device, d, 5, 25), _run(device, d, 5, 25)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()


def test_loss_falls_with_more_steps(device):
    """200 steps at 1e-2 on ratings in [1, 5]: every row with a history ends
    below where it started (the f64 restatement does, asserted first)."""
    c = _case(50, 5)
    lr = fo.step_sizes(LR, 200)
    _, _, l64 = fo.fold_in(c["emb"][:5], c["gamma"], c["beta"], c["item_vec"], c["indptr"], c["item_rows"],
                           c["ratings"], 200, lr)
    has = ~np.isnan(l64[:, 0])
    assert (l64[has, 1] < l64[has, 0]).all()
    h = _hrec()
    t = {k: torch.as_tensor(v, device=device) for k, v in c.items()}
    loss = h.tt_fold_in_users(t["emb"].clone(), t["gamma"], t["beta"], t["item_vec"], t["indptr"], t["item_rows"],
                              t["ratings"], torch.as_tensor(lr, device=device), fo.BETA_1, np.float32(1) - fo.BETA_1,
                              fo.BETA_2, np.float32(1) - fo.BETA_2, fo.EPSILON).cpu().numpy()
    assert (loss[has, 1] < loss[has, 0]).all()


def test_no_rows_and_no_loss_output(device):
    h, c = _hrec(), _case(7, 5)
    t = {k: torch.as_tensor(v, device=device) for k, v in c.items()}
    emb = t["emb"].clone()
    lr = torch.as_tensor(fo.step_sizes(LR, 3), device=device)
    adam = (fo.BETA_1, np.float32(1) - fo.BETA_1, fo.BETA_2, np.float32(1) - fo.BETA_2, fo.EPSILON)
    out = h.tt_fold_in_users(emb, t["gamma"], t["beta"], t["item_vec"], t["indptr"][:1], t["item_rows"][:0],
                             t["ratings"][:0], lr, *adam)
    assert tuple(out.shape) == (0, 2) and torch.equal(emb, t["emb"])
    assert h.tt_fold_in_users(emb, t["gamma"], t["beta"], t["item_vec"], t["indptr"], t["item_rows"], t["ratings"],
                              lr, *adam, want_loss=False) is None
    ref, _ = _run(device, 7, 5, 3)
    assert emb.cpu().numpy().tobytes() == ref.tobytes()
