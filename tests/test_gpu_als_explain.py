"""GPU: hrec_als_explain against the numpy oracle (tests/explain_oracle.py).

Every generated call of explain_oracle.CALLS (ranks (10, 16) .. (64, 64);
history lengths 1 .. 200 around the 4-rating step, the 32-rating chunk and the
64-entry window; list_n 1, 16, 17, 33 around the group of 16 entries, ragged;
top_m 1, 5, 32; 300 rows; shared segments, no history, bad entries, an implicit
row without a rating > 0) is run twice (equal bits) and compared with the
longdouble oracle:
  values: per call, the oracle's own f64 path is measured against its
    longdouble path, err = max |c64 - cld| over the call's rows; the kernel
    gets 8 x err, plus 2^-50 sum_j |c_ij| as an absolute floor (both are
    backward-stable f64 solves of the same system, differing in summation
    order and in the reciprocal-plus-Newton pivots: a small constant factor
    and no more). The statistic is taken over the call, not per row: a row
    may hold a single contribution, whose f64 error is one draw and can fall
    an order of magnitude below u cond(A) |c| (measured: rows300-exp, row 159,
    one history entry, cond(A) = 83, c = 2.06: oracle error 2.0e-15, kernel
    error 3.0e-14, u cond |c| = 1.9e-14). A total is a sum over the row's
    entries, so its bound uses the oracle's summed error, max_i sum_j
    |c64 - cld|, in place of err;
  positions and lengths: exactly (tests/test_explain_oracle.py asserts the gap
    condition for every call, so none is left out); ties by construction
    separately.
Both sides take the SAME YtY: the library's hrec_als_gramian, read back."""
import numpy as np
import pytest

import explain_oracle as eo

pytestmark = pytest.mark.gpu


def run(call, want_row=True, yty=None):
    """One kernel call on a Call's host arrays: numpy (total, pos, val, len, row or None, yty)."""
    import torch
    from src import _hrec

    dev = "cuda"
    Y = torch.as_tensor(call.Y, device=dev)
    if call.implicit and yty is None:
        yty = _hrec.als_gramian(Y, call.k)
    elif yty is not None:
        yty = torch.as_tensor(np.ascontiguousarray(yty), device=dev)
    hist = tuple(torch.as_tensor(a, device=dev) for a in (call.hist_rows, call.indptr, call.cols, call.vals))
    ll = None if call.list_len is None else torch.as_tensor(call.list_len, device=dev)
    out = _hrec.als_explain(torch.as_tensor(call.lists, device=dev), hist, Y, call.k, call.reg, call.top_m,
                            implicit=bool(call.implicit), alpha=call.alpha, yty=yty, list_len=ll, want_row=want_row)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out) + (None if yty is None else yty.cpu().numpy(),)


def check(call, got):
    """Compare one call with the oracle; returns the largest (error - floor) / (8 x oracle error) seen."""
    total, pos, val, ln, rowx, yty = got
    worst = 0.0
    cache = {}
    err_max = err_sum = eo.LD(0)
    for r in range(len(call.hist_rows)):  # the oracle's rows, and its own f64 error over the call
        key = (int(call.hist_rows[r]), call.row_entries(r).tobytes())
        if key in cache:
            continue
        rld, r64 = cache[key] = (call.oracle_row(r, eo.LD, yty), call.oracle_row(r, eo.F64, yty))
        valid = ~np.isnan(rld.c).all(axis=1)
        if rld.ok and valid.any():
            assert r64.ok
            err = np.abs(r64.c.astype(eo.LD) - rld.c)[valid][:, rld.elig]
            err_max, err_sum = max(err_max, err.max()), max(err_sum, err.sum(axis=1).max())
    for r in range(len(call.hist_rows)):
        rld, r64 = cache[(int(call.hist_rows[r]), call.row_entries(r).tobytes())]
        wpos, wval, wlen = eo.top_lists(rld, call.top_m)
        assert np.array_equal(ln[r], wlen), (call.name, r)
        assert np.array_equal(pos[r], wpos), (call.name, r)
        dead = np.arange(call.top_m)[None, :] >= wlen[:, None]
        assert np.isnan(val[r][dead]).all() and np.isfinite(val[r][~dead]).all()
        if rowx is not None:
            assert (rowx[r, call.k:] == 0).all()
            if rld.x is None:
                assert (rowx[r] == 0).all()  # what the half-sweep leaves such a row at
            else:
                x = rld.x.astype(np.float64)
                assert (np.abs(rowx[r, :call.k] - x) <= 2.0 ** -23 * np.abs(x) + 2.0 ** -40 * np.abs(x).max()).all()
        if not rld.ok:
            assert np.isnan(total[r]).all() and (ln[r] == 0).all()
            continue
        valid = ~np.isnan(rld.c).all(axis=1)
        assert np.isnan(total[r][~valid]).all() and (ln[r][~valid] == 0).all()
        floor = eo.FLOOR * np.abs(rld.c[:, rld.elig]).sum(axis=1)  # per entry
        for i in np.nonzero(valid)[0]:
            dv = np.abs(val[r, i, :wlen[i]].astype(eo.LD) - wval[i, :wlen[i]]).max()
            dt = abs(eo.LD(total[r, i]) - rld.total()[i])
            for d, ref in ((dv, err_max), (dt, err_sum)):
                if ref > 0:
                    worst = max(worst, float(max(d - floor[i], 0) / (8 * ref)))
            assert dv <= 8 * err_max + floor[i], (call.name, r, i, float(dv), float(8 * err_max + floor[i]))
            assert dt <= 8 * err_sum + floor[i], (call.name, r, i, float(dt), float(8 * err_sum + floor[i]))
    return worst


@pytest.mark.parametrize("call", eo.CALLS, ids=[c.name for c in eo.CALLS])
def test_against_the_longdouble_oracle(device, call):
    got = run(call)
    again = run(call, yty=got[5])
    for a, b in zip(got[:5], again[:5]):
        assert a.tobytes() == b.tobytes()  # the same call twice: equal bits
    worst = check(call, got)
    print("%s: largest (error - floor) / (8 x oracle f64 error) = %.3f" % (call.name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["len-k50-kp64-exp", "len-k20-kp32-imp", "rows300-imp"])
def test_without_out_row_the_other_outputs_keep_their_bits(device, name):
    call = next(c for c in eo.CALLS if c.name == name)
    full = run(call)
    bare = run(call, want_row=False, yty=full[5])
    assert bare[4] is None
    for a, b in zip(full[:4], bare[:4]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["len-k10-kp16-exp", "len-k20-kp32-exp", "len-k64-kp64-exp", "len-k16-kp16-imp",
                                  "len-k50-kp64-imp"])
def test_out_row_has_the_half_sweeps_bits(device, name):
    import torch
    from src import _hrec

    call = next(c for c in eo.CALLS if c.name == name)
    got = run(call)
    Y = torch.as_tensor(call.Y, device="cuda")
    csr = tuple(torch.as_tensor(a, device="cuda") for a in (call.indptr, call.cols, call.vals))
    dst = torch.empty((len(call.indptr) - 1, call.kp), dtype=torch.float32, device="cuda")
    if call.implicit:
        _hrec.als_half_sweep_implicit(*csr, Y, call.k, call.reg, call.alpha, torch.as_tensor(got[5], device="cuda"), dst)
    else:
        _hrec.als_half_sweep(*csr, Y, call.k, call.reg, dst)
    torch.cuda.synchronize()
    assert got[4].tobytes() == dst.cpu().numpy()[call.hist_rows].tobytes()


def _tie_call(lengths_cols_vals, k=10, kp=16, top_m=8):
    call = eo.Call("ties", k, kp, 0, 0.0, 77, (len(lengths_cols_vals[0]),), (0, 0), 18, top_m, ragged=False)
    call.cols = np.asarray(lengths_cols_vals[0], np.int32)
    call.vals = np.asarray(lengths_cols_vals[1], np.float32)
    return call


def test_equal_contributions_keep_the_earlier_position_first(device):
    # the same item with the same rating twice: two bit-equal contributions
    call = _tie_call(([5, 9, 5, 30, 9], [2.0, 3.0, 2.0, 1.0, 3.0]))
    total, pos, val, ln, _, _ = run(call)
    assert (ln == 5).all()
    for r in range(2):
        for i in range(call.list_n):
            p, v = list(pos[r, i, :5]), val[r, i, :5]
            assert sorted(p) == [0, 1, 2, 3, 4] and (np.diff(v) <= 0).all()
            assert p.index(0) + 1 == p.index(2) and p.index(1) + 1 == p.index(4)
            assert v[p.index(0)] == v[p.index(2)] and v[p.index(1)] == v[p.index(4)]
    check(call, (total, pos, val, ln, None, None))  # the oracle has the same ties and the same rule
    # a tie across two 64-entry windows, and one inside the second window
    rng = np.random.default_rng(5)
    cols = rng.permutation(eo.N_ITEMS)[:150]
    vals = rng.uniform(0.5, 5.0, 150)
    cols[100], vals[100] = cols[3], vals[3]
    cols[140], vals[140] = cols[70], vals[70]
    call = _tie_call((cols, vals), k=20, kp=32, top_m=32)
    call.top_m = 32
    # make the tied entries large so that they are among the top 32: the contribution grows with the rating
    for j in (3, 100, 70, 140):
        call.vals[j] = np.float32(40.0 if j in (3, 100) else -40.0)
    got = run(call)
    check(call, got[:4] + (None, None))
    rld = call.oracle_row(0, eo.LD)
    wpos, _, _ = eo.top_lists(rld, 32)
    seen = 0
    for i in range(call.list_n):
        p = list(wpos[i])
        for a, b in ((3, 100), (70, 140)):
            if a in p and b in p:
                assert p.index(a) + 1 == p.index(b)
                seen += 1
    assert seen >= call.list_n  # the construction does put tied pairs into the lists


def test_unusable_factorisation_and_empty_shapes(device):
    import torch
    from src import _hrec

    # a zero matrix: implicit, alpha 0, reg_param 0 and YtY = 0
    call = next(c for c in eo.CALLS if c.name == "alpha0")
    saved = call.reg
    try:
        call.reg = 0.0
        total, pos, val, ln, rowx, _ = run(call, yty=np.zeros((call.kp, call.kp)))
    finally:
        call.reg = saved
    assert np.isnan(total).all() and (ln == 0).all() and (pos == -1).all() and np.isnan(val).all()
    # n_rows == 0 and list_n == 0: HREC_OK, nothing to write
    Y = torch.as_tensor(call.Y, device="cuda")
    hist = tuple(torch.as_tensor(a, device="cuda") for a in (call.hist_rows[:0], call.indptr, call.cols, call.vals))
    out = _hrec.als_explain(torch.zeros((0, 4), dtype=torch.int64, device="cuda"), hist, Y, call.k, 0.1, 5)
    assert out[0].shape == (0, 4) and out[1].shape == (0, 4, 5)
    hist = tuple(torch.as_tensor(a, device="cuda") for a in (call.hist_rows, call.indptr, call.cols, call.vals))
    out = _hrec.als_explain(torch.zeros((2, 0), dtype=torch.int64, device="cuda"), hist, Y, call.k, 0.1, 5)
    torch.cuda.synchronize()
    assert out[0].shape == (2, 0) and out[3].shape == (2, 0)
