"""GPU: hrec_user_metrics through _hrec.user_metrics against the numpy oracle of
its contract (tests/user_metrics_oracle.py, itself pinned to the reference's
goldens on the CPU). Precision, Recall and status exactly; NDCG, MAE and RMSE
within rtol 2 (m + 8) 2^-52, m the row's common items.
"""
import math

import numpy as np
import pytest
import torch

import user_metrics_oracle as um
from conftest import load_golden

pytestmark = pytest.mark.gpu

KS = (5, 10, 15, 20)
RATED = (0, 1, 2, 7, 8, 9, 64, 65, 128, 129, 300)


def _csr(users, dev):
    """Device CSR of [(ratings in frame order, cols)] (None: a row without ratings)."""
    rows, indptr, cols, ratings, frame = [], [0], [], [], []
    for u in users:
        if u is None:
            rows.append(-1)
            continue
        r, c = np.asarray(u[0], np.float64), np.asarray(u[1], np.int64)
        order = np.argsort(c, kind="stable")
        rows.append(len(indptr) - 1)
        cols += c[order].tolist()
        ratings += r[order].tolist()
        frame += r.tolist()
        indptr.append(len(cols))
    t = lambda x, d: torch.tensor(x, dtype=d, device=dev)  # noqa: E731
    return (t(rows, torch.int64), t(indptr, torch.int64), t(cols, torch.int32), t(ratings, torch.float64),
            t(frame, torch.float64))


def _ranked(scores, L):
    return np.stack([um.ranking(row)[:L] for row in scores]) if len(scores) else np.zeros((0, L), np.int64)


def _expect(users, scores, ks, ndcg_k, ranked, lens=None):
    exp, status, ms = [], [], []
    for i, u in enumerate(users):
        r, c = (np.zeros(0), np.zeros(0, np.int64)) if u is None else u
        lst = ranked[i][: (len(ranked[i]) if lens is None else lens[i])]
        v, s = um.user_metrics(r, c, scores[i], ks, ndcg_k, ranked=lst)
        exp.append(v), status.append(s), ms.append(int((np.asarray(c) >= 0).sum()))
    return np.array(exp).reshape(len(users), 2 * len(ks) + 3), np.array(status, np.int32), ms


def _compare(got, got_status, exp, exp_status, ms, nk):
    assert np.array_equal(got_status, exp_status), (got_status, exp_status)
    assert np.array_equal(got[:, : 2 * nk], exp[:, : 2 * nk])  # Precision and Recall: exact
    for i, m in enumerate(ms):
        for j in range(2 * nk, 2 * nk + 3):
            g, e = float(got[i, j]), float(exp[i, j])
            if math.isnan(e) or e == 0.0:
                assert (math.isnan(g) and math.isnan(e)) or g == e, (i, j, g, e)
            else:
                assert abs(g - e) <= um.rtol(m) * abs(e), (i, j, g, e, m)


def _run(device, users, scores, ks=KS, ndcg_k=10, source=None, ranked=None, lens=None, **kw):
    from src import _hrec

    L = min(max(ks), scores.shape[1])
    ranked = _ranked(scores, L) if ranked is None else ranked
    per_row, status, sums = _hrec.user_metrics(
        torch.as_tensor(ranked, device=device), ks, _csr(users, device), torch.as_tensor(scores, device=device),
        source=source, ndcg_k=ndcg_k,
        list_len=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=device), **kw)
    return per_row.cpu().numpy(), status.cpu().numpy(), sums.cpu().numpy(), ranked


def _check_sums(per_row, status, sums, ks):
    from src import _hrec

    names = _hrec.um_sums(ks)
    ncol = 2 * len(ks) + 3
    rated = (status & um.NO_RATINGS) == 0
    for j in range(ncol):
        ok = rated & np.isfinite(per_row[:, j])
        assert sums[ncol + j] == ok.sum(), names[ncol + j]
        np.testing.assert_allclose(sums[j], per_row[ok, j].sum(), rtol=1e-13, atol=0, err_msg=names[j])
    for b in range(um.STATUS_BITS):
        assert sums[2 * ncol + b] == ((status >> b) & 1).sum(), names[2 * ncol + b]


def _user(rng, n_rated, n, inside=None):
    """n_rated ratings; `inside` of them (default: about half, at most n) in the frame."""
    if n_rated == 0:
        return None
    inside = min(n, (n_rated + 1) // 2) if inside is None else inside
    cols = np.full(n_rated, -1, np.int64)
    cols[rng.permutation(n_rated)[:inside]] = rng.permutation(n)[:inside]
    kind = int(rng.integers(0, 3))
    ratings = (rng.integers(1, 6, n_rated).astype(np.float64) if kind == 0 else
               np.round(rng.uniform(1, 5, n_rated), 1) if kind == 1 else rng.uniform(1, 5, n_rated))
    return ratings, cols


def _scores(rng, n_rows, n, dtype):
    s = rng.normal(3.0, 1.0, (n_rows, n))
    s[:, ::3] = np.round(s[:, ::3])  # ties
    return s.astype(dtype)


def _fused(als, tt, fb, wins):
    """The oracle's fused matrix (hrec_hybrid_lists' arithmetic) and its minmax rows."""
    a = np.where(np.isnan(als), fb[None, :], als.astype(np.float64))
    amin, amax = np.nanmin(a, axis=1), np.nanmax(a, axis=1)
    tmin, tmax = np.nanmin(tt, axis=1), np.nanmax(tt, axis=1)
    ra, rt = amax - amin, tmax - tmin
    ascale = 1.0 / np.where(ra < 10 * np.finfo(np.float64).eps, 1.0, ra)
    tscale = (np.float32(1.0) / np.where(rt < 10 * np.finfo(np.float32).eps, np.float32(1.0), rt)).astype(np.float32)
    amin_ = 0.0 - amin * ascale
    tmin_ = (np.float32(0.0) - tmin * tscale).astype(np.float32)
    an = a * ascale[:, None] + amin_[:, None]
    tn = (tt * tscale[:, None]).astype(np.float32) + tmin_[:, None]
    w0 = np.where(wins != 0, 0.8, 0.2)[:, None]
    w1 = np.where(wins != 0, 0.2, 0.8)[:, None]
    fused = w0 * an + w1 * tn.astype(np.float64)
    return fused, np.stack([amin, amax, tmin.astype(np.float64), tmax.astype(np.float64)], axis=1)


def _source_inputs(rng, source, n_rows, n, device):
    """(the f64 / f32 matrix the oracle sees, the kernel's scores, extra keyword arguments)."""
    if source == "f64":
        s = _scores(rng, n_rows, n, np.float64)
        return s, s, {}
    if source == "f32":
        s = _scores(rng, n_rows, n, np.float32)
        return s, s, {}
    als = _scores(rng, n_rows, n, np.float32)
    als[rng.random((n_rows, n)) < 0.1] = np.nan
    if n_rows > 1:
        als[-1, :] = np.nan  # a cold user: the whole row is the fallback vector
    fb = rng.normal(3.0, 1.0, n)
    fb_d = torch.as_tensor(fb, device=device)
    if source == "als":
        return np.where(np.isnan(als), fb[None, :], als.astype(np.float64)), als, {"fallback": fb_d}
    tt = _scores(rng, n_rows, n, np.float32)
    wins = (np.arange(n_rows) % 2).astype(np.int32)
    fused, mm = _fused(als, tt, fb, wins)
    return fused, als, {"fallback": fb_d, "tt": torch.as_tensor(tt, device=device),
                        "minmax": torch.as_tensor(mm, device=device),
                        "row_wins": torch.as_tensor(wins, device=device)}


def test_golden_cases_as_one_batch(device):
    cases = load_golden("evaluation.json")["cases"]
    users, rows = [], []
    for c in cases:
        a = {int(i): v for i, v in c["actual"]}
        p = {int(i): v for i, v in c["pred"]}
        r, cols, pred = um.from_dicts(a, p)
        users.append((r, cols))
        rows.append(pred.astype(np.float64))
    n = max(len(r) for r in rows)
    scores = np.full((len(rows), n), np.nan)  # NaN pads rank last and are nobody's rated item
    for i, r in enumerate(rows):
        scores[i, : len(r)] = r
    for ndcg_k in (5, 10):
        got, st, sums, ranked = _run(device, users, scores, ks=(5, 10), ndcg_k=ndcg_k)
        exp, est, ms = _expect(users, scores, (5, 10), ndcg_k, ranked)
        _compare(got, st, exp, est, ms, 2)
        _check_sums(got, st, sums, (5, 10))
        for i, c in enumerate(cases):  # and the reference's numbers themselves
            prec, rec = dict(c["precision"]), dict(c["recall"])
            nd = dict(c["ndcg"])[ndcg_k]
            for j, k in enumerate((5, 10)):
                assert got[i, j] == prec[k]["ok"] and got[i, 2 + j] == rec[k]["ok"]
            assert ("raises" in nd) == bool(st[i] & um.NDCG_UNDEFINED)
            assert ("raises" in c["mae_rmse"]) == bool(st[i] & um.ERR_UNDEFINED)
            if "ok" in nd and nd["ok"] != 0.0:
                assert abs(got[i, 4] - nd["ok"]) <= um.rtol(ms[i]) * nd["ok"]
            if "ok" in c["mae_rmse"]:
                for g, e in zip(got[i, 5:], c["mae_rmse"]["ok"]):
                    assert abs(g - e) <= um.rtol(ms[i]) * abs(e)


@pytest.mark.parametrize("source", ["f64", "f32", "als", "fused"])
@pytest.mark.parametrize("n", [1, 7, 64, 65, 1000])
@pytest.mark.parametrize("n_rows", [1, 4, 5])
def test_shapes_and_sources(device, n_rows, n, source):
    rng = np.random.default_rng(1000 * n_rows + n)
    seen, s, kw = _source_inputs(rng, source, n_rows, n, device)
    users = [_user(rng, RATED[(i + n) % len(RATED)], n) for i in range(n_rows)]
    got, st, sums, ranked = _run(device, users, s, source=source, **kw)
    exp, est, ms = _expect(users, seen, KS, 10, ranked)
    _compare(got, st, exp, est, ms, len(KS))
    _check_sums(got, st, sums, KS)


@pytest.mark.parametrize("source", ["f64", "f32", "als", "fused"])
def test_every_rated_count(device, source):
    n = 1000
    rng = np.random.default_rng(5)
    seen, s, kw = _source_inputs(rng, source, len(RATED), n, device)
    users = [_user(rng, c, n, inside=min(c, n) if i % 2 else None) for i, c in enumerate(RATED)]
    got, st, sums, ranked = _run(device, users, s, source=source, **kw)
    exp, est, ms = _expect(users, seen, KS, 10, ranked)
    _compare(got, st, exp, est, ms, len(KS))
    assert st[0] & um.NO_RATINGS and not (st[1:] & um.NO_RATINGS).any()
    _check_sums(got, st, sums, KS)
    if source == "fused":  # the recomputed fused scores carry the oracle matrix's bits
        got64, st64, sums64, _ = _run(device, users, seen, source="f64", ranked=ranked)
        assert np.array_equal(got, got64, equal_nan=True) and np.array_equal(st, st64)
        assert sums.tobytes() == sums64.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_edge_rows(device, dtype):
    n = 64
    rng = np.random.default_rng(9)
    s = _scores(rng, 10, n, dtype)
    edges = np.array([0.33, 0.66, np.nextafter(0.33, 0), np.nextafter(0.66, 0), np.nextafter(0.33, 1),
                      np.nextafter(0.66, 1), 0.0, 1.0])
    users = [
        (rng.uniform(1, 5, 12), np.full(12, -1, np.int64)),              # 0: every rated item outside the frame
        (np.array([4.0, 4.2]), np.array([3, 40])),                        # 1: both on the band's edges
        (np.full(9, 3.0), np.arange(9) * 5),                              # 2: constant ratings
        (rng.uniform(1, 5, 6), np.array([1, 2, 3, 4, 5, 6])),             # 3: constant predictions (below)
        (rng.uniform(1, 5, 6), np.array([10, 11, 12, 13, 14, 15])),       # 4: a NaN prediction (below)
        (1.0 + 4.0 * edges, np.arange(8) * 2),                            # 5: scaled ratings around 0.33 / 0.66
        (np.array([1.0, 5.0, 2.0, 3.0, 4.0, 2.5, 3.5, 4.5]), np.arange(8) + 20),  # 6: scaled predictions (below)
        (np.array([2.0, 3.0, 5.0]), np.array([-1, 7, -1])),               # 7: one common item
        None,                                                             # 8: no ratings
        (rng.uniform(1, 5, 30), np.concatenate([np.full(10, -1), rng.permutation(n)[:20]])),  # 9: ordinary
    ]
    s[3, 1:7] = 2.5
    s[4, 12] = np.nan
    s[6, 20:28] = (1.0 + 4.0 * edges[rng.permutation(8)]).astype(dtype)
    got, st, sums, ranked = _run(device, users, s)
    exp, est, ms = _expect(users, s, KS, 10, ranked)
    _compare(got, st, exp, est, ms, len(KS))
    _check_sums(got, st, sums, KS)
    assert st[0] & um.NO_COMMON and got[0, -3:].tolist() == [0.0, 0.0, 0.0]
    # the band of {4.0, 4.2}: mean 4.1, 4.1 - 0.1 = 3.9999999999999996 <= 4.0 but 4.1 + 0.1 = 4.199999999999999 < 4.2,
    # so the item at column 3 is the one relevant item
    assert not st[1] & um.NO_RELEVANT
    for i, k in enumerate(KS):
        hit = 1.0 if 3 in ranked[1][:k].tolist() else 0.0
        assert got[1, i] == hit / k and got[1, len(KS) + i] == hit
    for i in (2, 3, 4, 7):
        assert st[i] & um.ERR_UNDEFINED and math.isnan(got[i, -1])
    assert st[7] & um.NDCG_UNDEFINED and not st[2] & um.NDCG_UNDEFINED and got[2, -3] == 0.0
    assert st[8] == um.NO_RATINGS | um.NO_COMMON | um.NO_RELEVANT and not got[8].any()
    assert st[9] == 0


def test_list_shorter_than_k_and_strided_lists(device):
    from src import _hrec

    n, n_rows = 200, 6
    rng = np.random.default_rng(3)
    s = _scores(rng, n_rows, n, np.float64)
    users = [_user(rng, 40, n, inside=40) for _ in range(n_rows)]
    lens = [0, 3, 5, 12, 20, 20]
    got, st, _, ranked = _run(device, users, s, lens=lens)
    exp, est, ms = _expect(users, s, KS, 10, ranked, lens)
    _compare(got, st, exp, est, ms, len(KS))
    assert not got[0, :8].any()
    # a model's half of an out_top-shaped [n_rows][2][kk] buffer: a view with row stride 2 * kk
    both = torch.full((n_rows, 2, 20), -7, dtype=torch.int64, device=device)
    both[:, 1, :] = torch.as_tensor(ranked, device=device)
    per_row, status, _ = _hrec.user_metrics(both[:, 1, :], KS, _csr(users, device), torch.as_tensor(s, device=device))
    full, est, ms = _expect(users, s, KS, 10, ranked)
    _compare(per_row.cpu().numpy(), status.cpu().numpy(), full, est, ms, len(KS))


def test_equal_inputs_give_equal_sums_bits(device):
    n, n_rows = 300, 1001  # more than one partial per reduction lane
    rng = np.random.default_rng(4)
    s = _scores(rng, n_rows, n, np.float32)
    users = [_user(rng, int(rng.integers(0, 12)), n) for _ in range(n_rows)]
    ranked = _ranked(s, 20)
    a = _run(device, users, s, ranked=ranked)
    b = _run(device, users, s, ranked=ranked)
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()
    _check_sums(a[0], a[1], a[2], KS)
    exp, est, ms = _expect(users[:64], s[:64], KS, 10, ranked[:64])
    _compare(a[0][:64], a[1][:64], exp, est, ms, len(KS))


def test_no_actual_csr_and_k_bounds(device):
    from src import _hrec

    s = torch.zeros((3, 10), dtype=torch.float64, device=device)
    ranked = torch.arange(10, device=device).repeat(3, 1)
    per_row, status, sums = _hrec.user_metrics(ranked, (1, 1024), None, s)
    assert not per_row.cpu().numpy().any()
    assert (status.cpu().numpy() == um.NO_RATINGS | um.NO_COMMON | um.NO_RELEVANT).all()
    assert sums.cpu().numpy()[-1] == 3
    for ks in ((0,), (1025,), tuple(range(1, 10))):
        with pytest.raises(_hrec.HrecError):
            _hrec.user_metrics(ranked, ks, None, s)
