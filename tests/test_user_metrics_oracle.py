"""CPU: the numpy oracle of hrec_user_metrics (tests/user_metrics_oracle.py)
against the reference's own numbers (tests/golden/evaluation.json, executed
from the reference) and against the per-user RecommenderEvaluator, which those
goldens pin: Precision / Recall exactly, the undefined cases, NDCG / MAE / RMSE
within rtol 2 (m + 8) 2^-52 (summation order, divisions, square root), the f64
and the np.float32 dtype rule, and np.mean's bits for the threshold.
"""
import math
import warnings

import numpy as np
import pytest

import user_metrics_oracle as um
from conftest import load_golden


def _cases():
    return load_golden("evaluation.json")["cases"]


def _dicts(c):
    return {int(i): v for i, v in c["actual"]}, {int(i): v for i, v in c["pred"]}


def _common_count(a, p):
    return len(set(a) & set(p))


def _close(got, exp, m):
    assert math.isfinite(got) and abs(got - exp) <= um.rtol(m) * abs(exp), (got, exp, m)


def test_golden_precision_recall_exact():
    for c in _cases():
        a, p = _dicts(c)
        ratings, cols, pred = um.from_dicts(a, p)
        ks = [k for k, _ in c["recall"]]
        out, _ = um.user_metrics(ratings, cols, pred, k_values=ks)
        prec = dict((k, e["ok"]) for k, e in c["precision"])
        for i, (k, e) in enumerate(c["recall"]):
            assert out[len(ks) + i] == e["ok"], (k, out, e)
            if k > 0:
                assert out[i] == prec[k], (k, out, prec)


def test_golden_ndcg_mae_rmse_and_undefined_cases():
    seen_sizes, n_undefined = set(), 0
    for c in _cases():
        a, p = _dicts(c)
        ratings, cols, pred = um.from_dicts(a, p)
        m = _common_count(a, p)
        seen_sizes.add(len(a))
        for k, e in c["ndcg"]:
            out, status = um.user_metrics(ratings, cols, pred, ndcg_k=k)
            nd = out[-3]
            if "raises" in e:
                assert e["raises"] == "ValueError" and status & um.NDCG_UNDEFINED and math.isnan(nd)
                n_undefined += 1
            else:
                assert not status & um.NDCG_UNDEFINED
                if e["ok"] == 0.0:
                    assert nd == 0.0
                else:
                    _close(nd, e["ok"], m)
        e = c["mae_rmse"]
        if "raises" in e:
            assert e["raises"] == "ValueError" and status & um.ERR_UNDEFINED
            assert math.isnan(out[-2]) and math.isnan(out[-1])
            n_undefined += 1
        else:
            assert not status & um.ERR_UNDEFINED
            for got, exp in zip(out[-2:], e["ok"]):
                if exp == 0.0:
                    assert got == 0.0
                else:
                    _close(got, exp, m)
    assert {1, 2} <= seen_sizes  # the cases with 1 and 2 rated items are among the goldens
    assert n_undefined > 0


def _random_case(rng, f32):
    n = int(rng.integers(1, 60))
    n_act = int(rng.integers(1, 40))
    items = rng.permutation(400)[: n + n_act]
    kind = int(rng.integers(0, 4))
    if kind == 0:
        ratings = rng.integers(1, 6, size=n_act).astype(np.float64)
    elif kind == 1:
        ratings = np.round(rng.uniform(1, 5, size=n_act), 1)
    elif kind == 2:
        ratings = rng.uniform(1, 5, size=n_act)
    else:  # scaled values on and around the grade edges
        ratings = np.array([1.0, 5.0] + list(1.0 + 4.0 * rng.choice([0.33, 0.66, 0.3299999, 0.6600001, 0.5],
                                                                     size=max(n_act - 2, 0))))[:n_act]
    overlap = int(rng.integers(0, min(n, n_act) + 1))
    a_items = list(items[:n_act])
    p_items = list(items[n_act - overlap: n_act - overlap + n])
    if kind == 3:
        scores = 1.0 + 4.0 * rng.choice([0.33, 0.66, 0.3299999, 0.6600001, 0.1, 0.9], size=len(p_items))
    elif int(rng.integers(0, 3)) == 0:
        scores = np.round(rng.uniform(0, 5, size=len(p_items)), 0)
    else:
        scores = rng.normal(3.0, 1.5, size=len(p_items))
    conv = np.float32 if f32 else float
    actual = {int(i): float(r) for i, r in zip(a_items, ratings)}
    pred = {int(i): conv(s) for i, s in zip(p_items, scores)}
    return actual, pred


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "float32"])
def test_random_cases_match_per_user_evaluator(f32):
    from src.evaluation import RecommenderEvaluator

    ev = RecommenderEvaluator()
    rng = np.random.default_rng(11 + int(f32))
    n_defined = n_undefined = 0
    for _ in range(400):
        a, p = _random_case(rng, f32)
        ratings, cols, pred = um.from_dicts(a, p)
        assert pred.dtype == (np.float32 if f32 else np.float64)
        m = _common_count(a, p)
        for k in (5, 10):
            out, status = um.user_metrics(ratings, cols, pred, ndcg_k=k)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    exp = float(ev.ndcg_at_k(a, p, k))
            except ValueError:
                assert status & um.NDCG_UNDEFINED and math.isnan(out[-3])
                n_undefined += 1
            else:
                assert not status & um.NDCG_UNDEFINED
                n_defined += 1
                if exp == 0.0:
                    assert out[-3] == 0.0
                else:
                    _close(out[-3], exp, m)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                exp = [float(x) for x in ev.mae_rmse(a, p)]
        except ValueError:
            assert status & um.ERR_UNDEFINED and math.isnan(out[-2]) and math.isnan(out[-1])
            n_undefined += 1
        else:
            assert not status & um.ERR_UNDEFINED
            for got, e in zip(out[-2:], exp):
                if e == 0.0:
                    assert got == 0.0
                else:
                    _close(got, e, m)
        assert bool(status & um.NO_COMMON) == (m == 0)
    assert n_defined > 300 and n_undefined > 10


def test_grades_match_digitize_on_the_edges():
    x = np.array([0.0, 0.33, np.nextafter(0.33, 0), 0.66, np.nextafter(0.66, 0), 1.0, np.nan, -1.0, 2.0])
    assert np.array_equal(um._grades(x), np.digitize(x, [0.33, 0.66]))


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 127, 128, 129, 136, 300])
def test_threshold_bits_equal_np_mean(n):
    rng = np.random.default_rng(n)
    for ratings in (np.round(rng.uniform(1, 5, size=n), 1), rng.uniform(1, 5, size=n), rng.normal(size=n) * 1e3):
        got = um.threshold(ratings)
        exp = np.mean(list(ratings))
        assert np.float64(got).tobytes() == np.float64(exp).tobytes(), (n, got, exp)


def test_band_edge_ratings():
    # mean(4.0, 4.2) = 4.1 (to its bits); both items sit on the band's edges as the reference computes them
    a = {1: 4.0, 2: 4.2}
    thr = np.mean(list(a.values()))
    exp = [thr - 0.1 <= r <= thr + 0.1 for r in a.values()]
    ratings, cols, pred = um.from_dicts(a, {1: 1.0, 2: 2.0, 3: 3.0})
    out, status = um.user_metrics(ratings, cols, pred, k_values=(3,))
    assert out[0] == sum(exp) / 3 and out[1] == (1.0 if any(exp) else 0.0)
    assert bool(status & um.NO_RELEVANT) == (not any(exp))
