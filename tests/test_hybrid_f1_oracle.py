"""CPU: tests/hybrid_f1_oracle.py against src.als_model.compute_f1_score (the
reference's, pinned by tests/golden/f1.json): the same Python float for a
dict's items taken as the candidate frame in dict order."""
import numpy as np
from conftest import load_golden
from hybrid_f1_oracle import dict_f1, f1_value, model_f1, selection


def _same(got, exp):
    assert float(got) == float(exp) and np.float64(got).view(np.int64) == np.float64(exp).view(np.int64), (got, exp)


def test_golden_cases():
    from src.als_model import compute_f1_score

    seen = 0
    for rec in load_golden("f1.json")["cases"]:
        if rec["k"] <= 0:
            continue
        actual = {int(i): s for i, s in rec["actual"]}
        pred = {int(i): s for i, s in rec["pred"]}
        exp = compute_f1_score(actual, pred, k=rec["k"])
        assert float(exp) == rec["als"] == rec["tt"]
        _same(dict_f1(actual, pred, rec["k"]), exp)
        _same(dict_f1(actual, {i: np.float32(s) for i, s in pred.items()}, rec["k"], as_f32=True),
              compute_f1_score(actual, {i: np.float32(s) for i, s in pred.items()}, k=rec["k"]))
        seen += 1
    assert seen >= 3


def test_random_dicts():
    """Tied scores, labels outside the candidates, n < k, an empty
    intersection; f64 (ALS side) and f32 (two-tower side) scores."""
    from src.als_model import compute_f1_score

    rng = np.random.default_rng(5)
    kinds = set()
    for trial in range(400):
        n = int(rng.integers(1, 40))
        k = int(rng.choice([1, 3, 10, 25, 64]))
        ids = rng.permutation(200)[:n].tolist()
        levels = int(rng.choice([2, 4, 1000]))
        for as_f32 in (False, True):
            raw = rng.integers(0, levels, n) / 3.0
            pred = {i: (np.float32(s) if as_f32 else float(s)) for i, s in zip(ids, raw)}
            inside = rng.choice(ids, int(rng.integers(0, min(n, 6) + 1)), replace=False).tolist()
            outside = (300 + rng.permutation(50)[: int(rng.integers(0, 4))]).tolist()
            if trial % 7 == 0:  # nothing of the user's among the model's best
                order = sorted(pred.items(), key=lambda x: x[1], reverse=True)
                inside = [i for i, _ in order[k:]][:3]
            actual = {int(i): 1.0 for i in inside + outside}
            if not actual:
                continue
            exp = compute_f1_score(actual, pred, k=k)
            _same(dict_f1(actual, pred, k, as_f32=as_f32), exp)
            kinds |= {("n<k", n < k), ("outside", bool(outside)), ("zero", exp == 0), ("tied", levels <= 4)}
    assert kinds == {(a, b) for a in ("n<k", "outside", "zero", "tied") for b in (True, False)}


def test_selection_order():
    nan = float("nan")
    assert selection([1.0, nan, 3.0, 3.0, -0.0, 0.0, nan], 10).tolist() == [2, 3, 0, 4, 5, 1, 6]
    assert selection(np.array([2, 2, 2], np.float32), 2).tolist() == [0, 1]
    assert f1_value(0, 10, 3) == 0 and f1_value(2, 10, 4) == 2 * (0.2 * 0.5) / (0.2 + 0.5)


def test_model_f1_rows():
    """label_rows = -1, label_total = 0, labels all outside, total above the
    candidate labels, default_wins."""
    als = np.array([[3, 2, 1, 0]] * 5, np.float32)
    tt = np.array([[0, 1, 2, 3]] * 5, np.float32)
    rows = np.array([0, -1, 1, 2, 3], np.int64)
    indptr = np.array([0, 2, 2, 2, 3], np.int64)
    cols = np.array([0, 1, 3], np.int32)
    total = np.array([2, 0, 4, 5], np.int32)
    for dw in (0, 1):
        f1, wins, top = model_f1(als, tt, 2, (rows, indptr, cols, total), default_wins=dw)
        assert top[0].tolist() == [[0, 1], [3, 2]]
        assert f1[0].tolist() == [1.0, 0.0] and wins[0] == 1
        assert np.isnan(f1[1]).all() and wins[1] == dw          # no label row
        assert np.isnan(f1[2]).all() and wins[2] == dw          # label_total 0
        assert f1[3].tolist() == [0.0, 0.0] and wins[3] == 0    # labels, none a candidate
        assert f1[4].tolist() == [0.0, f1_value(1, 2, 5)] and wins[4] == 0
