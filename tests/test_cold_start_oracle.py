"""CPU: the sklearn oracle of the ALS cold-start fallback
(tests/cold_start_oracle.py): every query of the seeded cases is decided, the
per-pair form the reference calls and the matrix form agree on the designed
rows, the oracle reproduces the reference-executed fixtures, and the designed
rows give the lists derived by hand."""
import numpy as np
import pytest
from conftest import dec_pairs, load_golden

import cold_start_oracle as co


@pytest.mark.parametrize("case", co.CASES, ids=co.case_id)
def test_every_query_is_decided(case):
    """A condition on the seeded inputs, not a measurement: the gaps that decide
    a list exceed 1e3 * tol(dim) for every query of every case, so no
    evaluation order within tol can change a list. (A seed that gave an
    undecided query would be replaced, never the rule.)"""
    res = co.case_oracle(case)
    assert co.MARGIN == 1e3
    print(co.case_id(case), "smallest gap / (1e3 tol)", res.slack.min(), "at query", int(res.slack.argmin()))
    assert (res.slack > 1.0).all(), np.flatnonzero(res.slack <= 1.0)


def test_tolerance_and_threshold():
    assert co.tol(16) == 20 * 2.0 ** -52 and 2 * co.tol(16) < 8.9e-15
    assert co.SMALL == 10 * 2.0 ** -52
    # sklearn's own rule at the edges the cases are built on
    assert co.similarity_matrix([[1e-16, 0, 0], [1, 0, 0]])[0, 1] == 1e-16
    assert co.similarity_matrix([[1e-16, 0], [3e-16, 0]])[0, 1] == 1e-16 * 3e-16
    assert co.similarity_matrix([[2.2e-15, 0], [1, 0]])[0, 1] == 2.2e-15
    assert co.similarity_matrix([[2.3e-15, 0], [1, 0]])[0, 1] == 1.0
    assert co.similarity_matrix([[1e-200, 0], [1, 0]])[0, 1] == 1e-200
    for name in co.TINY + ("above",):  # no tiny norm within 0.5 % of the threshold
        scale, ce, cf = co.EDGE_ROWS[name][1]
        norm = scale * np.hypot(ce, cf)
        assert norm == 0.0 or abs(norm / co.SMALL - 1.0) > 0.005, name


@pytest.mark.parametrize("case", co.EDGE_CASES, ids=co.case_id)
def test_per_pair_and_matrix_forms_agree_on_the_designed_rows(case):
    """The reference calls cosine_similarity once per pair; the oracle takes one
    matrix per case. On the designed rows both give the same list, and
    similarities within 2 tol(dim)."""
    X, ratings = co.case_inputs(case)
    res = co.case_oracle(case)
    for name, q in co.edge_rows(case).items():
        others, sims = co.pair_similarities(X, q)
        assert co.kept(others, sims) == res.lists[q], name
        assert co.slack(others, sims, case.dim) > 1.0, name
        assert np.abs(sims - res.sim[q, others]).max() <= 2 * co.tol(case.dim), name


def _feature_dict(case):
    return {int(i): {"features": np.asarray(f, dtype=np.float64), "rating": r} for i, f, r in case["item_features"]}


def test_oracle_reproduces_similar_items_fixture():
    """tests/golden/similar_items.json (the reference's _find_similar_items,
    duplicate and zero rows included), by the per-pair form: the fixture's ties
    are exact only between equal calls."""
    n_queries = 0
    for case in load_golden("similar_items.json")["cases"]:
        feats = _feature_dict(case)
        ids = list(feats)
        X = np.stack([feats[i]["features"] for i in ids])
        for q in case["queries"]:
            want = case["similar"][str(q)]
            if q not in feats:
                assert want == []  # the reference's KeyError branch: nothing for the oracle to compute
                continue
            got = co.kept(*co.pair_similarities(X, ids.index(q)))
            assert [ids[j] for j in got] == want, q
            n_queries += 1
    assert n_queries > 0


def test_oracle_reproduces_als_fallback_fixture():
    """tests/golden/als_fallback.json: the items Spark left without a prediction
    take np.mean of the oracle's list, else the global mean — values and types."""
    n_fallback = 0
    for case in load_golden("als_fallback.json")["cases"]:
        feats = _feature_dict(case)
        ids = list(feats)
        X = np.stack([feats[i]["features"] for i in ids])
        ratings = [feats[i]["rating"] for i in ids]
        spark = {int(i): p for i, p in case["spark_predictions"]}
        exp = dec_pairs(case["result"])
        assert [i for i, _ in exp] == case["query"]
        for item, want in exp:
            if spark.get(item) is not None:
                continue  # Spark's own prediction: not the fallback
            lst = co.kept(*co.pair_similarities(X, ids.index(item))) if item in feats else []
            mean = co.mean_rating(ratings, lst)
            got = case["global_mean"] if mean is None else mean
            assert float(got) == float(want) and type(got) is type(want), item
            n_fallback += 1
    assert n_fallback > 0


def _direction_cosine_list(X, skip):
    """By hand, for a query row that sklearn normalises to e (the first unit
    vector): its similarity to row o is o[0] / |o| when |o| >= 10 * eps and
    o[0] itself (tiny) otherwise. The 3 largest, kept above 0.5, in extended
    precision and without sklearn."""
    Xl = np.asarray(X, np.longdouble)
    norm = np.sqrt((Xl * Xl).sum(axis=1))
    cos = np.where(norm < co.SMALL, Xl[:, 0], Xl[:, 0] / np.where(norm < co.SMALL, 1, norm))
    others = [j for j in range(len(X)) if j != skip]
    order = sorted(others, key=lambda j: cos[j], reverse=True)[:co.K]
    return [j for j in order if cos[j] > co.THRESHOLD]


@pytest.mark.parametrize("case", co.EDGE_CASES, ids=co.case_id)
def test_designed_rows_by_hand(case):
    """The rows with a norm below 10 * eps (and the exact zero, and the rows
    whose squares underflow) keep NO similar item: each of their similarities
    is at most their own norm (about 1e-16), never near 0.5. They are kept by
    no other item either. The 2.3e-15 e row is normalised to e; its partners
    have cosines 1 / sqrt(1.01) > 1 / sqrt(1.09) > 1 / sqrt(1.25) with it, in
    that order. At dim 9 and 16 no Gaussian row comes near (the list is the
    three partners); at dim 2 and 3 some of the ~500 Gaussian rows lie within
    the partners' 6 - 27 degrees of e, so there the list is derived from the
    direction cosines o[0] / |o| in extended precision instead."""
    X, ratings = co.case_inputs(case)
    res = co.case_oracle(case)
    rows = co.edge_rows(case)
    tiny = {rows[name] for name in co.TINY}
    for name in co.TINY:
        assert res.lists[rows[name]] == [] and res.means[rows[name]] is None, name
    for q, lst in enumerate(res.lists):
        assert not tiny & set(lst), q
    partners = [rows["partner_a"], rows["partner_b"], rows["partner_c"]]
    above = rows["above"]
    cos = [res.sim[above, p] for p in partners]
    want = [1 / np.sqrt(1.01), 1 / np.sqrt(1.09), 1 / np.sqrt(1.25)]
    assert np.abs(np.array(cos) - want).max() <= 2 * co.tol(case.dim)
    by_hand = _direction_cosine_list(X, above)
    assert res.lists[above] == by_hand
    if case.dim >= 9:
        assert by_hand == partners
        assert res.means[above] == np.mean([ratings[p] for p in partners])
    # the partners themselves rank in that order among the row's similarities
    assert sorted(partners, key=lambda p: res.sim[above, p], reverse=True) == partners
    # and each partner sees the normalised row (similarity > 0.89), not the row left at 2.2e-15
    for p in partners:
        assert res.sim[p, above] > 0.89 and res.sim[p, rows["below"]] < 1e-14


@pytest.mark.parametrize("case", co.EDGE_CASES, ids=co.case_id)
def test_package_oracle_follows_the_same_rule(case):
    """oracle.fusion's numpy restatement (the checker of the other suites and of
    the benchmark's CPU leg) keeps the lists of sklearn on the designed rows."""
    from oracle import fusion as ofus

    X, ratings = co.case_inputs(case)
    res = co.case_oracle(case)
    feats = {j: {"features": X[j], "rating": ratings[j]} for j in range(case.n)}
    for name, q in co.edge_rows(case).items():
        assert ofus.find_similar_items(feats, q) == res.lists[q], name


def _chain_lists(X, small):
    """The library's arithmetic as its source states it (sequential non-FMA f64
    norm, x / norm with a norm below `small` — or equal to 0 when small is None
    — taken as 1, sequential dot), in numpy: the lists it would keep."""
    X = np.asarray(X, np.float64)
    nr = np.zeros(len(X))
    for c in range(X.shape[1]):
        nr = nr + X[:, c] * X[:, c]
    nr = np.sqrt(nr)
    nr[(nr == 0.0) if small is None else (nr < small)] = 1.0
    Xn = X / nr[:, None]
    S = np.zeros((len(X), len(X)))
    for c in range(X.shape[1]):
        S = S + Xn[:, c:c + 1] * Xn[:, c][None, :]
    return [co.kept(*co.matrix_similarities(S, q)) for q in range(len(X))], S


@pytest.mark.parametrize("case", co.CASES, ids=co.case_id)
def test_cases_tell_the_two_norm_rules_apart(case):
    """What the cases can see: a sequential f64 chain with sklearn's rule gives
    every list of the oracle (and similarities within 2 tol of sklearn's); with
    only an exact zero norm replaced it gives wrong lists on every edge case
    and none on a plain one."""
    X, _ = co.case_inputs(case)
    res = co.case_oracle(case)
    lists, S = _chain_lists(X, co.SMALL)
    off = ~np.eye(case.n, dtype=bool)
    err = np.abs(S - res.sim)[off].max()
    print(co.case_id(case), "max |chain - sklearn|", err, "2 tol", 2 * co.tol(case.dim))
    assert err <= 2 * co.tol(case.dim)
    assert lists == res.lists
    wrong = sum(a != b for a, b in zip(_chain_lists(X, None)[0], res.lists))
    print(co.case_id(case), "lists wrong under the exact-zero rule:", wrong)
    assert (wrong > 0) == case.edge
