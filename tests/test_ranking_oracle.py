"""CPU: the plain-Python ranking oracle (tests/ranking_oracle.py) against the
three-row example of Spark's RankingMetricsSuite: the fractions at 1e-15, the
decimals (as the suite prints them) at 1e-5."""
import math

import pytest
from ranking_oracle import gain_table, mean_metrics, row_metrics

PREDS = [[1, 6, 2, 7, 8, 3, 9, 10, 4, 5], [4, 1, 5, 6, 2, 7, 3, 8, 9, 10], [1, 2, 3, 4, 5]]
LABELS = [[1, 2, 3, 4, 5], [1, 2, 3], []]
PRECISION, RECALL, MAP, MAP_K, NDCG = range(5)

FRACTIONS = [
    (PRECISION, 1, 1 / 3), (PRECISION, 2, 1 / 3), (PRECISION, 3, 1 / 3), (PRECISION, 4, 0.25),
    (PRECISION, 5, 4 / 15), (PRECISION, 10, 4 / 15), (PRECISION, 15, 8 / 45),
    (RECALL, 1, 1 / 15), (RECALL, 2, 8 / 45), (RECALL, 3, 11 / 45), (RECALL, 4, 11 / 45), (RECALL, 5, 16 / 45),
    (RECALL, 10, 2 / 3), (RECALL, 15, 2 / 3),
    (MAP_K, 1, 1 / 3), (MAP_K, 2, 0.25), (NDCG, 3, 1 / 3),
]
DECIMALS = [(MAP, 10, 0.355026), (NDCG, 5, 0.328788), (NDCG, 10, 0.487913), (NDCG, 15, 0.487913)]


@pytest.mark.parametrize("metric,k,expected", FRACTIONS)
def test_spark_example_fractions(metric, k, expected):
    assert mean_metrics(PREDS, LABELS, k)[metric] == pytest.approx(expected, rel=0, abs=1e-15)


@pytest.mark.parametrize("metric,k,expected", DECIMALS)
def test_spark_example_decimals(metric, k, expected):
    assert mean_metrics(PREDS, LABELS, k)[metric] == pytest.approx(expected, rel=0, abs=1e-5)


def test_map_does_not_depend_on_k():
    assert len({mean_metrics(PREDS, LABELS, k)[MAP] for k in (1, 2, 5, 10, 15, 1000)}) == 1


def test_rows_by_hand():
    # row 1: hits at positions 0, 2, 5, 8, 9 of 10, five labels
    p, r, ap, ap_k, ndcg = row_metrics(PREDS[0], LABELS[0], 5)
    assert p == 2 / 5 and r == 2 / 5
    assert ap == ((((1 / 1 + 2 / 3) + 3 / 6) + 4 / 9) + 5 / 10) / 5
    assert ap_k == (1 / 1 + 2 / 3) / 5
    g = gain_table(5)
    assert ndcg == (g[0] + g[2]) / ((((g[0] + g[1]) + g[2]) + g[3]) + g[4])
    assert row_metrics(PREDS[2], LABELS[2], 5) == (0.0, 0.0, 0.0, 0.0, 0.0)


def test_duplicates_short_lists_and_a_given_gain_table():
    # labels count once; a list shorter than k and than the label set; an empty list
    assert row_metrics([7, 7], [7, 7, 9], 4) == row_metrics([7, 7], [9, 7], 4)
    p, r, ap, ap_k, ndcg = row_metrics([7, 7], [9, 7], 4)
    assert (p, r) == (2 / 4, 2 / 2) and ap == (1 / 1 + 2 / 2) / 2 and ap_k == ap
    g = gain_table(4)
    assert ndcg == (g[0] + g[1]) / (g[0] + g[1])  # n = min(max(2, 2), 4) = 2
    assert row_metrics([], [1, 2], 3) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert row_metrics([5], [-1, 5, 2 ** 40], 1, gain=[2.0])[NDCG] == 1.0
    assert math.isnan(mean_metrics([], [], 3)[0])
