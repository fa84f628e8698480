"""Spark 3.5 RankingMetrics with binary relevance, restated in plain Python:
the reference the ranking kernel (hrec_ranking_metrics) and
ALSModel.ranking_metrics are tested against. Python floats (IEEE f64), sums
added one term at a time in ascending position, set() for the labels.

row_metrics(pred, labels, k) -> (precision@k, recall@k, AP, AP@k, NDCG@k) of
one row; an empty label set gives five zeros (Spark logs a warning and
returns 0.0). gain (optional): the table gain[i] = 1 / ln(i + 2) to use in
place of math.log, for a bit-for-bit comparison with a caller that made its
table another way."""
import math


def gain_table(k):
    return [1.0 / math.log(i + 2) for i in range(k)]


def row_metrics(pred, labels, k, gain=None):
    lab = set(int(x) for x in labels)
    pred = [int(x) for x in pred]
    m, n_pred = len(lab), len(pred)
    if m == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0)
    gain = gain_table(k) if gain is None else [float(g) for g in gain]
    hits_k = sum(1 for i in range(min(n_pred, k)) if pred[i] in lab)
    precision = hits_k / k
    recall = hits_k / m

    def prec_sum(n):
        cnt, total = 0, 0.0
        for i in range(n):
            if pred[i] in lab:
                cnt += 1
                total = total + cnt / (i + 1)
        return total

    ap = prec_sum(min(max(n_pred, m), n_pred)) / min(m, max(n_pred, m))
    ap_k = prec_sum(min(k, n_pred)) / min(m, k)
    n = min(max(n_pred, m), k)
    dcg = 0.0
    for i in range(min(n, n_pred)):
        if pred[i] in lab:
            dcg = dcg + gain[i]
    idcg = 0.0
    for i in range(min(m, n)):
        idcg = idcg + gain[i]
    return (precision, recall, ap, ap_k, dcg / idcg)


def mean_metrics(preds, label_sets, k, gain=None):
    """(mean precision@k, recall@k, MAP, MAP@k, NDCG@k) over the rows, by
    math.fsum / count; NaNs for no rows."""
    rows = [row_metrics(p, lab, k, gain) for p, lab in zip(preds, label_sets)]
    if not rows:
        return (float("nan"),) * 5
    return tuple(math.fsum(r[j] for r in rows) / len(rows) for j in range(5))
