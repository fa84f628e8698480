"""Offline quality metrics: the drop-in for src/evaluation.py.

`RecommenderEvaluator` keeps the reference's per-user dict API
(src/evaluation.py:19-149): Precision@k / Recall@k against the "manuscript"
relevance band (ratings within ±0.1 of the user's mean rating), NDCG@k on
3-level grades, MAE/RMSE after a 1–5 rescale, and `comprehensive_evaluation`.
The ranking step of P@k/R@k — `sorted(scores, reverse=True)[:k]`, stable, so
ties keep dict order — is the device's stable top-k (`hrec_topk_f64`); the
per-user set arithmetic that follows is O(k) host work. NDCG and MAE/RMSE
call the same sklearn functions the reference calls (its dependency,
requirements.txt), on the same inputs in the same set-iteration order.

`compute_f1_score` is also exported here: src/hybrid_system.py:15 imports it
from this module, where the reference never defines it.

Reference behaviour kept on purpose (pinned by tests/golden/evaluation.json,
produced by executing the reference):
  * `comprehensive_evaluation` raises ValueError — it hands dicts to
    sklearn's f1_score;
  * NDCG on a single common item and MAE/RMSE on constant ratings raise
    ValueError (sklearn rejects one document / NaN).
Plotting needs matplotlib/seaborn, which this build does not ship.

Not in the reference (failures raise): `evaluate_scores`, the same
metrics for every user of a score matrix in one device pass (`_hrec.topk`
followed by hrec_user_metrics), `summarize`, and the helpers
HybridRecommendationSystem.evaluate_users shares with it (the actual-ratings
CSR, the result frame); and `evaluate_lists`, the label-free
list-quality measures of any lists frame over any vector matrix
(hrec_list_quality).
"""
import os

import numpy as np
import torch

from . import _hrec, ranked_lists
from .als_model import compute_f1_score  # noqa: F401  (D2)

_BAND = 0.1  # the manuscript's relevance tolerance around the mean rating


def _relevance_band(actual_ratings, tolerance=_BAND):
    """(threshold, relevant item set): items rated within ±tolerance of the
    mean rating (src/evaluation.py:29-31, 142-146)."""
    threshold = np.mean(list(actual_ratings.values()))
    lo, hi = threshold - tolerance, threshold + tolerance
    return threshold, {item for item, r in actual_ratings.items() if lo <= r <= hi}


def ranked_items(predicted_scores, k):
    """The first k items of sorted(predicted_scores.items(), key=score,
    reverse=True): a stable descending top-k on the device."""
    items = list(predicted_scores.keys())
    k = int(k) if k >= 0 else max(len(items) + int(k), 0)  # Python slice [:k] semantics
    if k == 0 or not items:
        return []
    _hrec.require_device()
    vals = torch.tensor([float(v) for v in predicted_scores.values()], dtype=torch.float64, device="cuda")
    idx, _ = _hrec.topk(vals, min(int(k), len(items)))
    return [items[i] for i in idx[0].tolist()]


def _common(actual_ratings, predicted_scores):
    # the reference's set intersection, iterated in the same (hash) order
    common = set(actual_ratings.keys()) & set(predicted_scores.keys())
    return ([actual_ratings[i] for i in common], [predicted_scores[i] for i in common]) if common else None


# ------------------------------------------------- batched evaluation
EVALUATE_ROWS = 65535  # rows of one hrec_user_metrics / hrec_topk call


def metric_columns(k_values):
    """The batched frames' metric columns in the order of comprehensive_evaluation's keys."""
    cols = []
    for k in k_values:
        cols += [f"Precision@{int(k)}", f"Recall@{int(k)}"]
    return cols + ["NDCG", "MAE", "RMSE"]


def check_k_values(k_values, ndcg_k):
    ks = [int(k) for k in k_values]
    if not 1 <= len(ks) <= _hrec.UM_MAX_K:
        raise ValueError(f"k_values must hold 1 .. {_hrec.UM_MAX_K} values (got {len(ks)})")
    for k in ks + [int(ndcg_k)]:
        if not 1 <= k <= _hrec.UM_LIST_MAX:
            raise ValueError(f"k_values and ndcg_k must be in [1, {_hrec.UM_LIST_MAX}] (got {k})")
    return ks, int(ndcg_k)


def actual_csr(data, users, item_ids, rating_col="average_review_rating"):
    """The host arrays of hrec_user_metrics' actual CSR for `users` (int64,
    ascending, distinct) over the candidate ids `item_ids` (int64, distinct,
    frame order) from `data` (columns userId, itemId, rating_col): (rows int64
    [len(users)]: q, or -1 for a user without rows in `data`; indptr int64
    [len(users) + 1]; cols int32: each rated item's candidate column,
    ascending per user, -1 outside the frame; ratings f64 aligned with cols;
    frame f64: the user's ratings in frame order). Rows of other users are
    ignored. A (userId, itemId) pair held twice raises ValueError (the
    reference's dict(zip(...)) would silently keep the last one)."""
    from .ranked_lists import int_ids

    du, di = int_ids(data["userId"], "userId"), int_ids(data["itemId"], "itemId")
    r = np.asarray(data[rating_col], dtype=np.float64)
    users, item_ids = np.asarray(users, np.int64), np.asarray(item_ids, np.int64)
    n = users.size
    indptr = np.zeros(n + 1, np.int64)
    if n == 0 or du.size == 0:
        return np.full(n, -1, np.int64), indptr, np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
    q = np.minimum(np.searchsorted(users, du), n - 1)
    keep = users[q] == du
    q, di, r = q[keep], di[keep], r[keep]
    if q.size == 0:
        return np.full(n, -1, np.int64), indptr, np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
    by_user = np.argsort(q, kind="stable")  # frame order within a user
    q, di, r = q[by_user], di[by_user], r[by_user]
    if item_ids.size:
        sorter = np.argsort(item_ids, kind="stable")
        p = np.minimum(np.searchsorted(item_ids[sorter], di), item_ids.size - 1)
        col = np.where(item_ids[sorter][p] == di, sorter[p], -1)
    else:
        col = np.full(di.size, -1, np.int64)
    # one int64 key per pair (ids fit 32 bits: int_ids; q < 2^31)
    pair = np.sort(q * (1 << 32) + (di - di.min()))
    if pair.size > 1 and np.any(pair[1:] == pair[:-1]):
        raise ValueError("data holds a (userId, itemId) pair more than once: a user's ratings must be one per item")
    # by user, then by column; stable: items outside the frame (-1) first, in frame order
    by_col = np.argsort(q * (item_ids.size + 1) + (col + 1), kind="stable")
    counts = np.bincount(q, minlength=n)
    np.cumsum(counts, out=indptr[1:])
    rows = np.where(counts > 0, np.arange(n, dtype=np.int64), -1)
    return rows, indptr, col[by_col].astype(np.int32), r[by_col], r


def actual_csr_device(data, users, item_ids, rating_col, dev):
    """actual_csr as device tensors, and the host mask of the users that have rows."""
    rows, indptr, cols, ratings, frame = actual_csr(data, users, item_ids, rating_col)
    return tuple(torch.as_tensor(a, device=dev) for a in (rows, indptr, cols, ratings, frame)), rows >= 0


def metrics_frame(users, per_row, status, k_values, has_rows):
    """The batched result: userId (the users with rows, ascending), the
    reference's result keys and the row's status bits (_hrec.UM_STATUS)."""
    import pandas as pd

    per_row, status = np.asarray(per_row)[has_rows], np.asarray(status)[has_rows]
    native = _hrec.um_columns(k_values)
    frame = {"userId": np.asarray(users)[has_rows]}
    for name in metric_columns(k_values):
        frame[name] = per_row[:, native.index(name)]
    frame["status"] = status.astype(np.int32)
    return pd.DataFrame(frame)


class RecommenderEvaluator:
    """src/evaluation.py:19 — same methods and return values."""

    @staticmethod
    def evaluate_scores(data, scores, user_ids, item_ids, k_values=(5, 10, 15, 20), ndcg_k=10,
                        rating_col="average_review_rating"):
        """The per-user methods above for many users in one device pass (not
        in the reference): `scores` [len(user_ids), len(item_ids)] (f32 or f64,
        array or device tensor) holds user_ids[i]'s predicted score of
        item_ids[j]; `data` (columns userId, itemId, rating_col) the actual
        ratings, each (userId, itemId) once (else ValueError). Returns a
        DataFrame with `userId` (the users of `data` that are in user_ids,
        ascending), `Precision@k` and `Recall@k` per k of k_values (at most 8,
        each in 1 .. 1024), `NDCG` (at ndcg_k), `MAE`, `RMSE` and `status`.
        A row equals precision_at_k / recall_at_k / ndcg_at_k / mae_rmse of
        (actual = {itemId: rating} of the user's rows in frame order,
        predicted = {item_ids[j]: scores[i, j]}): Precision and Recall
        exactly, the others to the summation order. f32 scores follow the
        np.float32 arithmetic of the per-user path, f64 scores its Python
        float arithmetic. Where the per-user methods raise ValueError (NDCG
        with one common item; MAE / RMSE with one common item, constant
        ratings or scores, a NaN score) the value is NaN and the bit of
        `status` is set (_hrec.UM_STATUS names the bits). The F1_Score entry
        of comprehensive_evaluation, which raises in the reference, has no
        column. The ranking is the device's stable top-k (equal scores keep
        item_ids order, NaN last) followed by hrec_user_metrics."""
        ks, ndcg_k = check_k_values(k_values, ndcg_k)
        _hrec.require_device()
        uid = np.asarray(user_ids).reshape(-1).astype(np.int64)
        iid = np.asarray(item_ids).reshape(-1).astype(np.int64)
        if np.unique(uid).size != uid.size or np.unique(iid).size != iid.size:
            raise ValueError("evaluate_scores: user_ids and item_ids must not repeat an id")
        s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores))
        if s.dtype not in (torch.float32, torch.float64):
            s = s.to(torch.float64)
        if s.dim() != 2 or tuple(s.shape) != (uid.size, iid.size):
            raise ValueError("evaluate_scores: scores must be [len(user_ids), len(item_ids)]")
        if iid.size == 0:
            raise ValueError("evaluate_scores: no candidate item")
        s = s.cuda()
        dev = s.device
        order = np.argsort(uid, kind="stable")
        users = uid[order]
        (rows, *csr), has_rows = actual_csr_device(data, users, iid, rating_col, dev)
        inverse = np.empty_like(order)
        inverse[order] = np.arange(order.size)
        rows = rows[torch.as_tensor(inverse, device=dev)]  # score row i is user uid[i]
        kk = min(max(ks), iid.size)
        out = []
        for lo in range(0, uid.size, EVALUATE_ROWS):
            part = s[lo: lo + EVALUATE_ROWS]
            ranked, _ = _hrec.topk(part if part.is_contiguous() else part.contiguous(), kk)
            per_row, status, _ = _hrec.user_metrics(ranked, ks, (rows[lo: lo + EVALUATE_ROWS], *csr), part,
                                                    ndcg_k=ndcg_k)
            out.append(torch.cat([per_row, status.double().unsqueeze(1)], dim=1))
        ncol = 2 * len(ks) + 3
        host = (torch.cat(out) if out else torch.zeros((0, ncol + 1), dtype=torch.float64)).cpu().numpy()[order]
        return metrics_frame(users, host[:, :ncol], host[:, ncol], ks, has_rows)

    @staticmethod
    def evaluate_lists(lists, item_ids, vectors, history=None):
        """The list-quality measures (not in the reference) of any lists
        frame: `lists` has `userId` and `recommendations` (per user a list of
        (itemId, rating) tuples: what the models' recommend_for_* methods
        return); `vectors` [len(item_ids), d <= 256] (f32; array or device
        tensor) holds the vector of candidate item_ids[j] the cosines are
        taken between. Returns ranked_lists.list_quality's dict
        ("catalogCoverage", "distributionalCoverage", "gini",
        "personalization", "intraListDiversity", "unexpectedness", "novelty",
        "averagePopularity", "count", "novelty_unseen"), with k = the longest
        list of the frame; an itemId outside item_ids enters nothing. history
        (optional): a DataFrame with userId and itemId columns, typically the
        training frame; without it novelty, averagePopularity and
        unexpectedness are NaN. One hrec_list_quality pass over the lists."""
        _hrec.require_device()
        iid = ranked_lists.int_ids(np.asarray(item_ids).reshape(-1), "item_ids")
        if np.unique(iid).size != iid.size:
            raise ValueError("evaluate_lists: item_ids must not repeat an id")
        v = vectors if isinstance(vectors, torch.Tensor) else torch.as_tensor(np.asarray(vectors, np.float32))
        if v.dim() != 2 or v.shape[0] != iid.size or not 1 <= v.shape[1] <= _hrec.LQ_MAX_D:
            raise ValueError(f"evaluate_lists: vectors must be [len(item_ids), 1 .. {_hrec.LQ_MAX_D}]")
        v = v.to(torch.float32).cuda().contiguous()
        dev = v.device
        cols, lens = ranked_lists.lists_frame_columns(lists, iid)
        if cols.shape[1] > _hrec.LQ_LIST_MAX:
            raise ValueError(f"evaluate_lists: a list is longer than {_hrec.LQ_LIST_MAX}")
        hist = tables = None
        if history is not None:
            users = ranked_lists.int_ids(lists["userId"], "userId")
            uniq = np.unique(users)
            hu, hi = ranked_lists.history_frame(history)
            indptr, hcols = ranked_lists.exclusion_csr(uniq, iid, hu, hi, dev, EVALUATE_ROWS,
                                                       what="history: userId and itemId")
            hist = (torch.as_tensor(np.searchsorted(uniq, users).astype(np.int64), device=dev), indptr, hcols)
            tables = ranked_lists.history_tables(hu, hi, iid, dev)

        def batches():
            for lo in range(0, cols.shape[0], EVALUATE_ROWS):
                sl = slice(lo, lo + EVALUATE_ROWS)
                yield (torch.as_tensor(cols[sl], device=dev), torch.as_tensor(lens[sl], device=dev),
                       None if hist is None else (hist[0][sl], *hist[1:]))

        return ranked_lists.list_quality(batches, v, int(v.shape[1]), max(int(cols.shape[1]), 1), tables)

    @staticmethod
    def diversify_lists(lists, item_ids, vectors, mmr, num):
        """Greedy Maximal Marginal Relevance over any lists frame (not in the
        reference): `lists`, `item_ids` and `vectors` as in evaluate_lists,
        each list a pool of (itemId, rating) tuples, best first, of at most
        1024 entries; mmr a ranked_lists.MMR (its lambda_ is used; the pool is
        the list as given). Returns a frame with the same first column and
        `recommendations`: per list min(num, its entries inside item_ids) of
        its own tuples, unchanged, in SELECTION order (hrec_mmr_rerank: each
        pick trades its rating, min-max scaled over the list, against its
        largest cosine to the picks before). A tuple whose itemId is outside
        item_ids is never picked. num > the longest list is clipped to it."""
        import pandas as pd

        _hrec.require_device()
        mmr = ranked_lists.check_mmr(mmr)
        num = ranked_lists.check_num(num, ranked_lists.MMR.POOL_MAX, "num")
        iid = ranked_lists.int_ids(np.asarray(item_ids).reshape(-1), "item_ids")
        if np.unique(iid).size != iid.size:
            raise ValueError("diversify_lists: item_ids must not repeat an id")
        v = vectors if isinstance(vectors, torch.Tensor) else torch.as_tensor(np.asarray(vectors, np.float32))
        if v.dim() != 2 or v.shape[0] != iid.size or not 1 <= v.shape[1] <= _hrec.LQ_MAX_D:
            raise ValueError(f"diversify_lists: vectors must be [len(item_ids), 1 .. {_hrec.LQ_MAX_D}]")
        v = v.to(torch.float32).cuda().contiguous()
        dev = v.device
        recs = list(lists["recommendations"])
        cols, lens = ranked_lists.lists_frame_columns(lists, iid)
        if cols.shape[1] > ranked_lists.MMR.POOL_MAX:
            raise ValueError(f"diversify_lists: a list is longer than {ranked_lists.MMR.POOL_MAX}")
        key = lists.columns[0]
        if cols.shape[1] == 0 or iid.size == 0:
            return pd.DataFrame({key: lists[key].to_numpy(), "recommendations": [[] for _ in recs]})
        scores = np.full(cols.shape, np.nan, np.float64)
        scores[np.arange(cols.shape[1])[None, :] < lens[:, None]] = [float(s) for r in recs for _, s in r]
        inv = _hrec.row_inv_norms(v)
        kk = min(num, int(cols.shape[1]))
        out = []
        for lo in range(0, cols.shape[0], EVALUATE_ROWS):
            sl = slice(lo, lo + EVALUATE_ROWS)
            pos, out_len, _ = _hrec.mmr_rerank(torch.as_tensor(cols[sl], device=dev),
                                               torch.as_tensor(scores[sl], device=dev), v, inv, mmr.lambda_, kk,
                                               pool_len=torch.as_tensor(lens[sl], device=dev))
            out.append(torch.cat([pos, out_len.unsqueeze(1)], dim=1))
        host = torch.cat(out).cpu().numpy()
        picked = [[r[p] for p in row[:row[-1]]] for r, row in zip(recs, host.tolist())]
        return pd.DataFrame({key: lists[key].to_numpy(), "recommendations": picked})

    @staticmethod
    def similar_rows(vectors, ids, queries=None, num=10, min_similarity=None):
        """Cosine neighbours among the rows of any matrix (not in the
        reference; user-tower outputs for instance): `vectors` [len(ids), d <=
        256] (f32; array or device tensor) holds the vector of ids[j] (int,
        distinct). Returns a lists frame with `id` (queries None: every id, in
        row order; an array-like otherwise: its distinct ids ascending, those
        outside `ids` left out) and `recommendations`: the `num` (1 .. 1024)
        nearest other rows as (id, similarity: float) tuples, best first;
        equal similarities keep the earlier row first; min_similarity (None:
        no cut) keeps the similarities above it. hrec_cosine_topk: the same
        bits on every call. evaluate_lists and diversify_lists take the frame
        as it is."""
        _hrec.require_device()
        iid = ranked_lists.int_ids(np.asarray(ids).reshape(-1), "ids")
        if np.unique(iid).size != iid.size:
            raise ValueError("similar_rows: ids must not repeat an id")
        v = vectors if isinstance(vectors, torch.Tensor) else torch.as_tensor(np.asarray(vectors, np.float32))
        if v.dim() != 2 or v.shape[0] != iid.size or not 1 <= v.shape[1] <= _hrec.LQ_MAX_D:
            raise ValueError(f"similar_rows: vectors must be [len(ids), 1 .. {_hrec.LQ_MAX_D}]")
        v = v.to(torch.float32).cuda().contiguous()
        return ranked_lists.similar_rows_frame("id", iid, v, int(v.shape[1]), queries, num, min_similarity)

    @staticmethod
    def summarize(frame):
        """Per metric column of an evaluate_scores / evaluate_users frame: its
        mean over the users where it is defined (not NaN) and their count, as
        a DataFrame indexed by metric with columns `mean` and `count`."""
        import pandas as pd

        names = [c for c in frame.columns if c not in ("userId", "status")]
        means, counts = [], []
        for c in names:
            v = frame[c].to_numpy(dtype=np.float64)
            n = int(np.sum(~np.isnan(v)))
            means.append(float(np.nanmean(v)) if n else float("nan"))
            counts.append(n)
        return pd.DataFrame({"mean": means, "count": counts}, index=pd.Index(names, name="metric"))

    def __init__(self):
        from sklearn.preprocessing import MinMaxScaler

        self.scaler = MinMaxScaler()
        self.rating_scaler = MinMaxScaler()

    def precision_at_k(self, actual_ratings, predicted_scores, k=10):
        _, relevant = _relevance_band(actual_ratings)
        hits = sum(1 for item in ranked_items(predicted_scores, k) if item in relevant)
        return hits / k if k > 0 else 0.0

    def recall_at_k(self, actual_ratings, predicted_scores, k=10):
        _, relevant = _relevance_band(actual_ratings)
        if not relevant:
            return 0.0
        return len(set(ranked_items(predicted_scores, k)) & relevant) / len(relevant)

    def ndcg_at_k(self, actual_ratings, predicted_scores, k=10):
        from sklearn.metrics import ndcg_score

        pair = _common(actual_ratings, predicted_scores)
        if pair is None:
            return 0.0
        y_true, y_pred = (np.array(v).reshape(-1, 1) for v in pair)
        # both columns on the TRUE ratings' min-max fit, then 3 grades
        t = self.rating_scaler.fit_transform(y_true).ravel()
        p = self.rating_scaler.transform(y_pred).ravel()
        edges = [0.33, 0.66]
        return ndcg_score([np.digitize(t, edges)], [np.digitize(p, edges)], k=k)

    def mae_rmse(self, actual_ratings, predicted_scores):
        from sklearn.metrics import mean_absolute_error, mean_squared_error

        pair = _common(actual_ratings, predicted_scores)
        if pair is None:
            return 0.0, 0.0

        def to_1_5(v):
            lo, hi = min(v), max(v)
            return 1 + 4 * (np.array(v) - lo) / (hi - lo)

        with np.errstate(divide="ignore", invalid="ignore"):  # constant input -> NaN -> sklearn raises
            t, p = to_1_5(pair[0]), to_1_5(pair[1])
        return mean_absolute_error(t, p), np.sqrt(mean_squared_error(t, p))

    def _binarize(self, ratings_dict, tolerance=0.1):
        threshold = np.mean(list(ratings_dict.values()))
        return {item: int(threshold - tolerance <= r <= threshold + tolerance) for item, r in ratings_dict.items()}

    def comprehensive_evaluation(self, actual_ratings, predicted_scores, k_values=(5, 10, 15, 20)):
        from sklearn.metrics import f1_score

        results = {}
        for k in k_values:
            results[f"Precision@{k}"] = self.precision_at_k(actual_ratings, predicted_scores, k)
            results[f"Recall@{k}"] = self.recall_at_k(actual_ratings, predicted_scores, k)
        # the reference passes the binarised DICTS to sklearn, which
        # rejects them (ValueError) — kept as the reference behaves.
        results["F1_Score"] = f1_score(self._binarize(actual_ratings), self._binarize(predicted_scores))
        results["NDCG"] = self.ndcg_at_k(actual_ratings, predicted_scores)
        results["MAE"], results["RMSE"] = self.mae_rmse(actual_ratings, predicted_scores)
        return results

    def plot_precision_recall_at_k(self, results_dict, k_values, model_name, save_path=None):
        try:
            import matplotlib.pyplot as plt  # noqa: F401
        except ImportError as e:
            raise ImportError("plot_precision_recall_at_k needs matplotlib, which this build does not ship") from e
        raise NotImplementedError("plotting is outside the MI355X hot path")

    def load_predictions(self, user_id, pred_dir="results/predictions"):
        import pandas as pd

        df = pd.read_csv(os.path.join(pred_dir, f"user_{user_id}_predictions.csv"))
        return list(zip(df["itemId"], df["hybrid_score"]))
