"""Hybrid ALS + two-tower fusion — drop-in for the reference's src/hybrid_system.py.

Same class and methods as src/hybrid_system.py:20-120. adaptive_fusion and
the top-k of get_hybrid_recommendations run on the device through
hrec_fuse_topk (K9): sklearn MinMaxScaler arithmetic per model in its numpy
dtype, the (0.8, 0.2) / (0.2, 0.8) weights chosen by the strict
als_f1 > tt_f1 test, f64 fusion with numpy 1.21's scalar promotion (the
pinned numpy, requirements.txt:5), and a stable descending top-k that keeps
Python's sorted(..., reverse=True) tie order. The item order of the fused
list is the iteration order of set(als).union(set(tt)) (:61), built on the
host exactly as the reference builds it.

Not in the reference (failures raise): recommend_for_users /
recommend_for_all_users (the fused model's top-n lists for many users in one
device pass, with an optional seen-item exclusion) and ranking_metrics /
evaluate_ranking (Spark's five ranking metrics of those lists against a
held-out frame) — hrec_hybrid_lists over both models' batched scores. Equal
fused scores keep candidate-frame order there, not the set order above.
With actual= those four fuse each user by its own F1@k (DESIGN §23:
hrec_hybrid_model_f1, hrec_hybrid_lists_rowwise); evaluate_models /
fit_fusion_weights are the batch form of evaluate_individual_models.
evaluate_users is the batch form of the reference's evaluation loop
(RecommenderEvaluator's metrics of all three models per user; DESIGN §24:
hrec_user_metrics over the same scores and lists).
rank_of / full_ranking_metrics / evaluate_full_ranking place every held-out
item among ALL candidates of the fused ranking (expected percentile rank,
AUC, uncut reciprocal rank; DESIGN §26: hrec_rank_positions' fused source).
list_quality_metrics / evaluate_list_quality say what the fused lists look
like as a whole (coverage, Gini, novelty, diversity, unexpectedness; DESIGN
§27: hrec_list_quality over the lists' columns, still on the device).
"""
import itertools
import os
import warnings

import numpy as np
import pandas as pd
import torch
from sklearn.preprocessing import MinMaxScaler

from . import _hrec, ranked_lists
from .als_model import ALSModel
from .evaluation import compute_f1_score
from .two_tower_model import TwoTowerModel

warnings.filterwarnings("ignore")

def _as_scores(values):
    """np.array(list) as the reference builds it, then the dtype
    MinMaxScaler computes in (ints/bools -> float64, float32 stays)."""
    arr = np.array(values)
    if arr.dtype == np.float32:
        out = arr
    else:
        out = arr.astype(np.float64)
    if out.size == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 1)) while a minimum of 1 is required by "
                         "MinMaxScaler.")
    if np.isinf(out).any():
        raise ValueError("Input X contains infinity or a value too large for dtype('float64').")
    return out


def _set_fitted(scaler, lo, hi, n, dtype):
    """Leave `scaler` in the state MinMaxScaler.fit_transform of an [n, 1]
    column of `dtype` with min lo / max hi leaves it (the reference refits both
    scalers per fusion, src/hybrid_system.py:66-67); the O(1) attribute
    arithmetic is sklearn's (_data.py partial_fit, feature_range (0, 1))."""
    dmin = np.array([lo], dtype=dtype)
    dmax = np.array([hi], dtype=dtype)
    drange = dmax - dmin
    safe = drange.copy()
    safe[safe < 10 * np.finfo(safe.dtype).eps] = 1.0
    scaler.n_features_in_ = 1
    scaler.n_samples_seen_ = int(n)
    scaler.data_min_, scaler.data_max_, scaler.data_range_ = dmin, dmax, drange
    scaler.scale_ = (1 - 0) / safe
    scaler.min_ = 0 - dmin * scaler.scale_


def fuse_device(als_scores, tt_scores, als_wins, top_k, device=None, want_fused=True, scalers=None):
    """Fusion + stable top-k on the device. Returns (fused f64 [n] or None,
    top indices, top scores) as numpy arrays. `scalers` = (als_scaler,
    tt_scaler) are left fitted as the reference's fit_transform leaves them."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(als_scores, device=device)
    t = torch.as_tensor(tt_scores, device=device)
    n = a.numel()
    kk = n if top_k is None else (max(n + top_k, 0) if top_k < 0 else min(top_k, n))
    mm = torch.empty(4, dtype=torch.float64, device=device) if scalers is not None else None
    idx, sc, fused = _hrec.fuse_topk(a, t, als_wins, kk, want_fused=want_fused, minmax=mm)
    fused_np = fused.cpu().numpy() if fused is not None else None
    if scalers is not None:
        m = mm.cpu().numpy()
        _set_fitted(scalers[0], m[0], m[1], n, np.float64)
        _set_fitted(scalers[1], m[2], m[3], n, np.dtype(tt_scores.dtype))
    return fused_np, idx.cpu().numpy(), sc.cpu().numpy()


def _unique(vals, col):
    """No repeated id: a bincount when the ids are small non-negative ints
    (catalogue ids), else pandas' hash check."""
    if vals.size == 0:
        return True
    lo, hi = int(vals.min()), int(vals.max())
    if lo >= 0 and hi < 4 * vals.size + 4096:
        return int(np.bincount(vals.astype(np.int64, copy=False)).max()) <= 1
    return bool(col.is_unique)


def _scored(model, cls, user_id, all_items):
    if type(model).predict_for_user is cls.predict_for_user:
        return model._predict_device(user_id, all_items)
    return model.predict_for_user(user_id, all_items)


class HybridRecommendationSystem:
    def __init__(self):
        self.als_model = None
        self.twotower_model = None
        self.als_scaler = MinMaxScaler()
        self.twotower_scaler = MinMaxScaler()
        self.als_f1_score = 0.0
        self.twotower_f1_score = 0.0
        self.models_loaded = False
        self._flags_bad = False

    def load_models(self, als_model_path, twotower_model_path):
        try:
            print("=== Loading Pre-trained Models ===")
            self.als_model = ALSModel().load_model(als_model_path)
            self.twotower_model = TwoTowerModel.load_model(twotower_model_path)
            self.models_loaded = True
            print("\n=== Models loaded successfully ===")
            return True
        except Exception as e:
            print(f"Error loading models: {str(e)}")
            return False

    def evaluate_individual_models(self, test_user_id, actual_ratings, all_items, k=10):
        try:
            als_preds = self.als_model.predict_for_user(test_user_id, all_items)
            tt_preds = self.twotower_model.predict_for_user(test_user_id, all_items)
            self.als_f1_score = compute_f1_score(actual_ratings, dict(als_preds))
            self.twotower_f1_score = compute_f1_score(actual_ratings, dict(tt_preds))
            print(f"Model F1 Scores - ALS: {self.als_f1_score:.4f}, "
                  f"Two-Tower: {self.twotower_f1_score:.4f}")
            return self.als_f1_score, self.twotower_f1_score
        except Exception as e:
            print(f"Error evaluating models: {str(e)}")
            return 0.0, 0.0

    def _union(self, als_predictions, twotower_predictions):
        als_dict = dict(als_predictions)
        tt_dict = dict(twotower_predictions)
        items = list(set(als_dict.keys()).union(set(tt_dict.keys())))
        # [d.get(item, 0) for item in items] (:62-63), via map (same values)
        als_scores = _as_scores(list(map(als_dict.get, items, itertools.repeat(0))))
        tt_scores = _as_scores(list(map(tt_dict.get, items, itertools.repeat(0))))
        return items, als_scores, tt_scores

    def adaptive_fusion(self, als_predictions, twotower_predictions):
        try:
            items, als_scores, tt_scores = self._union(als_predictions, twotower_predictions)
            fused, _, _ = fuse_device(als_scores, tt_scores, self.als_f1_score > self.twotower_f1_score, 0,
                                      scalers=(self.als_scaler, self.twotower_scaler))
            return [(item, fused[i]) for i, item in enumerate(items)]
        except Exception as e:
            print(f"Error in adaptive fusion: {str(e)}")
            return []

    def save_predictions(self, user_id, predictions, save_dir="results/predictions"):
        os.makedirs(save_dir, exist_ok=True)
        file_path = os.path.join(save_dir, f"user_{user_id}_predictions.csv")
        df = pd.DataFrame(predictions, columns=["itemId", "hybrid_score"])
        df["userId"] = user_id
        df["prediction_rank"] = range(1, len(df) + 1)
        df["timestamp"] = pd.Timestamp.now()
        df.to_csv(file_path, index=False)
        print(f"Predictions saved to {file_path}")
        return file_path

    def load_predictions(self, user_id, save_dir="results/predictions"):
        file_path = os.path.join(save_dir, f"user_{user_id}_predictions.csv")
        if not os.path.exists(file_path):
            raise FileNotFoundError(f"No predictions found for user {user_id}")
        df = pd.read_csv(file_path)
        return list(zip(df["itemId"], df["hybrid_score"]))

    def get_hybrid_recommendations(self, user_id, all_items, actual_ratings=None, top_k=5,
                                   save_predictions=False):
        if not self.models_loaded:
            raise ValueError("Models not loaded. Call load_models() first.")
        try:
            # the drop-in models hand over device scores (the lists are built
            # below only if the list path runs); other model objects are used
            # through their predict_for_user as the reference does
            als_preds = _scored(self.als_model, ALSModel, user_id, all_items)
            tt_fast = None
            if (not save_predictions and not actual_ratings
                    and type(self.twotower_model).predict_for_user is TwoTowerModel.predict_for_user):
                # the candidate frame's item inputs built on the device (ids,
                # scaler, uniqueness checked there; read back with the top-k)
                tt_fast = self.twotower_model._predict_device_fast(user_id, all_items)
            if tt_fast is not None:
                self._flags_bad = False
                try:
                    top = self._top_on_device(als_preds, tt_fast[:2], top_k, flags=tt_fast[2])
                except Exception:
                    top, self._flags_bad = None, True
                if top is not None:
                    return top
                # ties or NaN scores: the list path on the same scores; bad
                # inputs: the host path (raises where the reference raises)
                tt_preds = tt_fast[:2] if not self._flags_bad else _scored(self.twotower_model, TwoTowerModel,
                                                                           user_id, all_items)
            else:
                tt_preds = _scored(self.twotower_model, TwoTowerModel, user_id, all_items)
            if actual_ratings:
                self.evaluate_individual_models(user_id, actual_ratings, all_items)
            if not save_predictions and tt_fast is None:
                try:
                    top = self._top_on_device(als_preds, tt_preds, top_k)
                except Exception:  # the list path below meets the same error and reports it as the reference does
                    top = None
                if top is not None:
                    return top
            if isinstance(als_preds, tuple):  # the lists predict_for_user returns (:101-102)
                als_preds = self.als_model._predictions_guarded(als_preds[0], als_preds[2])
            if isinstance(tt_preds, tuple):
                tt_preds = self.twotower_model._predictions(*tt_preds)
            try:
                items, als_scores, tt_scores = self._union(als_preds, tt_preds)
                fused, idx, sc = fuse_device(als_scores, tt_scores, self.als_f1_score > self.twotower_f1_score,
                                             top_k, want_fused=save_predictions,
                                             scalers=(self.als_scaler, self.twotower_scaler))
            except Exception as e:  # adaptive_fusion's own guard (:73-75) -> []
                print(f"Error in adaptive fusion: {str(e)}")
                items, fused, idx, sc = [], None, [], []
            top_recommendations = [(items[i], np.float64(s)) for i, s in zip(idx, sc)]
            if save_predictions:
                combined = [(item, fused[i]) for i, item in enumerate(items)] if fused is not None else []
                self.save_predictions(user_id, combined)
            return top_recommendations
        except Exception as e:
            print(f"Error generating recommendations: {str(e)}")
            return []

    def _top_on_device(self, als_side, tt_side, top_k, flags=None):
        """get_hybrid_recommendations without the Python lists: when both
        sides cover the same unique candidate ids (or the ALS side is empty,
        the reference's DataFrame wiring) the union is those ids;
        the fusion runs on the device scores (a cold ALS user's rows already
        hold the model's fallback vector, ALSModel._predict_device) and the
        top_k + 1 fused scores come back. If they are finite and strictly decreasing, the stable
        top_k is the same whatever order the reference's set(...) union put
        the items in, so it is returned; otherwise (ties, NaN/inf scores,
        duplicate or mismatched ids) None sends the call down the list path,
        which reproduces the set order exactly. The scalers are fitted as
        fit_transform leaves them either way (min/max are order-free).
        flags: the device input flags of TwoTowerModel._predict_device_fast
        (its device check replaces the host uniqueness pass); read back with
        the top-k; non-zero sets self._flags_bad and returns None."""
        if not isinstance(tt_side, tuple) or not isinstance(top_k, (int, np.integer)) or top_k < 0:
            return None
        frame, t = tt_side
        col = frame["itemId"]
        vals = col.values
        if not isinstance(vals, np.ndarray) or vals.dtype.kind not in "iu":
            return None
        if flags is None and not _unique(vals, col):
            return None
        n = t.numel()
        if isinstance(als_side, tuple):
            items, keys, a = als_side
            if keys.shape != vals.shape or not np.array_equal(keys, vals):
                return None
            a = a.double()
            def item(i): return items[i]      # the union keeps the ALS side's key objects
        elif not als_side:
            a = torch.zeros(n, dtype=torch.float64, device=t.device)  # finite: only t is checked below
            def item(i): return vals.item(i)  # iterating the Series yields .item() scalars
        else:
            return None
        k = min(int(top_k), n)
        k1 = min(k + 1, n)
        mm = torch.empty(4, dtype=torch.float64, device=t.device)
        idx, sc, _ = _hrec.fuse_topk(a, t, self.als_f1_score > self.twotower_f1_score, k1, want_fused=False,
                                     minmax=mm)
        fin = torch.isfinite(t).all()
        if isinstance(als_side, tuple):
            fin = fin & torch.isfinite(a).all()
        bad = fin.logical_not().double().view(1)
        parts = [sc, idx.double(), mm, bad] + ([flags.double()] if flags is not None else [])
        host = torch.cat(parts).cpu().numpy()
        sc_h, idx_h, m = host[:k1], host[k1:2 * k1].astype(np.int64), host[2 * k1: 2 * k1 + 4]
        if flags is not None and host[2 * k1 + 5] != 0:
            self._flags_bad = True
            return None
        if host[2 * k1 + 4] != 0 or not np.all(sc_h[:-1] > sc_h[1:]):
            return None
        _set_fitted(self.als_scaler, m[0], m[1], n, np.float64)
        _set_fitted(self.twotower_scaler, m[2], m[3], n, np.float32)
        return [(item(int(i)), np.float64(s)) for i, s in zip(idx_h[:k], sc_h[:k])]

    # ------------------------------------- batch top-n lists / ranking metrics
    # None of these has a counterpart in the reference: failures raise. The
    # third member of the family ALSModel.recommend_for_* / TwoTowerModel.
    # recommend_for_users started, over the same ranked_lists helpers.
    RECOMMEND_MAX = 1024               # largest list length (the library's top_k limit)
    RECOMMEND_SCORE_BYTES = 1 << 30    # a sub-batch's two score matrices (mode 1: its key matrix) stay under this
    RECOMMEND_ROWS = 65535             # rows of one hrec_hybrid_lists call
    RANKING_HOST_ROWS = TwoTowerModel.RANKING_HOST_ROWS
    RANKING_METRIC_NAMES = TwoTowerModel.RANKING_METRIC_NAMES

    def _require_models(self):
        if not self.models_loaded:
            raise ValueError("Models not loaded. Call load_models() first.")

    def _als_fallback(self, users, keys):
        """The f64 device vector that stands in for NaN transform results
        (ALSModel._cold_scores: what _predictions substitutes per item), or
        None when the ALS model knows every queried user and every candidate.
        Unknown ids without that vector raise ValueError."""
        m = self.als_model.model
        if m is None:
            raise RuntimeError("the ALS model is not trained or loaded")
        cold_users = int((m._lookup(m.user_ids, users) < 0).sum())
        cold_items = int((m._lookup(m.item_ids, keys) < 0).sum())
        if not cold_users and not cold_items:
            return None
        fb = self.als_model._cold_scores(keys)
        if fb is None:
            raise ValueError(f"{cold_users} queried user(s) and {cold_items} candidate item(s) are unknown to the ALS "
                             "model and its cold-start fallback vector is not available (item_features missing, "
                             "non-finite or outside hrec_cold_fallback); the per-call similarity search is not "
                             "part of the batched lists")
        return fb

    def _spans(self, s, e, N, row_bytes):
        """[s, e) cut into sub-batches whose rows of row_bytes * N bytes stay under RECOMMEND_SCORE_BYTES."""
        sub = max(1, min(self.RECOMMEND_ROWS, self.RECOMMEND_SCORE_BYTES // (row_bytes * N)))
        return [(s1, min(s1 + sub, e)) for s1 in range(s, e, sub)]

    def _scores(self, users, cand):
        """(ALS f32 [m, N] — transform's, NaN where an id is unknown —, two-tower f32 [m, N] — the bits
        predict_for_user gives) of a sub-batch of users."""
        tt = self.twotower_model
        a = self.als_model.model.score(users, cand.item_ids)
        U = tt.model.user_vectors(torch.as_tensor(users.astype(np.int32), device=tt.model.device))
        return a, _hrec.tt_score(U, cand.vectors)

    def _labels(self, users, cand, actual):
        """The device label inputs of hrec_hybrid_model_f1 for the queried
        `users` (ascending, distinct) from an `actual` frame (userId, itemId):
        (label_rows int64 [n]: q, or -1 for a user without rows in `actual`;
        indptr, cols: row q's distinct candidate FRAME ROW indices, ascending;
        total int32 [n]: the user's distinct itemIds, inside the candidate
        frame or not)."""
        dev = self.twotower_model.model.device
        au, ai = ranked_lists.int_ids(actual["userId"], "userId"), ranked_lists.int_ids(actual["itemId"], "itemId")
        indptr, cols = ranked_lists.exclusion_csr(users, cand.item_ids, au, ai, dev,
                                                  self.twotower_model.EXCLUSION_HOST_PAIRS,
                                                  what="actual: userId and itemId")
        total = ranked_lists.distinct_counts(users, au, ai, dev, self.RANKING_HOST_ROWS)
        rows = torch.arange(int(users.size), dtype=torch.int64, device=dev)
        return torch.where(total > 0, rows, torch.full_like(rows, -1)), indptr, cols, total

    def _adaptive_device(self, users, cand, kk, excl, fallback, labels, f1_k, als_wins):
        """Per sub-batch of `users`: both models' scores, hrec_hybrid_model_f1
        (mode 0) over them and — kk > 0 — hrec_hybrid_lists_rowwise (mode 0)
        with the weights the F1s just chose. All flags of both kinds are read
        back once, after the last sub-batch. A sub-batch whose F1 flag is set
        is redone whole (F1 in mode 1, the lists in mode 0 with their own flag
        read, then in mode 1 if it is set); one with only the lists flag set
        is redone in lists mode 1 with the weights it has. Returns device (f1
        f64 [n, 2], wins int32 [n], idx, val, lens) (the last three None when
        kk == 0)."""
        dev = self.twotower_model.model.device
        n, N = int(users.size), len(cand)
        f1 = torch.empty((n, 2), dtype=torch.float64, device=dev)
        wins = torch.empty(n, dtype=torch.int32, device=dev)
        idx = val = lens = None
        if kk:
            idx = torch.empty((n, kk), dtype=torch.int64, device=dev)
            val = torch.empty((n, kk), dtype=torch.float64, device=dev)
            lens = torch.empty(n, dtype=torch.int32, device=dev)
            rows = torch.arange(n, dtype=torch.int64, device=dev)  # query q reads exclusion row q

        def f1_pass(s, e, a, t, mode):
            f, w, over = _hrec.hybrid_model_f1(a, t, f1_k, labels=(labels[0][s:e], *labels[1:]),
                                               default_wins=als_wins, fallback=fallback, mode=mode)
            f1[s:e], wins[s:e] = f, w
            return over

        def lists_pass(s, e, a, t, mode):
            i, v, m, over = _hrec.hybrid_lists_rowwise(a, t, kk, wins[s:e], fallback=fallback,
                                                       excl=None if excl is None else (rows[s:e], *excl), mode=mode)
            idx[s:e], val[s:e], lens[s:e] = i, v, m
            return over

        spans = self._spans(0, n, N, 8)
        flags = []
        for s, e in spans:
            a, t = self._scores(users[s:e], cand)
            flags.append(f1_pass(s, e, a, t, 0))
            if kk:
                flags.append(lists_pass(s, e, a, t, 0))
        flags = torch.cat(flags).tolist()  # one host read
        per = 2 if kk else 1
        for q, (s, e) in enumerate(spans):
            f1_over, lists_over = flags[per * q], bool(kk) and flags[per * q + 1]
            if not f1_over and not lists_over:
                continue
            for s1, e1 in self._spans(s, e, N, 16):
                a, t = self._scores(users[s1:e1], cand)
                if f1_over:
                    f1_pass(s1, e1, a, t, 1)
                    if kk and int(lists_pass(s1, e1, a, t, 0).item()):
                        lists_pass(s1, e1, a, t, 1)
                else:
                    lists_pass(s1, e1, a, t, 1)
        return f1, wins, idx, val, lens

    def _recommend_device(self, users, cand, num, exclude=None, actual=None, f1_k=10, _columns=False, diversify=None,
                          similarity="twotower"):
        """Top-`num` fused candidates for each of `users` (TwoTowerModel.
        _query_users' array): device (raw itemIds int64 [n, kk], fused scores
        f64 [n, kk], lens int32 [n] or None when every list is full), kk =
        min(num, candidates). Past a list's length: id 0, score NaN. Users go
        through hrec_hybrid_lists in sub-batches (mode 0); the sub-batches
        whose overflow flag is set — read back once, after the last one — are
        redone in mode 1. With `actual`: _adaptive_device, each user with
        rows there fused by its own two F1@f1_k. _columns (internal): return
        (candidate frame rows int64 [n, kk], scores, lens int32 [n]) instead:
        the lists before the id gather. diversify (optional): a
        ranked_lists.MMR; the top max(pool, num) are ranked as above and
        hrec_mmr_rerank picks num of them, in selection order, with cosines
        between _similarity_vectors(cand, similarity)."""
        num = ranked_lists.check_num(num, self.RECOMMEND_MAX, "num_items")
        f1_k = ranked_lists.check_num(f1_k, self.RECOMMEND_MAX, "f1_k")
        tt = self.twotower_model
        dev = tt.model.device
        n, N = int(users.size), len(cand)
        kk = min(num, N)
        if diversify is not None:
            mmr = ranked_lists.check_mmr(diversify)
            vectors, d = self._similarity_vectors(cand, similarity)
            pool = self._recommend_device(users, cand, max(num, mmr.pool), exclude, actual, f1_k, _columns=True)
            picked = ranked_lists.diversify(*pool, vectors, None, d, mmr, num)
            return ranked_lists.diversify_finish(cand.ids_dev, *picked, N, _columns, exclude is not None)
        if n == 0 or kk == 0:
            return ranked_lists.empty_lists(n, kk, torch.float64, dev, exclude is not None or _columns)
        excl = tt._exclusion(users, cand, exclude) if exclude is not None else None
        fallback = self._als_fallback(users, cand.item_ids)
        als_wins = self.als_f1_score > self.twotower_f1_score
        if actual is not None:
            _, _, idx, val, lens = self._adaptive_device(users, cand, kk, excl, fallback,
                                                         self._labels(users, cand, actual), f1_k, als_wins)
            if _columns:
                return idx, val, lens
            ids, val = ranked_lists.pad_lists(cand.ids_dev, idx, val, lens, N)
            return ids, val, (None if exclude is None else lens)
        rows = torch.arange(n, dtype=torch.int64, device=dev)  # query q reads exclusion row q
        idx = torch.empty((n, kk), dtype=torch.int64, device=dev)
        val = torch.empty((n, kk), dtype=torch.float64, device=dev)
        lens = torch.empty(n, dtype=torch.int32, device=dev)

        def run(s, e, mode):
            a, t = self._scores(users[s:e], cand)
            i, v, m, over = _hrec.hybrid_lists(a, t, kk, als_wins, fallback=fallback,
                                               excl=None if excl is None else (rows[s:e], *excl), mode=mode)
            idx[s:e], val[s:e], lens[s:e] = i, v, m
            return over

        spans = self._spans(0, n, N, 8)
        flagged = torch.cat([run(s, e, 0) for s, e in spans]).tolist()  # one host read
        for (s, e), over in zip(spans, flagged):
            if over:
                for s1, e1 in self._spans(s, e, N, 16):
                    run(s1, e1, 1)
        if _columns:
            return idx, val, lens
        ids, val = ranked_lists.pad_lists(cand.ids_dev, idx, val, lens, N)
        return ids, val, (None if exclude is None else lens)

    def recommend_for_users(self, users, item_features, num_items, exclude=None, actual=None, f1_k=10,
                            diversify=None, similarity="twotower"):
        """Top-n lists of the fused model for many users in one device pass:
        a DataFrame with `userId` (the distinct ids of `users`, ascending; a
        DataFrame with a userId column or an array-like) and `recommendations`:
        the user's top num_items (1 .. 1024) candidates of `item_features` (a
        frame, or TwoTowerModel.candidates()'s object) as (itemId, score)
        tuples, best first. A score is bit for bit the np.float64 that
        adaptive_fusion(als_model.predict_for_user(u, ids), twotower_model.
        predict_for_user(u, frame)) gives that pair over the same frame, with
        the weights als_f1_score / twotower_f1_score choose at call time. The
        ALS score of a pair is transform's f32; where that is NaN (a user or
        an item the ALS model does not know) it is the item's cold-start
        value, ALSModel._cold_scores — when that vector is not available and
        some queried user or candidate is unknown, ValueError. A user id
        outside the two-tower user table raises IndexError.
        exclude (optional): a DataFrame with userId and itemId columns,
        typically the training frame. Both scalers are fitted over ALL
        candidates, excluded ones included (the left-anti join comes after
        the ranking and does not re-scale): each list is the full ranking
        without the excluded pairs, cut to num_items, shorter only when fewer
        entries remain; a user with everything excluded keeps its row with an
        empty list.
        Ties: equal fused scores keep candidate-frame order. The reference
        (and get_hybrid_recommendations) orders them by the iteration order
        of a Python set; the lists do not reproduce that.
        Non-finite scores: a row follows hrec_fuse_topk's arithmetic — NaN is
        ignored by the scalers and a NaN fused score ranks last, in frame
        order; the ValueError the per-user path raises for infinite scores is
        not reproduced. One GPU; models not loaded raise ValueError.
        actual (optional): a DataFrame with userId and itemId columns (other
        columns ignored, repeated pairs counting once, users outside the
        query changing nothing): the known items of some users. A queried
        user with rows there is fused with the weights ITS OWN two F1@f1_k
        choose — what get_hybrid_recommendations(u, items, actual_ratings=
        that user's items) does through evaluate_individual_models: each
        model's own top f1_k (1 .. 1024) over ALL candidates (before and
        independent of `exclude`, as the scalers are) against the user's
        items, those outside the candidate frame counting in recall's
        denominator; (0.8, 0.2) when the ALS F1 is strictly larger, else
        (0.2, 0.8). Every other user keeps the instance's weights. The call
        leaves als_f1_score / twotower_f1_score as they are (the reference
        leaves the last evaluated user's scores there). Within a
        model's top f1_k equal scores keep frame order and NaN scores rank
        last in frame order; for non-finite two-tower scores the reference's
        order is Python's unspecified one and is not reproduced.
        diversify (optional; here and in the methods below): a
        ranked_lists.MMR(lambda_, pool). The fused model ranks max(pool,
        num_items) candidates (after exclude) and greedy Maximal Marginal
        Relevance picks num_items of them, each pick trading its fused score
        (min-max scaled over the pool) against its largest cosine to the picks
        before; similarity chooses the vectors as in list_quality_metrics
        ("twotower": the candidates' item-tower vectors, "als": the ALS item
        factors). The lists are then in SELECTION order, no longer descending
        by score; a tuple keeps the score bits the plain list has for that
        item. None: the plain ranking (similarity is not read)."""
        self._require_models()
        cand = self.twotower_model.candidates(item_features)
        users = self.twotower_model._query_users(users)
        ids, val, lens = self._recommend_device(users, cand, num_items, exclude, actual, f1_k, diversify=diversify,
                                                similarity=similarity)
        return ranked_lists.lists_frame("userId", users, ids, val, lens)

    def recommend_for_all_users(self, item_features, num_items, exclude=None, actual=None, f1_k=10, diversify=None,
                                similarity="twotower"):
        """recommend_for_users for every user of the two-tower user table."""
        self._require_models()
        return self.recommend_for_users(np.arange(int(self.twotower_model.num_users), dtype=np.int64), item_features,
                                        num_items, exclude, actual, f1_k, diversify, similarity)

    def fold_in_users(self, data, item_features, replace=False, **two_tower_kwargs):
        """Fold the users of `data` (userId, itemId, average_review_rating)
        into both models without a refit: ALSModel.fold_in_users(data,
        replace) solves their factor rows against the fixed item factors,
        TwoTowerModel.fold_in_users(data, item_features, **two_tower_kwargs)
        (steps=, learning_rate=) fits their embedding rows with everything
        else frozen. Returns {"als": the ALS call's dict, "twotower": the
        two-tower call's frame}. A folded user has a finite ALS row, so the
        cold-start substitution no longer applies to it and every list and
        metric call personalises both halves. No counterpart in the
        reference: failures raise. The candidates are built (or their stamp
        checked) and the user id range is checked before the ALS call, and a
        ValueError of the ALS call leaves both models as they were."""
        self._require_models()
        item_features = self.twotower_model.candidates(item_features)
        self.twotower_model._fold_in_user_ids(data)
        return {"als": self.als_model.fold_in_users(data, replace=replace),
                "twotower": self.twotower_model.fold_in_users(data, item_features, **two_tower_kwargs)}

    # What the fused lists look like as a whole: ALSModel.list_quality_metrics
    # / evaluate_list_quality for recommend_for_users' lists. No counterpart
    # in the reference: failures raise.
    LIST_QUALITY_METRIC_NAMES = ranked_lists.LIST_QUALITY_NAMES
    LIST_QUALITY_SIMILARITIES = ("twotower", "als")

    def _similarity_vectors(self, cand, similarity):
        """(vectors f32 device [candidates, >= d], d) the cosines are taken between."""
        if similarity not in self.LIST_QUALITY_SIMILARITIES:
            raise ValueError(f"similarity must be one of {', '.join(self.LIST_QUALITY_SIMILARITIES)} "
                             f"(got {similarity!r})")
        if similarity == "twotower":
            return cand.vectors, (int(cand.vectors.shape[1]) if len(cand) else 1)
        m = self.als_model.model
        if m is None:
            raise RuntimeError("the ALS model is not trained or loaded")
        rows = torch.as_tensor(m._lookup(np.asarray(m.item_ids, np.int64), cand.item_ids), device=m.V.device)
        vec = m.V[rows.clamp(min=0)] * (rows >= 0).unsqueeze(1)  # an item the ALS model does not know: the zero vector
        return vec.contiguous(), m.k

    def similar_items(self, item_features, items=None, num=10, min_similarity=None, similarity="twotower"):
        """TwoTowerModel.similar_items over the candidates of `item_features`
        with the cosines of list_quality_metrics' `similarity`: "twotower":
        between the candidates' item-tower vectors; "als": between the ALS
        item factors gathered into candidate order, where an item the ALS
        model does not know is the zero vector: similarity 0.0 to everything.
        Equal similarities keep frame order. No counterpart in the reference:
        failures raise."""
        self._require_models()
        cand = self.twotower_model.candidates(item_features)
        vectors, d = self._similarity_vectors(cand, similarity)
        return ranked_lists.similar_rows_frame("itemId", cand.item_ids, vectors, d, items, num, min_similarity,
                                               ids_dev=cand.ids_dev)

    def list_quality_metrics(self, item_features, k=10, users=None, exclude=None, history=None, actual=None, f1_k=10,
                             similarity="twotower", diversify=None):
        """ALSModel.list_quality_metrics for the fused top-k lists over the
        candidates of `item_features` (recommend_for_users(users,
        item_features, k, exclude, actual, f1_k); users None: every user of
        the two-tower table), still on the device. similarity: "twotower":
        cosines between the candidates' item-tower vectors; "als": between the
        ALS item factors gathered into candidate order, an item the ALS model
        does not know being a zero vector (cosine 0 with everything). history:
        a DataFrame with userId and itemId columns (typically the training
        frame). "dropped" is 0: a user id outside the two-tower table raises
        IndexError, and users the ALS model does not know are served through
        its cold-start values as in recommend_for_users. diversify: the
        measures of recommend_for_users' diversified lists; the selection and
        the measures use the same `similarity` vectors."""
        self._require_models()
        tt = self.twotower_model
        cand = tt.candidates(item_features)
        k = ranked_lists.check_num(k, self.RECOMMEND_MAX, "k")
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        users = tt._query_users(np.arange(int(tt.num_users), dtype=np.int64) if users is None else users)
        dev = tt.model.device
        vectors, d = self._similarity_vectors(cand, similarity)
        hist, tables = tt._history(users, cand, history)

        def batches():
            cols, _, lens = self._recommend_device(users, cand, k, exclude, actual, f1_k, _columns=True,
                                                   diversify=diversify, similarity=similarity)
            rows = torch.arange(int(users.size), dtype=torch.int64, device=dev)  # query q reads history row q
            yield cols, lens, None if hist is None else (rows, *hist)

        res = ranked_lists.list_quality(batches, vectors, d, k, tables)
        res["dropped"] = 0
        return res

    def evaluate_list_quality(self, item_features, metric_name="catalogCoverage", k=10, users=None, exclude=None,
                              history=None, actual=None, f1_k=10, similarity="twotower", diversify=None):
        """One of list_quality_metrics' eight measures (a float)."""
        ranked_lists.check_metric_name(metric_name, self.LIST_QUALITY_METRIC_NAMES)
        return float(self.list_quality_metrics(item_features, k, users, exclude, history, actual, f1_k,
                                               similarity, diversify)[metric_name])

    def evaluate_models(self, data, item_features, k=10):
        """evaluate_individual_models for every user of `data` (columns
        userId, itemId) in one device pass: a DataFrame with `userId` (the
        distinct users of `data`, ascending), `als_f1` and `twotower_f1`
        (float64: compute_f1_score(that user's items, dict(model.
        predict_for_user(u, item_features)), k) bit for bit, ties and NaN as
        in recommend_for_users' `actual`) and `als_wins` (bool: als_f1 >
        twotower_f1). k in 1 .. 1024. The instance's attributes are not
        touched. Unknown ALS ids without a fallback vector raise ValueError, a
        user id outside the two-tower table IndexError."""
        self._require_models()
        k = ranked_lists.check_num(k, self.RECOMMEND_MAX, "k")
        cand = self.twotower_model.candidates(item_features)
        users = self.twotower_model._query_users(data)
        if users.size and len(cand):
            f1, wins, *_ = self._adaptive_device(users, cand, 0, None, self._als_fallback(users, cand.item_ids),
                                                 self._labels(users, cand, data), k, False)
            f1, wins = f1.cpu().numpy(), wins.cpu().numpy() != 0
        else:  # no candidate: every selection is empty
            f1, wins = np.zeros((users.size, 2), np.float64), np.zeros(users.size, bool)
        return pd.DataFrame({"userId": users, "als_f1": f1[:, 0], "twotower_f1": f1[:, 1], "als_wins": wins})

    def fit_fusion_weights(self, data, item_features, k=10):
        """Global weights from a validation frame: sets als_f1_score /
        twotower_f1_score to np.mean of evaluate_models' two columns and
        returns the pair. An empty `data` raises ValueError."""
        scores = self.evaluate_models(data, item_features, k)
        if len(scores) == 0:
            raise ValueError("fit_fusion_weights: `data` holds no user")
        self.als_f1_score = float(np.mean(scores["als_f1"].to_numpy()))
        self.twotower_f1_score = float(np.mean(scores["twotower_f1"].to_numpy()))
        return self.als_f1_score, self.twotower_f1_score

    EVALUATE_MODELS = ("als", "twotower", "hybrid")

    def evaluate_users(self, data, item_features, k_values=(5, 10, 15, 20), ndcg_k=10,
                       models=EVALUATE_MODELS, actual=None, f1_k=10,
                       rating_col="average_review_rating"):
        """The reference's evaluation protocol (RecommenderEvaluator's
        Precision@k / Recall@k, NDCG, MAE, RMSE; reproduce_results.sh loops
        over the test users for it) for every user of `data` (columns userId,
        itemId, rating_col; each pair once, else ValueError) in one device
        pass: {model: DataFrame} for each of `models`, with the columns of
        RecommenderEvaluator.evaluate_scores. A user's row is what the
        per-user methods return for actual = {itemId: rating} of its rows in
        frame order and predicted = dict(als_model.predict_for_user(u, ids)) /
        dict(twotower_model.predict_for_user(u, frame)) / dict(adaptive_fusion
        (those two)) over `item_features`: ALS and fused scores as f64, the
        two-tower's as np.float32. Per sub-batch both models' scores are
        computed once; hrec_hybrid_model_f1 gives each model's own top max(k),
        hrec_hybrid_lists_rowwise the fused lists and scaler extremes, and
        hrec_user_metrics runs once per model; scores and lists stay on the
        device and one host read returns the tables.
        actual / f1_k: as in recommend_for_users — a user with rows in
        `actual` is fused with the weights its own two F1@f1_k choose, every
        other user (all of them without `actual`) with the instance's.
        Cold ALS ids use the cold-start vector; without it they raise
        ValueError, as the lists do. Ties among fused scores keep
        candidate-frame order, not the reference's set order. No exclusion:
        the reference's metrics are taken over all candidates. One GPU."""
        from . import evaluation as ev

        self._require_models()
        ks, ndcg_k = ev.check_k_values(k_values, ndcg_k)
        f1_k = ranked_lists.check_num(f1_k, self.RECOMMEND_MAX, "f1_k")
        models = tuple(models)
        for m in models:
            if m not in self.EVALUATE_MODELS:
                raise ValueError(f"models must be among {self.EVALUATE_MODELS} (got {m!r})")
        tt = self.twotower_model
        dev = tt.model.device
        cand = tt.candidates(item_features)
        users = tt._query_users(data)
        n, N = int(users.size), len(cand)
        if N == 0:
            raise ValueError("evaluate_users: the candidate frame is empty")
        (act_rows, *csr), has_rows = ev.actual_csr_device(data, users, cand.item_ids, rating_col, dev)
        ncol = 2 * len(ks) + 3
        if n == 0 or not models:
            return {m: ev.metrics_frame(users, np.zeros((n, ncol)), np.zeros(n), ks, has_rows) for m in models}
        kmax = max(ks)
        fallback = self._als_fallback(users, cand.item_ids)
        als_wins = self.als_f1_score > self.twotower_f1_score
        labels = self._labels(users, cand, actual) if actual is not None else None
        want_top = "als" in models or "twotower" in models
        want_fused = "hybrid" in models
        out = torch.empty((len(models), n, ncol + 1), dtype=torch.float64, device=dev)

        def run(s, e, mode):
            a, t = self._scores(users[s:e], cand)
            flags, top, wins = [], None, None
            lab = None if labels is None else (labels[0][s:e], *labels[1:])
            if want_fused and lab is not None and f1_k != kmax:  # the weights' own k
                _, wins, over = _hrec.hybrid_model_f1(a, t, f1_k, labels=lab, default_wins=als_wins,
                                                      fallback=fallback, mode=mode)
                flags.append(over)
            if lab is None and not want_top:  # the instance's weights for every row
                wins = torch.full((e - s,), int(als_wins), dtype=torch.int32, device=dev)
            if want_top or (want_fused and wins is None):
                _, w, over, top = _hrec.hybrid_model_f1(a, t, kmax, labels=lab, default_wins=als_wins,
                                                        fallback=fallback, mode=mode, want_top=True)
                wins = w if wins is None else wins
                flags.append(over)
            rows = (act_rows[s:e], *csr)
            if want_fused:
                idx, _, lens, over, mm = _hrec.hybrid_lists_rowwise(a, t, kmax, wins, fallback=fallback, mode=mode,
                                                                    want_minmax=True)
                flags.append(over)
            for i, m in enumerate(models):
                if m == "als":
                    res = _hrec.user_metrics(top[:, 0, :], ks, rows, a, source="als", ndcg_k=ndcg_k,
                                             fallback=fallback)
                elif m == "twotower":
                    res = _hrec.user_metrics(top[:, 1, :], ks, rows, t, source="f32", ndcg_k=ndcg_k)
                else:
                    res = _hrec.user_metrics(idx, ks, rows, a, source="fused", ndcg_k=ndcg_k, list_len=lens, tt=t,
                                             fallback=fallback, minmax=mm, row_wins=wins)
                out[i, s:e, :ncol], out[i, s:e, ncol] = res[0], res[1].double()
            return torch.cat(flags).sum().view(1)

        spans = self._spans(0, n, N, 8)
        flagged = torch.cat([run(s, e, 0) for s, e in spans]).tolist()  # one host read
        for (s, e), over in zip(spans, flagged):
            if over:
                for s1, e1 in self._spans(s, e, N, 16):
                    run(s1, e1, 1)  # mode 1 ranks every key: its flags are always 0
        host = out.cpu().numpy()  # one host read: the per-row tables
        return {m: ev.metrics_frame(users, host[i, :, :ncol], host[i, :, ncol], ks, has_rows)
                for i, m in enumerate(models)}

    def ranking_metrics(self, data, item_features, k=10, label_col=None, min_rating=None, exclude=None, actual=None,
                        f1_k=10, diversify=None, similarity="twotower"):
        """Spark's RankingMetrics (binary relevance) of the fused model's top-k
        lists over `item_features` against `data` (columns userId, itemId):
        the five RANKING_METRIC_NAMES plus "count", with TwoTowerModel.
        ranking_metrics' semantics (ground truth = the user's itemIds in
        `data`, of the rows with label_col >= min_rating when given; each
        metric the mean over the `count` users, NaN when count is 0; each list
        evaluated at its own length). exclude, actual and f1_k as in
        recommend_for_users. The lists go from hrec_hybrid_lists into hrec_ranking_metrics without
        leaving the device. diversify and similarity as in recommend_for_users:
        the metrics of the diversified lists, in selection order."""
        self._require_models()
        tt = self.twotower_model
        cand = tt.candidates(item_features)
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        return ranked_lists.ranking_metrics(
            data, k, label_col, min_rating, tt.model.device, self.RANKING_HOST_ROWS, self.RANKING_METRIC_NAMES,
            lambda users, k: self._recommend_device(tt._query_users(users), cand, k, exclude, actual, f1_k,
                                                    diversify=diversify, similarity=similarity)[::2])

    def evaluate_ranking(self, data, item_features, metric_name="meanAveragePrecision", k=10, label_col=None,
                         min_rating=None, exclude=None, actual=None, f1_k=10, diversify=None, similarity="twotower"):
        """Spark's RankingEvaluator(metricName=metric_name, k=k).evaluate of
        the fused model's lists for the users of `data` (a float)."""
        ranked_lists.check_metric_name(metric_name, self.RANKING_METRIC_NAMES)
        return float(self.ranking_metrics(data, item_features, k, label_col, min_rating, exclude, actual,
                                          f1_k, diversify, similarity)[metric_name])

    # --------------------------------- positions in the full catalogue
    FULL_RANKING_METRIC_NAMES = ranked_lists.FULL_RANK_NAMES

    def _full_rank(self, users, items, weights, cand, exclude):
        """(rank per pair, metrics) of ranked_lists.full_rank_metrics over the
        fused scores: per sub-batch both score matrices, the scaler extremes
        from the hrec_hybrid_lists call the list path makes (top_k 1: only its
        out_minmax is used), then hrec_rank_positions' fused source with the
        instance's weights in every row."""
        tt = self.twotower_model
        dev = tt.model.device
        queried = tt._query_users(users)  # an id outside the user table: IndexError
        N = len(cand)
        if queried.size == 0 or N == 0:
            return ranked_lists.full_rank_metrics(users, items, weights, cand.item_ids, dev, None, 8, 1)
        excl = tt._exclusion(queried, cand, exclude) if exclude is not None else None
        fallback = self._als_fallback(queried, cand.item_ids)
        als_wins = self.als_f1_score > self.twotower_f1_score

        def scores(uids):
            a, t = self._scores(uids, cand)
            *_, mm = _hrec.hybrid_lists(a, t, 1, als_wins, fallback=fallback, mode=0, want_minmax=True)
            kw = dict(scores=a, source="fused", tt=t, fallback=fallback, minmax=mm,
                      row_wins=torch.full((uids.size,), int(als_wins), dtype=torch.int32, device=dev))
            if excl is not None:  # exclusion row q is queried[q]
                kw["excl"] = (torch.as_tensor(np.searchsorted(queried, uids), device=dev), *excl)
            return kw

        return ranked_lists.full_rank_metrics(users, items, weights, cand.item_ids, dev, scores, 8,
                                              self.RECOMMEND_SCORE_BYTES, max_rows=self.RECOMMEND_ROWS,
                                              host_rows=self.RANKING_HOST_ROWS)

    def rank_of(self, data, item_features, exclude=None):
        """A copy of `data` (columns userId, itemId) with an int64 `rank`
        column: the 0-based position of the row's item among ALL candidates of
        `item_features` in the user's fused ranking (recommend_for_users'
        scores, weights and ties: equal fused scores in frame order, NaN last)
        without the pairs of `exclude`. For any n <= 1024, rank < n holds
        exactly when the item stands at position rank of the user's list from
        recommend_for_users(users, item_features, n, exclude). -1: the item is
        not a candidate, or the pair is excluded. The scalers are fitted over
        all candidates, as for the lists; cold ALS ids use the cold-start
        vector (ValueError without it). Every user is fused with the
        instance's weights: the per-user `actual=` weights of
        recommend_for_users are not part of these methods."""
        self._require_models()
        cand = self.twotower_model.candidates(item_features)
        users = ranked_lists.int_ids(data["userId"], "userId")
        items = ranked_lists.int_ids(data["itemId"], "itemId")
        rank, _ = self._full_rank(users, items, None, cand, exclude)
        return ranked_lists.rank_frame(data, rank)

    def full_ranking_metrics(self, data, item_features, weight_col=None, min_rating=None, label_col=None,
                             exclude=None):
        """ALSModel.full_ranking_metrics of the fused model over the
        candidates of `item_features`: {"meanPercentileRank", "auc",
        "meanReciprocalRank", "count", "pairs", "unranked", "dropped"} of the
        pairs of `data` among ALL candidates, ranked as rank_of ranks them
        (ties in frame order, not counted as 1/2). `dropped` is 0. The
        instance's weights for every user; per-user `actual=` weights are not
        part of these methods."""
        self._require_models()
        cand = self.twotower_model.candidates(item_features)
        users, items, weights = ranked_lists.full_rank_frame(data, weight_col, min_rating, label_col)
        _, res = self._full_rank(users, items, weights, cand, exclude)
        res["dropped"] = 0
        return res

    def evaluate_full_ranking(self, data, item_features, metric_name="meanPercentileRank", weight_col=None,
                              min_rating=None, label_col=None, exclude=None):
        """One of full_ranking_metrics' meanPercentileRank, auc,
        meanReciprocalRank (a float)."""
        ranked_lists.check_metric_name(metric_name, self.FULL_RANKING_METRIC_NAMES)
        return float(self.full_ranking_metrics(data, item_features, weight_col, min_rating, label_col,
                                               exclude)[metric_name])

    def cleanup(self):
        if self.als_model:
            self.als_model.stop_spark()
