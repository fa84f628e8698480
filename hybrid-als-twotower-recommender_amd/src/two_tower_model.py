"""Two-tower content model — drop-in for the reference's src/two_tower_model.py.

Same class, methods, arguments and return values as src/two_tower_model.py:17-245.
The Keras graph (:38-89), `model.fit` (:111) and `model.predict` (:145) are
replaced by the device engine in tt_engine.py (hrec_tt_* / hrec_adam_* HIP
kernels). Host-side feature assembly (_prepare_features, the MinMaxScaler on
[price, average_review_rating]) is kept exactly, including the scaler refit
on every _prepare_features call.

Not in the reference (failures raise): recommend_for_users /
recommend_for_all_users (top-n lists for many users in one device pass, with
an optional seen-item exclusion), ranking_metrics / evaluate_ranking (Spark's
five ranking metrics of those lists against a held-out frame) and candidates
(the item tower's vectors of a frame, computed once) — hrec_dot_topk /
hrec_dot_topk_excluding at widths 32 / 64 / 128 / 256, the materialised
hrec_tt_score chain at any other width. Likewise transform /
regression_metrics / evaluate: the prediction of every row of a frame and the
regression metrics of a split, over hrec_tt_predict_pairs /
hrec_tt_pair_metrics.

Deviations from the committed reference (documented in DESIGN.md):
  * `if val_data:` on a DataFrame raises in the reference (D5); here
    val_data is tested with `is not None`, so EarlyStopping(patience=3,
    restore_best_weights=True) on val_loss works as the code intends. The
    ModelCheckpoint('tmp_best.keras') file is not written.
  * load_model's missing Keras import (D3) is not reproduced.
  * ids go through float32 like Keras Input(shape=(1,)) (D11) and must then
    index inside the tables (Keras raises there too).
"""
import os
import pickle

import numpy as np
import pandas as pd
import torch
from sklearn.model_selection import train_test_split  # noqa: F401  (reference import surface)
from sklearn.preprocessing import MinMaxScaler

from . import _hrec, pair_metrics, ranked_lists
from .als_model import _int_ids
from .tt_engine import TABLES, DeviceTwoTower


class TwoTowerCandidates:
    """A candidate frame on the device (TwoTowerModel.candidates): item_ids
    (numpy int64, frame order) and ids_dev (the same on the device), vectors
    (f32 device [n, d], the item tower's outputs), and the stamp of the
    weights they were built from: the engine object, its `iterations`, and
    the fitted scaler's parameters (scale_, min_) the numeric inputs went
    through."""

    def __init__(self, item_ids, ids_dev, vectors, engine, iterations, scaler_stamp=None):
        self.item_ids = item_ids
        self.ids_dev = ids_dev
        self.vectors = vectors
        self.engine = engine
        self.iterations = int(iterations)
        self.scaler_stamp = scaler_stamp
        self._sorted = None  # (ids ascending, their frame rows), built by the first rows_of

    def __len__(self):
        return int(self.item_ids.size)

    def rows_of(self, item_ids):
        """Frame rows (int64 device [n]) of a device int64 id list: a binary
        search over the frame's sorted (distinct) ids; -1 for an id the frame
        does not hold."""
        if len(self) == 0:
            return torch.full_like(item_ids, -1)
        if self._sorted is None:
            self._sorted = torch.sort(self.ids_dev)
        sid, order = self._sorted
        pos = torch.searchsorted(sid, item_ids).clamp_(max=sid.numel() - 1)
        return torch.where(sid[pos] == item_ids, order[pos], torch.full_like(item_ids, -1))


class History:
    """The subset of keras.callbacks.History the reference touches."""

    def __init__(self):
        self.history = {}
        self.epoch = []


def _ids(values, n, name):
    """Keras Input(shape=(1,)) is float32; Embedding casts to int32 (D11)."""
    a = np.asarray(values).astype(np.float32).astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{name}: id out of range [0, {n})")
    return a.astype(np.int32)


def _minmax_transform(scaler, frame, cols):
    """scaler.transform(frame[cols]) (:143). For a fitted MinMaxScaler over
    plain int / float64 columns this is sklearn's own arithmetic on a float64
    copy (X *= scale_; X += min_, sklearn/preprocessing/_data.py) without its
    per-call validation overhead (~2 ms per 100k rows); anything else — other
    scalers, clip, float32 or object columns, non-finite values, name or width
    mismatches — goes through scaler.transform itself."""
    sub = frame[cols]
    names = getattr(scaler, "feature_names_in_", None)
    if (type(scaler) is not MinMaxScaler or scaler.clip or not hasattr(scaler, "scale_") or len(sub) == 0
            or getattr(scaler, "n_features_in_", None) != len(cols)
            or (names is not None and list(names) != list(cols))
            or not all(dt == np.float64 or (dt.kind in "iu" and dt != np.bool_) for dt in sub.dtypes)):
        return scaler.transform(sub)
    X = sub.to_numpy(dtype=np.float64, copy=True)
    if np.isinf(X).any():
        return scaler.transform(sub)  # sklearn's own error
    X *= scaler.scale_
    X += scaler.min_
    return X


class TwoTowerModel:
    """Two-Tower Model Architecture (src/two_tower_model.py:17-36)."""

    def __init__(self, num_users, num_items, num_manufacturers, num_categories,
                 embedding_size=50, learning_rate=0.001, seed=0):
        self.num_users = num_users
        self.num_items = num_items
        self.num_manufacturers = num_manufacturers
        self.num_categories = num_categories
        self.embedding_size = embedding_size
        self.learning_rate = learning_rate
        self.model = None
        self.scaler = MinMaxScaler()
        self.is_trained = False
        self.seed = seed
        self._inputs_ws = None  # hrec_tt_item_inputs' presence bitmap, reused across calls

    def _build_item_tower(self):
        """(:38-66) -> (inputs, item_vec) as the reference returns them: the
        four inputs by their Input-layer names, and the tower itself —
        item_vec = LN(Dense(d)(concat[E_item, E_man(8), E_cat(8),
        relu(Dense(16)(numeric))])) — as a function of those inputs on the
        device (K4, csrc/tt_mfma.hip; the parameters build_model allocates)."""
        inputs = ["item_id_in", "manufacturer_in", "category_in", "numeric_in"]

        def item_vec(item_id_in, manufacturer_in, category_in, numeric_in):
            if self.model is None:
                raise RuntimeError("item tower: call build_model() first (it owns the tower's weights)")
            dev, sz = self.model.device, self.model.sizes
            ids = [torch.as_tensor(_ids(x, sz[t], name), device=dev)
                   for x, t, name in ((item_id_in, "item_emb", "item_id_in"), (manufacturer_in, "man_emb", "manufacturer_in"),
                                      (category_in, "cat_emb", "category_in"))]
            num = np.ascontiguousarray(np.asarray(numeric_in, dtype=np.float32).reshape(-1, 2))
            return self.model.item_vectors(*ids, torch.as_tensor(num, device=dev))

        return inputs, item_vec

    def build_model(self, init=None):
        """Allocate the parameters (Keras initialisers) on the device (:68-89)."""
        self.model = DeviceTwoTower(self.num_users, self.num_items, self.num_manufacturers, self.num_categories,
                                    self.embedding_size, self.learning_rate, seed=self.seed, init=init)
        return self.model

    # ------------------------------------------------------------ features
    def _prepare_features(self, data):
        if data is None:
            return None
        return {
            "user_in": data["userId"].values,
            "item_id_in": data["itemId"].values,
            "manufacturer_in": data["manufacturer_id"].values,
            "category_in": data["category_id"].values,
            "numeric_in": self.scaler.fit_transform(data[["price", "average_review_rating"]]),
        }

    def _device_inputs(self, feats):
        dev = self.model.device
        sz = self.model.sizes
        return (torch.as_tensor(_ids(feats["user_in"], sz["user_emb"], "user_in"), device=dev),
                torch.as_tensor(_ids(feats["item_id_in"], sz["item_emb"], "item_id_in"), device=dev),
                torch.as_tensor(_ids(feats["manufacturer_in"], sz["man_emb"], "manufacturer_in"), device=dev),
                torch.as_tensor(_ids(feats["category_in"], sz["cat_emb"], "category_in"), device=dev),
                torch.as_tensor(np.ascontiguousarray(np.asarray(feats["numeric_in"], dtype=np.float32).reshape(-1, 2)), device=dev))

    # --------------------------------------------------------------- train
    def _evaluate_loss(self, dev_inputs, y):
        pred = self.model.predict_rows(*dev_inputs).cpu().numpy()
        e = pred - y.cpu().numpy()
        return float(np.mean(e * e))

    def fit_batches(self, dev_inputs, y, batches):
        """Run train steps over explicit index batches (one Keras epoch with a
        given shuffle order); returns (sum_sq_err, sum_abs_err) over the epoch."""
        stats = []
        for idx in batches:
            idx_t = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=self.model.device)
            parts = [t.index_select(0, idx_t).contiguous() for t in dev_inputs]  # batch assembly
            stats.append(self.model.train_step(*parts, y.index_select(0, idx_t).contiguous()))
        if not stats:
            return 0.0, 0.0
        st = torch.stack(stats).cpu().numpy().astype(np.float64)
        return float(st[:, 0].sum()), float(st[:, 1].sum())

    def train(self, train_data, val_data=None, batch_size=256, epochs=10, shuffle_seed=None):
        """Training process with early stopping (:91-121)."""
        if self.model is None:
            self.build_model()
        train_features = self._prepare_features(train_data)
        val_features = self._prepare_features(val_data) if val_data is not None else None
        dev_in = self._device_inputs(train_features)
        y = torch.as_tensor(np.asarray(train_data["average_review_rating"], dtype=np.float32),
                            device=self.model.device)
        if val_features is not None:
            val_in = self._device_inputs(val_features)
            val_y = torch.as_tensor(np.asarray(val_data["average_review_rating"], dtype=np.float32),
                                    device=self.model.device)
        n = len(y)
        rng = np.random.default_rng(self.seed if shuffle_seed is None else shuffle_seed)
        history = History()
        best, best_snap, wait = np.inf, None, 0
        for epoch in range(int(epochs)):
            order = rng.permutation(n)  # Keras fit(shuffle=True)
            batches = [order[s: s + batch_size] for s in range(0, n, batch_size)]
            sq, ab = self.fit_batches(dev_in, y, batches)
            history.epoch.append(epoch)
            history.history.setdefault("loss", []).append(sq / n)
            history.history.setdefault("mae", []).append(ab / n)
            if val_features is not None:
                vl = self._evaluate_loss(val_in, val_y)
                history.history.setdefault("val_loss", []).append(vl)
                # EarlyStopping(monitor='val_loss', patience=3, restore_best_weights=True)
                if vl < best:
                    best, best_snap, wait = vl, self.model.snapshot(), 0
                else:
                    wait += 1
                    if wait >= 3:
                        if best_snap is not None:
                            self.model.restore(best_snap)
                        break
        self.is_trained = True
        return history

    # ------------------------------------------------------------- predict
    def predict_for_user(self, user_id, item_features):
        """Generate predictions for one user over candidate rows (:136-146)."""
        scored = self._predict_device(user_id, item_features)
        return self._predictions(*scored) if scored else []

    def _score_device(self, inputs):
        """model.predict on the assembled inputs: f32 device scores [n]."""
        dev_in = self._device_inputs(inputs)
        u = dev_in[0][:1]
        uvec = self.model.user_vectors(u)
        ivec = self.model.item_vectors(*dev_in[1:])
        return _hrec.tt_score(uvec, ivec).reshape(-1)

    @staticmethod
    def _predictions(item_features, scores):
        predictions = scores.cpu().numpy().reshape(-1, 1)
        col = item_features["itemId"]
        # iterating a numpy-backed Series yields values.item(i), which is
        # what ndarray.tolist() builds in one call (same objects and types)
        keys = col.to_numpy().tolist() if isinstance(col.array, pd.arrays.NumpyExtensionArray) else col
        return list(zip(keys, predictions.flatten()))

    def _predict_device(self, user_id, item_features):
        """For HybridRecommendationSystem's array path: predict_for_user up to
        the device scores, (item_features, f32 device scores [n]); [] for an
        empty frame. Raises where predict_for_user raises."""
        inputs = {
            # the reference's np.full(len(item_features), user_id) column holds
            # one id n times, and one user vector serves every row
            # (_score_device): that id alone is converted and range-checked
            # (the same cast, the same error) and sent to the device
            "user_in": np.full(1, user_id),
            "item_id_in": item_features["itemId"].values,
            "manufacturer_in": item_features["manufacturer_id"].values,
            "category_in": item_features["category_id"].values,
            "numeric_in": _minmax_transform(self.scaler, item_features, ["price", "average_review_rating"]),
        }
        if len(item_features) == 0:
            return []
        return item_features, self._score_device(inputs)

    _FAST_ID_COLS = ("itemId", "manufacturer_id", "category_id")
    _FAST_NUM_COLS = ("price", "average_review_rating")

    def _predict_device_fast(self, user_id, item_features):
        """_predict_device for a plain candidate frame with the item-side
        input work on the device (hrec_tt_item_inputs: id casts and range
        checks, the MinMaxScaler transform, the candidates' uniqueness):
        (item_features, f32 device scores [n], device flags int32 [1]), or
        None when the frame or scaler is outside that path. Non-zero flags
        mean the inputs are NOT the model's (an id out of range, an infinite
        value, a repeated item id): the caller redoes the call through
        _predict_device, which raises where predict_for_user raises. The user
        id is checked here, on the host, first — as _device_inputs does."""
        sc = self.scaler
        if (self.model is None or type(sc) is not MinMaxScaler
                or sc.clip or not hasattr(sc, "scale_") or getattr(sc, "n_features_in_", None) != 2):
            return None
        names = getattr(sc, "feature_names_in_", None)
        if names is not None and list(names) != list(self._FAST_NUM_COLS):
            return None
        series = self._fast_columns(item_features)
        if series is None:
            return None
        n = len(item_features)
        cols = []
        for c, s in zip(self._FAST_ID_COLS + self._FAST_NUM_COLS, series):
            a = s.to_numpy()
            if not isinstance(a, np.ndarray) or a.ndim != 1 or len(a) != n:
                return None
            if c in self._FAST_ID_COLS:
                if a.dtype.kind not in "iu" or a.dtype == np.uint64:
                    return None
                a = a.astype(np.int64, copy=False)
            else:  # to_numpy(dtype=float64) of _minmax_transform: floats as they are, ints converted
                if not (a.dtype == np.float64 or (a.dtype.kind in "iu" and a.dtype != np.bool_)):
                    return None
                a = a.astype(np.float64, copy=False)
            cols.append(np.ascontiguousarray(a))
        dev, sz = self.model.device, self.model.sizes
        u = torch.as_tensor(_ids(np.full(1, user_id), sz["user_emb"], "user_in"), device=dev)
        t = [torch.from_numpy(a).to(dev) for a in cols]
        item, man, cat, num, flags, self._inputs_ws = _hrec.tt_item_inputs(
            *t, (sz["item_emb"], sz["man_emb"], sz["cat_emb"]), sc.scale_, sc.min_, self._inputs_ws)
        uvec = self.model.user_vectors(u)
        ivec = self.model.item_vectors(item, man, cat, num)
        return item_features, _hrec.tt_score(uvec, ivec).reshape(-1), flags

    def _fast_columns(self, item_features):
        """The five Series _predict_device reads, through the same lookups
        (frame["col"] for the ids, frame[[price, rating]] for the scaler), or
        None: an empty candidate set, a missing or repeated column, or a
        lookup that is not a plain Series. Besides a DataFrame this takes any
        candidates object answering those lookups from a frame (e.g. an item
        id array whose ["col"] comes from the item frame, bench.py)."""
        try:
            if len(item_features) == 0:
                return None
            if isinstance(item_features, pd.DataFrame):
                if not item_features.columns.is_unique or not all(
                        c in item_features.columns for c in self._FAST_ID_COLS + self._FAST_NUM_COLS):
                    return None
                return [item_features[c] for c in self._FAST_ID_COLS + self._FAST_NUM_COLS]
            ids = [item_features[c] for c in self._FAST_ID_COLS]
            sub = item_features[list(self._FAST_NUM_COLS)]
        except Exception:  # the host path makes the same lookups and reports the error
            return None
        if (not isinstance(sub, pd.DataFrame) or list(sub.columns) != list(self._FAST_NUM_COLS)
                or not all(type(s) is pd.Series for s in ids)):
            return None
        return ids + [sub[c] for c in self._FAST_NUM_COLS]

    # ------------------------------------- batch top-n lists / ranking metrics
    # None of these has a counterpart in the reference: failures raise.
    # Scoring route, by embedding_size d:
    #   d in {32, 64, 128, 256}: the fused matrix-core top-k over f32 operands,
    #     hrec_dot_topk (no exclusion) / hrec_dot_topk_excluding — its f32
    #     scores are hrec_tt_score's fmaf chain in the same k order, i.e. the
    #     bits predict_for_user gives;
    #   any other d (the constructor default 50 among them): hrec_tt_score ->
    #     hrec_mask_rows_f32 -> hrec_topk_f32 over materialised scores, in user
    #     sub-batches of at most RECOMMEND_FALLBACK_BYTES — hrec_tt_score adds
    #     those widths in the order k = 0 .. d-1, which the zero-padded
    #     matrix-core operand would not reproduce.
    RECOMMEND_MAX = 1024                 # largest list length (the library's top_k limit)
    RECOMMEND_FALLBACK_BYTES = 1 << 30   # a materialised score matrix stays under this (per sub-batch)
    EXCLUSION_HOST_PAIRS = 1 << 16       # exclusion lists up to this many pairs are built on the host
    RANKING_HOST_ROWS = 1 << 16          # frames up to this many rows: the label CSR is built on the host
    RANKING_METRIC_NAMES = ("meanAveragePrecision", "meanAveragePrecisionAtK", "precisionAtK", "recallAtK",
                            "ndcgAtK")

    def candidates(self, item_features):
        """The candidate frame on the device, for the methods below: its
        itemId column (int64, frame order), the item tower's f32 vectors and a
        stamp of the weights they come from. The item inputs are assembled as
        predict_for_user assembles them (_ids, the fitted scaler's transform),
        over the whole frame in one item_vectors call, so the vectors are bit
        for bit those predict_for_user(u, item_features) scores with. Repeated
        itemIds raise ValueError. Passing a TwoTowerCandidates checks its stamp
        and returns it: RuntimeError after the weights moved on (a training
        step) or the scaler was refitted to other parameters (_prepare_features
        refits it on every call), since predict_for_user would then score
        other vectors."""
        if self.model is None:
            raise RuntimeError("the two-tower model is not built or loaded")
        if isinstance(item_features, TwoTowerCandidates):
            if (item_features.engine is not self.model or item_features.iterations != self.model.iterations
                    or item_features.scaler_stamp != self._scaler_stamp()):
                raise RuntimeError("candidates: built from other weights or another scaler fit than the model holds "
                                   "now; build them again")
            return item_features
        ids = _int_ids(item_features["itemId"], "itemId")
        if np.unique(ids).size != ids.size:
            raise ValueError("candidates: the frame repeats an itemId")
        dev, sz = self.model.device, self.model.sizes
        if ids.size == 0:
            vec = torch.empty((0, int(self.embedding_size)), dtype=torch.float32, device=dev)
        else:
            num = _minmax_transform(self.scaler, item_features, ["price", "average_review_rating"])
            vec = self.model.item_vectors(
                torch.as_tensor(_ids(item_features["itemId"].values, sz["item_emb"], "item_id_in"), device=dev),
                torch.as_tensor(_ids(item_features["manufacturer_id"].values, sz["man_emb"], "manufacturer_in"),
                                device=dev),
                torch.as_tensor(_ids(item_features["category_id"].values, sz["cat_emb"], "category_in"), device=dev),
                torch.as_tensor(np.ascontiguousarray(np.asarray(num, dtype=np.float32).reshape(-1, 2)), device=dev))
        return TwoTowerCandidates(ids, torch.as_tensor(ids, device=dev), vec, self.model, self.model.iterations,
                                  self._scaler_stamp())

    def _scaler_stamp(self):
        """The fitted scaler's parameters as bytes (None before a fit)."""
        sc = self.scaler
        if not hasattr(sc, "scale_") or not hasattr(sc, "min_"):
            return None
        return (np.asarray(sc.scale_, np.float64).tobytes(), np.asarray(sc.min_, np.float64).tobytes())

    def _exclusion(self, users, cand, exclude):
        """The device exclusion CSR of an `exclude` frame (columns userId,
        itemId): row q is the queried users[q] (ascending, distinct), the
        columns are candidate FRAME ROW indices (the frame holds its itemIds
        in any order). Pairs with a user outside `users` or an item outside
        the frame are dropped."""
        eu, ei = _int_ids(exclude["userId"], "userId"), _int_ids(exclude["itemId"], "itemId")
        return ranked_lists.exclusion_csr(users, cand.item_ids, eu, ei, self.model.device, self.EXCLUSION_HOST_PAIRS,
                                          what="exclude: userId and itemId")

    def _query_users(self, users):
        """The distinct user ids, ascending (int64); an id outside the user
        table raises _ids's IndexError."""
        if isinstance(users, pd.DataFrame):
            users = users["userId"]
        if self.model is None:
            raise RuntimeError("the two-tower model is not built or loaded")
        return np.unique(_ids(np.asarray(users).reshape(-1), self.model.sizes["user_emb"], "user_in").astype(np.int64))

    def _recommend_device(self, users, cand, num, exclude=None, _columns=False, diversify=None):
        """Top-`num` candidates for each of `users` (_query_users' array):
        device (raw itemIds int64 [n, kk], scores f32 [n, kk], lens int32 [n]
        or None when every list is full), kk = min(num, candidates). Past a
        list's length: id 0, score NaN. _columns (internal): return (candidate
        frame rows int64 [n, kk], scores, lens or None) instead: the lists
        before the id gather. diversify (optional): a ranked_lists.MMR; the top
        max(pool, num) are ranked as above and hrec_mmr_rerank picks num of
        them (cosines between the candidates' vectors), in selection order."""
        num = ranked_lists.check_num(num, self.RECOMMEND_MAX, "num_items")
        dev = self.model.device
        n, N = int(users.size), int(cand.vectors.shape[0])
        kk = min(num, N)
        if diversify is not None:
            mmr = ranked_lists.check_mmr(diversify)
            pool = self._recommend_device(users, cand, max(num, mmr.pool), exclude, _columns=True)
            picked = ranked_lists.diversify(*pool, cand.vectors, None, int(cand.vectors.shape[1]) if N else 1, mmr,
                                            num)
            return ranked_lists.diversify_finish(cand.ids_dev, *picked, N, _columns, exclude is not None)
        if n == 0 or kk == 0:
            empty = ranked_lists.empty_lists(n, kk, torch.float32, dev, exclude is not None)
            return empty
        excl = self._exclusion(users, cand, exclude) if exclude is not None else None
        U = self.model.user_vectors(torch.as_tensor(users.astype(np.int32), device=dev))
        V = cand.vectors
        rows = torch.arange(n, dtype=torch.int64, device=dev)  # query q reads exclusion row q
        lens = None
        if int(self.embedding_size) in _hrec.DOT_DK:
            if excl is None:
                idx, val = _hrec.dot_topk(U, V, kk)
            else:
                idx, val, lens = _hrec.dot_topk_excluding(U, V, kk, rows, *excl)
        else:
            idx = torch.empty((n, kk), dtype=torch.int64, device=dev)
            val = torch.empty((n, kk), dtype=torch.float32, device=dev)
            lens = None if excl is None else torch.empty(n, dtype=torch.int32, device=dev)
            _hrec.topk_materialised(lambda s, e: _hrec.tt_score(U[s:e].contiguous(), V), 0, n, N, kk,
                                    self.RECOMMEND_FALLBACK_BYTES, idx, val, lens,
                                    None if excl is None else (rows, *excl))
        if _columns:
            return idx, val, lens
        if lens is None:
            return cand.ids_dev[idx], val, None
        return (*ranked_lists.pad_lists(cand.ids_dev, idx, val, lens, N), lens)

    def recommend_for_users(self, users, item_features, num_items, exclude=None, diversify=None):
        """Top-n lists for many users in one device pass: a DataFrame with
        `userId` (the distinct ids of `users`, ascending; a DataFrame with a
        userId column or an array-like) and `recommendations`: the user's top
        num_items (1 .. 1024) candidates of `item_features` (a frame, or
        candidates()'s object) as (itemId, rating) tuples, best first. A rating
        is the f32 predict_for_user gives that pair over the same frame; equal
        ratings keep frame order (what Python's stable sorted(...,
        reverse=True) gives predict_for_user's list). A user id outside [0,
        num_users) raises IndexError.
        exclude (optional): a DataFrame with userId and itemId columns,
        typically the training frame. Its pairs never appear: each list is the
        full ranking without them, cut to num_items, shorter only when fewer
        entries remain; a user with everything excluded keeps its row with an
        empty list. Pairs with a user outside the table or an item not in the
        candidate frame, and repeated pairs, change nothing.
        embedding_size 32 / 64 / 128 / 256 takes the fused matrix-core top-k
        (hrec_dot_topk / hrec_dot_topk_excluding); any other width, the
        default 50 included, the materialised hrec_tt_score chain (see the
        note above).
        diversify (optional; here and in the methods below): a
        ranked_lists.MMR(lambda_, pool). The model ranks max(pool, num_items)
        candidates (after exclude) and greedy Maximal Marginal Relevance picks
        num_items of them, each pick trading its rating (min-max scaled over
        the pool) against its largest cosine, between the candidates'
        item-tower vectors, to the picks before. The lists are then in
        SELECTION order, no longer descending by rating; a tuple keeps the
        rating bits the plain list has for that item. None: the plain ranking."""
        cand = self.candidates(item_features)
        users = self._query_users(users)
        ids, val, lens = self._recommend_device(users, cand, num_items, exclude, diversify=diversify)
        return ranked_lists.lists_frame("userId", users, ids, val, lens)

    def recommend_for_all_users(self, item_features, num_items, exclude=None, diversify=None):
        """recommend_for_users for users 0 .. num_users - 1."""
        return self.recommend_for_users(np.arange(int(self.num_users), dtype=np.int64), item_features, num_items,
                                        exclude, diversify)

    def similar_items(self, item_features, items=None, num=10, min_similarity=None):
        """implicit's similar_items over a candidate frame (or candidates()'s
        object): a DataFrame with `itemId` (None: every candidate, in frame
        order; a DataFrame with an itemId column or an array-like otherwise:
        its distinct ids ascending, those outside the frame left out) and
        `recommendations`: the `num` (1 .. 1024) nearest other candidates by
        the cosine between item-tower vectors, as (itemId, similarity: float)
        tuples, best first. Equal similarities keep frame order; the item
        itself never appears; min_similarity (None: no cut) keeps the
        similarities above it. Any embedding_size up to 256 (the default 50
        included) goes through hrec_cosine_topk; the same bits on every call."""
        cand = self.candidates(item_features)
        d = int(cand.vectors.shape[1]) if len(cand) else 1
        return ranked_lists.similar_rows_frame("itemId", cand.item_ids, cand.vectors, d, items, num, min_similarity,
                                               ids_dev=cand.ids_dev)

    def ranking_metrics(self, data, item_features, k=10, label_col=None, min_rating=None, exclude=None,
                        diversify=None):
        """Spark's RankingMetrics (binary relevance) of the model's top-k
        lists over `item_features` against `data` (columns userId, itemId):
        ALSModel.RANKING_METRIC_NAMES' five metrics plus "count", with
        ALSModel.ranking_metrics' semantics. A user's ground truth is the set
        of its itemIds in `data` — with min_rating, of the rows whose
        label_col (default average_review_rating) is >= min_rating; a user
        left with no row does not appear. Items absent from the candidate
        frame stay in the set: never hit, counted in its size. Each metric is
        the mean over the `count` users (NaN when count is 0). exclude as in
        recommend_for_users; each list is evaluated at its own length. A user
        id outside the table raises IndexError. The lists go from the top-k
        into hrec_ranking_metrics without leaving the device. diversify: the
        metrics of recommend_for_users' diversified lists, in selection order."""
        cand = self.candidates(item_features)
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        return ranked_lists.ranking_metrics(
            data, k, label_col, min_rating, self.model.device, self.RANKING_HOST_ROWS, self.RANKING_METRIC_NAMES,
            lambda users, k: self._recommend_device(self._query_users(users), cand, k, exclude,
                                                    diversify=diversify)[::2])  # IndexError

    def evaluate_ranking(self, data, item_features, metric_name="meanAveragePrecision", k=10, label_col=None,
                         min_rating=None, exclude=None, diversify=None):
        """Spark's RankingEvaluator(metricName=metric_name, k=k).evaluate of
        the model's lists for the users of `data` (a float)."""
        ranked_lists.check_metric_name(metric_name, self.RANKING_METRIC_NAMES)
        return float(self.ranking_metrics(data, item_features, k, label_col, min_rating, exclude,
                                          diversify)[metric_name])

    # ------------------------------------------------------------ list quality
    # ALSModel.list_quality_metrics / evaluate_list_quality over a candidate
    # frame. No counterpart in the reference: failures raise.
    LIST_QUALITY_METRIC_NAMES = ranked_lists.LIST_QUALITY_NAMES

    def _history(self, users, cand, history):
        """(the queried users' history CSR: _exclusion's, the frame's two
        tables) of a history frame, (None, None) without one."""
        if history is None or len(cand) == 0:
            return None, None
        return (self._exclusion(users, cand, history),
                ranked_lists.history_tables(*ranked_lists.history_frame(history), cand.item_ids, self.model.device))

    def list_quality_metrics(self, item_features, k=10, users=None, exclude=None, history=None, diversify=None):
        """ALSModel.list_quality_metrics for the model's top-k lists over the
        candidates of `item_features` (recommend_for_users(users,
        item_features, k, exclude); users None: every user of the table), still
        on the device. Cosines are taken between the candidates' item-tower
        vectors (TwoTowerCandidates.vectors). history: a DataFrame with userId
        and itemId columns (typically the training frame); its items outside
        the candidate frame enter nothing. The model has no coldStartStrategy:
        "dropped" is 0 and a user id outside the table raises IndexError.
        diversify: the measures of recommend_for_users' diversified lists."""
        cand = self.candidates(item_features)
        k = ranked_lists.check_num(k, self.RECOMMEND_MAX, "k")
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        users = self._query_users(np.arange(int(self.num_users), dtype=np.int64) if users is None else users)
        dev = self.model.device
        hist, tables = self._history(users, cand, history)

        def batches():
            cols, _, lens = self._recommend_device(users, cand, k, exclude, _columns=True, diversify=diversify)
            rows = torch.arange(int(users.size), dtype=torch.int64, device=dev)  # query q reads history row q
            yield cols, lens, None if hist is None else (rows, *hist)

        res = ranked_lists.list_quality(batches, cand.vectors, int(cand.vectors.shape[1]) if len(cand) else 1, k,
                                        tables)
        res["dropped"] = 0
        return res

    def evaluate_list_quality(self, item_features, metric_name="catalogCoverage", k=10, users=None, exclude=None,
                              history=None, diversify=None):
        """One of list_quality_metrics' eight measures (a float)."""
        ranked_lists.check_metric_name(metric_name, self.LIST_QUALITY_METRIC_NAMES)
        return float(self.list_quality_metrics(item_features, k, users, exclude, history, diversify)[metric_name])

    # --------------------------------- positions in the full catalogue
    # ALSModel.rank_of / full_ranking_metrics / evaluate_full_ranking over a
    # candidate frame. No counterpart in the reference: failures raise.
    FULL_RANKING_METRIC_NAMES = ranked_lists.FULL_RANK_NAMES

    def _full_rank(self, users, items, weights, cand, exclude):
        """(rank per pair, metrics) of ranked_lists.full_rank_metrics over the candidate frame."""
        dev = self.model.device
        queried = self._query_users(users)  # an id outside the user table: IndexError
        V = cand.vectors
        excl = self._exclusion(queried, cand, exclude) if exclude is not None and len(cand) else None

        def scores(uids):
            U = self.model.user_vectors(torch.as_tensor(uids.astype(np.int32), device=dev))
            kw = dict(scores=_hrec.tt_score(U, V), source="f32")
            if excl is not None:  # exclusion row q is queried[q]
                kw["excl"] = (torch.as_tensor(np.searchsorted(queried, uids), device=dev), *excl)
            return kw

        return ranked_lists.full_rank_metrics(users, items, weights, cand.item_ids, dev, scores, 4,
                                              self.RECOMMEND_FALLBACK_BYTES, host_rows=self.RANKING_HOST_ROWS)

    def rank_of(self, data, item_features, exclude=None):
        """A copy of `data` (columns userId, itemId) with an int64 `rank`
        column: the 0-based position of the row's item among ALL candidates of
        `item_features` (a frame, or candidates()'s object) in the user's
        ranking — larger predict_for_user score first, equal scores in frame
        order, NaN last — without the pairs of `exclude`. For any n <= 1024,
        rank < n holds exactly when the item stands at position rank of the
        user's list from recommend_for_users(users, item_features, n, exclude).
        -1: the item is not a candidate, or the pair is excluded. A user id
        outside the table raises IndexError. The scores are hrec_tt_score's
        at every width (predict_for_user's bits); scoring and counting
        (hrec_rank_positions) stay on the device."""
        cand = self.candidates(item_features)
        users, items = _int_ids(data["userId"], "userId"), _int_ids(data["itemId"], "itemId")
        rank, _ = self._full_rank(users, items, None, cand, exclude)
        return ranked_lists.rank_frame(data, rank)

    def full_ranking_metrics(self, data, item_features, weight_col=None, min_rating=None, label_col=None,
                             exclude=None):
        """ALSModel.full_ranking_metrics over the candidates of
        `item_features`: {"meanPercentileRank", "auc", "meanReciprocalRank",
        "count", "pairs", "unranked", "dropped"} of the pairs of `data` among
        ALL candidates (ties in frame order, not counted as 1/2; an item
        outside the candidate frame or an excluded pair is unranked and enters
        no statistic). The model has no coldStartStrategy: `dropped` is 0 and a
        user id outside the table raises IndexError."""
        cand = self.candidates(item_features)
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

    # ------------------------------------------- transform / regression metrics
    # The pointwise side (the reference compiles this model with
    # loss='mean_squared_error', metrics=['mae']): the prediction of every row
    # of a frame and the regression metrics of a split, as ALSModel.transform /
    # regression_metrics / evaluate. No counterpart in the reference: failures
    # raise. The model has no coldStartStrategy, so transform keeps every row.
    METRIC_NAMES = pair_metrics.METRIC_NAMES

    def _pair_operands(self, data, candidates):
        """(user ids int32 [n], item vectors f32 [m, d], item rows int64 [n]),
        all on the device: row p of `data` scores user p with item vector
        item_rows[p] (-1: an itemId the candidate frame does not hold)."""
        if self.model is None:
            raise RuntimeError("the two-tower model is not built or loaded")
        dev, sz = self.model.device, self.model.sizes
        users = torch.as_tensor(_ids(data["userId"].values, sz["user_emb"], "user_in"), device=dev)
        if candidates is not None:
            cand = self.candidates(candidates)
            return users, cand.vectors, cand.rows_of(torch.as_tensor(_int_ids(data["itemId"], "itemId"), device=dev))
        n = len(data)
        if n == 0:
            vec = torch.empty((0, int(self.embedding_size)), dtype=torch.float32, device=dev)
        else:
            num = _minmax_transform(self.scaler, data, ["price", "average_review_rating"])
            vec = self.model.item_vectors(
                torch.as_tensor(_ids(data["itemId"].values, sz["item_emb"], "item_id_in"), device=dev),
                torch.as_tensor(_ids(data["manufacturer_id"].values, sz["man_emb"], "manufacturer_in"), device=dev),
                torch.as_tensor(_ids(data["category_id"].values, sz["cat_emb"], "category_in"), device=dev),
                torch.as_tensor(np.ascontiguousarray(np.asarray(num, dtype=np.float32).reshape(-1, 2)), device=dev))
        return users, vec, torch.arange(n, dtype=torch.int64, device=dev)

    def transform(self, data, prediction_col="prediction", candidates=None):
        """A copy of `data` with the f32 prediction of every row in
        `prediction_col` (all rows kept), from one hrec_tt_predict_pairs
        launch; the user tower runs once per distinct user.
        Without `candidates`, `data` carries userId and the item columns
        predict_for_user needs; the item tower runs once per row over the
        fitted scaler's transform (never a refit), and row p has the bits
        predict_for_user(data.userId[p], data) gives at position p.
        With candidates (a frame, or candidates()'s object, whose stamp is
        checked as the list calls check it) `data` needs only userId and
        itemId: each itemId is looked up in the candidate frame on the device
        and scored with that row's vector - the bits predict_for_user over the
        candidate frame gives the pair; an itemId the frame does not hold gives
        NaN, a frame that repeats an itemId raises ValueError. A user id
        outside the table raises IndexError."""
        users, vec, rows = self._pair_operands(data, candidates)
        out = data.copy()
        out[prediction_col] = self.model.predict_pairs(users, vec, rows).cpu().numpy()
        return out

    def regression_metrics(self, data, label_col="average_review_rating", candidates=None):
        """Spark's RegressionMetrics of transform(data, candidates=candidates)
        against `label_col`: {"rmse", "mse", "mae", "r2", "var", "count",
        "dropped"} by ALSModel.regression_metrics' formulas. Rows with a NaN
        prediction (an item missing from the candidate frame) are left out and
        counted in "dropped". One hrec_tt_pair_metrics launch: the predictions
        never leave the device, only the ten f64 sums do."""
        users, vec, rows = self._pair_operands(data, candidates)
        y = torch.as_tensor(np.ascontiguousarray(np.asarray(data[label_col], np.float64)), device=self.model.device)
        sums = self.model.pair_sums(users, vec, rows, y)
        return pair_metrics.regression_metrics(dict(zip(_hrec.PAIR_SUMS, sums.tolist())))

    def evaluate(self, data, metric_name="rmse", label_col="average_review_rating", candidates=None):
        """One of rmse, mse, mae, r2, var of regression_metrics (a float).
        mse and mae are what Keras' model.evaluate reports for this model's
        loss='mean_squared_error' and metrics=['mae'], up to the f32 rounding
        of Keras' running batch means (the sums here are f64)."""
        ranked_lists.check_metric_name(metric_name, self.METRIC_NAMES)
        return float(self.regression_metrics(data, label_col, candidates)[metric_name])

    # ------------------------------------------------------------- fold-in
    # New users into a trained model without a refit. No
    # counterpart in the reference: failures raise.
    FOLD_IN_MAX_USER_ID = 1 << 24  # ids go through float32 (Keras Input(shape=(1,))): exact below this

    @classmethod
    def _fold_in_user_ids(cls, data):
        """data's userId column through _ids' float32 round trip (int64); IndexError outside [0, 2^24)."""
        users = np.asarray(data["userId"]).astype(np.float32).astype(np.int64)
        if users.size and (users.min() < 0 or users.max() >= cls.FOLD_IN_MAX_USER_ID):
            raise IndexError(f"user_in: id out of range [0, {cls.FOLD_IN_MAX_USER_ID})")
        return users

    def fold_in_users(self, data, item_features, steps=100, learning_rate=None):
        """Fit the user-embedding row of every user of `data` to that user's
        ratings with everything else frozen: `steps` Adam steps (a fresh
        optimiser per row, learning_rate or the model's) on the row alone, the
        user's whole history as one batch per step - what model.fit would do
        to that row - in one hrec_tt_fold_in_users launch for all users.
        data: userId, itemId, average_review_rating. item_features: a
        candidate frame or candidates()'s object; each itemId is looked up in
        it on the device and rows whose item it does not hold are dropped
        (their number: the returned frame's attrs["ratings_dropped"]). User
        ids take _ids' float32 round trip and must lie in [0, 2^24); an id
        beyond the user table grows it (DeviceTwoTower.grow_users: seeded
        Keras-init rows) and num_users with it. A row starts from what the
        table holds for that user. Only those users' rows of user_emb change:
        every other tensor, the Adam slots and `iterations` keep their bits, so
        a candidates() object built before the call stays valid. A user
        without a usable rating keeps its row and gets NaN losses.
        Returns a frame of userId (ascending), n_ratings, loss_before and
        loss_after (the mean squared error over the user's usable ratings)."""
        if self.model is None:
            raise RuntimeError("the two-tower model is not built or loaded")
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"steps must be >= 0 (got {steps})")
        cand = self.candidates(item_features)
        users = self._fold_in_user_ids(data)
        items = _int_ids(data["itemId"], "itemId")
        ratings = np.ascontiguousarray(np.asarray(data["average_review_rating"], dtype=np.float32))
        uniq, inv = np.unique(users, return_inverse=True)
        eng, dev = self.model, self.model.device
        if uniq.size == 0:
            out = pd.DataFrame({"userId": uniq, "n_ratings": np.zeros(0, np.int64),
                                "loss_before": np.zeros(0, np.float32), "loss_after": np.zeros(0, np.float32)})
            out.attrs["ratings_dropped"] = 0
            return out
        if int(uniq[-1]) + 1 > eng.sizes["user_emb"]:
            eng.grow_users(int(uniq[-1]) + 1)
            self.num_users = eng.sizes["user_emb"]
        # the history CSR: grouped by user, frame order inside a user; an item
        # outside the candidate frame keeps its slot as row -1, which the kernel skips
        inv_t = torch.as_tensor(np.ascontiguousarray(inv.reshape(-1)), device=dev)
        order = torch.sort(inv_t, stable=True).indices
        rows = cand.rows_of(torch.as_tensor(items, device=dev))
        indptr = torch.zeros(uniq.size + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(torch.bincount(inv_t, minlength=int(uniq.size)), 0)
        n_ok = torch.bincount(inv_t[rows >= 0], minlength=int(uniq.size))
        loss = eng.fold_in_users(torch.as_tensor(uniq, device=dev), indptr, rows[order].contiguous(),
                                 torch.as_tensor(ratings, device=dev)[order].contiguous(), cand.vectors, steps,
                                 learning_rate)
        loss = loss.cpu().numpy()
        n_ok = n_ok.cpu().numpy()
        out = pd.DataFrame({"userId": uniq, "n_ratings": n_ok, "loss_before": loss[:, 0], "loss_after": loss[:, 1]})
        out.attrs["ratings_dropped"] = int(users.size - n_ok.sum())
        return out

    # --------------------------------------------------------- persistence
    def save_model(self, model_path="models/twotower.keras"):
        os.makedirs(os.path.dirname(model_path) or ".", exist_ok=True)
        state = self.model.state_dict()
        state.update(self.model.optimizer_state())  # Keras saves the optimizer too (include_optimizer=True)
        meta = np.array([self.num_users, self.num_items, self.num_manufacturers, self.num_categories,
                         self.embedding_size], dtype=np.int64)
        with open(model_path, "wb") as f:
            # __seed__: grow_users draws new user rows from (the engine's seed, the old row count)
            np.savez(f, __meta__=meta, __lr__=np.float64(self.learning_rate), __seed__=np.int64(self.model.seed),
                     **state)
        with open(f"{model_path}_scaler.pkl", "wb") as f:
            pickle.dump(self.scaler, f)

    @classmethod
    def load_model(cls, model_path="models/twotower.keras"):
        with np.load(model_path, allow_pickle=False) as z:
            state = {k: z[k] for k in z.files}
        with open(f"{model_path}_scaler.pkl", "rb") as f:
            scaler = pickle.load(f)  # written by save_model above (own file)
        nu, ni, nm, nc, d = (int(x) for x in state["__meta__"])
        # a file written before the seed was saved: seed 0, the constructor's default
        loaded_model = cls(nu, ni, nm, nc, d, float(state["__lr__"]), seed=int(state.get("__seed__", 0)))
        loaded_model.build_model(init={k: v for k, v in state.items() if not k.startswith("__")})
        loaded_model.model.iterations = int(state["__iterations__"])
        loaded_model.model.load_optimizer_state(state)
        loaded_model.scaler = scaler
        loaded_model.is_trained = True
        return loaded_model


def hyperparameter_tuning(train_data, param_grid, val_size=0.2, random_state=42):
    """F1-based grid search (:169-236) over the device model. np.random.choice
    with random_state= raises TypeError in the reference (D4); a seeded
    Generator is used instead."""
    best_params = None
    best_f1 = 0.0
    train_users = train_data["userId"].unique()
    rng = np.random.default_rng(random_state)
    val_users = rng.choice(train_users, size=int(len(train_users) * val_size), replace=False)
    train_sub = train_data[~train_data["userId"].isin(val_users)]
    val_sub = train_data[train_data["userId"].isin(val_users)]
    # D4b: the reference sizes the tables by train_sub's distinct counts
    # (:186-189), but ids index the tables: once the validation users are
    # removed the largest user id is (almost surely) >= that count, Keras'
    # lookup raises, every grid point is skipped (:232-234) and the function
    # can only return None. Tables sized max(id) + 1 over train_data let the
    # loop do what it is written for.
    num_users = int(train_data["userId"].max()) + 1
    num_items = int(train_data["itemId"].max()) + 1
    num_man = int(train_data["manufacturer_id"].max()) + 1
    num_cat = int(train_data["category_id"].max()) + 1
    for params in param_grid:
        print(f"\nTesting parameters: {params}")
        try:
            model = TwoTowerModel(num_users=num_users, num_items=num_items, num_manufacturers=num_man,
                                  num_categories=num_cat, embedding_size=50, learning_rate=0.001)
            model.train(train_sub, val_sub, batch_size=params["batch_size"], epochs=params["epochs"])
            f1_scores = []
            items = val_sub[["itemId", "manufacturer_id", "category_id", "price",
                             "average_review_rating"]].drop_duplicates()
            for user_id in val_sub["userId"].unique()[:50]:
                sel = val_sub[val_sub["userId"] == user_id]
                actual = dict(zip(sel["itemId"], sel["average_review_rating"]))
                preds = model.predict_for_user(user_id, items)
                f1_scores.append(compute_f1_score(actual, dict(preds), k=10))
            avg_f1 = np.mean(f1_scores)
            print(f"  Avg F1@10: {avg_f1:.4f}")
            if avg_f1 > best_f1:
                best_f1 = avg_f1
                best_params = params.copy()
        except Exception as e:
            print(f"  Error with params {params}: {str(e)}")
            continue
    return best_params


def compute_f1_score(actual, pred, k=10):
    """src/two_tower_model.py:238-245 (k > 0 guarded)."""
    actual_items = set(actual.keys())
    pred_items = set(item for item, _ in sorted(pred.items(), key=lambda x: x[1], reverse=True)[:k])
    tp = len(actual_items & pred_items)
    precision = tp / k if k > 0 else 0
    recall = tp / len(actual_items) if len(actual_items) > 0 else 0
    return 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0
