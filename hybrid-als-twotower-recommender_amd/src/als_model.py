"""ALS collaborative filtering — drop-in for the reference's src/als_model.py.

Same class, method names, arguments, return values and error sentinels as
src/als_model.py:21-177; the Spark engine underneath (ALS.fit at :62,
ALSModel.transform at :75) is replaced by libhrec's HIP kernels:

  train            -> device CSR/CSC ingest + hrec_als_init_factors +
                      max_iter x (item half-sweep, user half-sweep)  [K1]
                      (under an initialised torch.distributed world of W
                      > 1 ranks — torchrun, one GPU per rank — every rank
                      calls train with the same frame; the users and items
                      are split into nnz-balanced row shards, the factors
                      replicated by RCCL all-gathers after each half-sweep,
                      and every rank ends with the full model: the factors
                      are bit-identical to the one-rank fit; with
                      implicit_prefs=True the row layouts permute the
                      summation order of YtY, so the implicit fit equals the
                      one-rank fit within the fit tolerance, rtol 1e-4 /
                      atol 1e-5, not bit for bit; nonnegative=True solves
                      every row by Spark's NNLS instead of Cholesky
                      (hrec_als_half_sweep_nonneg): explicit still
                      bit-identical, implicit within the fit tolerance)
  predict_for_user -> hrec_als_score (JVM-exact f32 dot, NaN for unknown
                      ids = coldStartStrategy "drop")                [K2]
                      + cold-start fallback via hrec_cosine_sim +
                      hrec_topk_f64 (_find_similar_items)            [K3]
  transform / regression_metrics / evaluate (Spark's ALSModel.transform on
                      a pair frame and RegressionEvaluator; not in the
                      reference) -> hrec_als_predict_pairs /
                      hrec_als_pair_metrics                          [K2x]
  recommend_for_all_users / _items / _user_subset / _item_subset (Spark's
                      recommendForAll* / recommendFor*Subset; not in the
                      reference) -> DeviceALSFactors.recommend: batches of
                      4096 query rows through hrec_als_score_topk_pruned
                      (bf16 matrix-core bound + the JVM-exact chain), raw
                      ids gathered on the device; with exclude= (a frame of
                      seen pairs, e.g. the training frame) through
                      hrec_als_score_topk_pruned_excluding: the same bound
                      over the unseen items of its sample, the seen items
                      left out before ranking; a batch without a usable
                      bound through hrec_als_score_topk_excluding (the
                      exact chain over every pair)
  ranking_metrics / evaluate_ranking (Spark's RankingMetrics /
                      RankingEvaluator: MAP, MAP@k, precision@k, recall@k,
                      NDCG@k; not in the reference) -> recommend's lists,
                      still on the device, against a label CSR ->
                      hrec_ranking_metrics                           [K2r]
  rank_of / full_ranking_metrics / evaluate_full_ranking (every held-out
                      item's position among ALL items: expected percentile
                      rank, AUC, uncut MRR; not in the reference) ->
                      hrec_als_score per sub-batch + hrec_rank_positions
  list_quality_metrics / evaluate_list_quality (what the lists look like as
                      a whole: coverage, entropy and Gini of the exposure,
                      personalization, novelty, intra-list diversity,
                      unexpectedness; not in the reference) -> recommend's
                      column lists, still on the device ->
                      hrec_row_inv_norms + hrec_list_quality
  explain / explain_recommendations (a prediction as a sum of one term per
                      item of the user's history, y_i^T A_u^-1 y_j weighted by
                      the rating; not in the reference) -> the pairs grouped
                      into lists, or recommend's column lists, still on the
                      device -> hrec_als_explain

`initialize_spark` / `stop_spark` keep their names: they bind / release the
HIP device session that plays the SparkSession's role.
"""
import json
import os
import pickle
import time
import warnings

import numpy as np
import torch

from . import _hrec, pair_metrics, ranked_lists
from .ranked_lists import int_ids as _int_ids
from .als_engine import DeviceALS, padded_k, process_group
from .als_ingest import check_same_frame, frame_fingerprint, sharded_ingest
from .data_preprocessing import get_item_features
from .synthetic import DeviceCSR

warnings.filterwarnings("ignore")


class DeviceSession:
    """What SparkSession is to the reference: the engine handle (one HIP
    device, its default stream)."""

    def __init__(self, device=None):
        _hrec.require_device()
        _hrec.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)

    def stop(self):
        torch.cuda.synchronize(self.device)


class DeviceALSFactors:
    """The fitted model (Spark's ALSModel): ids + factor matrices on the device."""

    def __init__(self, user_ids, item_ids, U, V, k, Vt=None):
        """Vt (optional): the transpose an earlier model built of the same V (fold_in_users)."""
        self.user_ids = np.asarray(user_ids)   # sorted unique raw ids
        self.item_ids = np.asarray(item_ids)
        self.U = U                               # [n_users, kp] f32 device
        self.V = V                               # [n_items, kp] f32 device
        self.k = int(k)
        self.Vt = Vt if Vt is not None else (_hrec.transpose(V) if V.shape[0] else V.t().contiguous())
        self._ids_dev = {}  # "user" / "item" -> the sorted ids on the device (_ids_device)
        self._rec_ops = {}  # "user" / "item" -> recommend()'s operands (_recommend_operands)

    @staticmethod
    def _lookup(ids, keys):
        keys = np.fromiter(keys, np.int64, len(keys)) if isinstance(keys, list) else np.asarray(keys)
        if len(ids) == 0:
            return np.full(keys.shape, -1, dtype=np.int64)
        pos = np.searchsorted(ids, keys)
        pos = np.clip(pos, 0, len(ids) - 1)
        ok = ids[pos] == keys
        return np.where(ok, pos, -1).astype(np.int64)

    def _lookup_device(self, keys, side="item"):
        """_lookup for long id lists: the same binary search on the device
        over a cached copy of the sorted item (or user) ids."""
        ids = self._ids_device(side)
        k = torch.as_tensor(keys, device=ids.device)
        if ids.numel() == 0:
            return torch.full_like(k, -1)
        pos = torch.searchsorted(ids, k).clamp_(max=ids.numel() - 1)
        return torch.where(ids[pos] == k, pos, torch.full_like(pos, -1))

    def score(self, user_ids, item_list):
        """f32 [len(user_ids), len(item_list)]; NaN where either id is unknown."""
        dev = self.U.device
        urows_h = self._lookup(self.user_ids, user_ids)
        if urows_h.size and (urows_h < 0).all():  # unknown users only: NaN everywhere, no transform to run
            return torch.full((urows_h.size, len(item_list)), float("nan"), dtype=torch.float32, device=dev)
        urows = torch.as_tensor(urows_h, device=dev)
        if isinstance(item_list, np.ndarray) and item_list.dtype == np.int64 and item_list.size > 4096:
            irows = self._lookup_device(item_list)
        else:
            irows = torch.as_tensor(self._lookup(self.item_ids, item_list), device=dev)
        return _hrec.als_score(self.U, urows, self.Vt, irows, irows.numel(), self.k)

    PAIR_DEVICE_LOOKUP = 4096  # id lists longer than this are looked up on the device

    def _pair_rows(self, user_ids, item_ids):
        """(user rows, item rows): int64 device tensors, -1 for an unknown id."""
        dev = self.U.device
        rows = []
        for side, ids, keys in (("user", self.user_ids, user_ids), ("item", self.item_ids, item_ids)):
            keys = np.asarray(keys, np.int64)
            if keys.size > self.PAIR_DEVICE_LOOKUP:
                rows.append(self._lookup_device(keys, side))
            else:
                rows.append(torch.as_tensor(self._lookup(ids, keys), device=dev))
        if rows[0].numel() != rows[1].numel():
            raise ValueError("user_ids and item_ids must have the same length")
        return rows

    def predict_pairs(self, user_ids, item_ids):
        """f32 device [n]: the prediction of pair (user_ids[p], item_ids[p])
        (Spark ALSModel.transform on a pair frame, hrec_als_predict_pairs);
        NaN where either id is unknown. The bits of score() for that pair."""
        urows, irows = self._pair_rows(user_ids, item_ids)
        return _hrec.als_predict_pairs(self.U, self.V, urows, irows, self.k)

    def pair_sums(self, user_ids, item_ids, labels):
        """{name: float} of _hrec.PAIR_SUMS for the pairs' predictions against
        labels (hrec_als_pair_metrics): one scoring launch, one small copy."""
        urows, irows = self._pair_rows(user_ids, item_ids)
        y = torch.as_tensor(np.asarray(labels, np.float64), device=self.U.device)
        sums = _hrec.als_pair_metrics(self.U, self.V, urows, irows, self.k, y)
        return dict(zip(_hrec.PAIR_SUMS, sums.tolist()))

    RECOMMEND_BATCH = 4096               # query rows per hrec_als_score_topk_pruned(_excluding) call
    RECOMMEND_FALLBACK_BYTES = 1 << 30   # the overflow fallback's score matrix stays under this (per sub-batch)
    RECOMMEND_MAX = 1024                 # largest list length (the library's top_k limit)

    def _recommend_operands(self, side):
        """What ranking the other side for `side`'s rows needs, built once per
        model and side: (query factors, candidate factors row-major, their
        transpose, their bf16 operand, the candidates' raw ids on the device).
        side "item" is side "user" with U and V swapped."""
        if side not in ("user", "item"):
            raise ValueError(f"side must be 'user' or 'item' (got {side!r})")
        cache = self._rec_ops
        if side not in cache:
            Q, F = (self.U, self.V) if side == "user" else (self.V, self.U)
            if side == "user":
                Ft = self.Vt
            else:
                Ft = _hrec.transpose(F) if F.shape[0] else F.t().contiguous()
            bf = _hrec.als_items_bf16(F, self.k) if F.shape[0] else None
            ids_h = self.item_ids if side == "user" else self.user_ids
            ids = torch.as_tensor(np.asarray(ids_h, np.int64), device=Q.device)
            cache[side] = (Q, F, Ft, bf, ids)
        return cache[side]

    EXCLUSION_HOST_PAIRS = 1 << 16  # exclusion lists up to this many pairs are built on the host

    def _ids_device(self, side):
        """The sorted user (or item) ids on the device, cached."""
        if side not in self._ids_dev:
            ids_h = self.item_ids if side == "item" else self.user_ids
            self._ids_dev[side] = torch.as_tensor(np.asarray(ids_h, np.int64), device=self.U.device)
        return self._ids_dev[side]

    def exclusion(self, side, user_ids, item_ids):
        """The exclusion CSR recommend(side, ..., exclude=) takes, from the
        (user_ids[p], item_ids[p]) pairs of e.g. the training frame: device
        (indptr int64 [n_side + 1], cols int32), a row's columns ascending and
        distinct. Pairs with an id the model does not know are dropped,
        duplicates removed. side "user": rows are user rows, columns item
        rows; "item": the transpose. Built on the host up to
        EXCLUSION_HOST_PAIRS pairs, on the device (one sort of 64-bit keys)
        above; the ids may be numpy arrays or device tensors."""
        if side not in ("user", "item"):
            raise ValueError(f"side must be 'user' or 'item' (got {side!r})")
        sides = ("user", "item") if side == "user" else ("item", "user")  # (rows, columns)
        known = {"user": self.user_ids, "item": self.item_ids}
        pairs = {"user": user_ids, "item": item_ids}
        return ranked_lists.exclusion_csr(
            *(known[s] for s in sides), *(pairs[s] for s in sides), self.U.device, self.EXCLUSION_HOST_PAIRS,
            cols_sorted=True, device_keys=lambda: tuple(self._ids_device(s) for s in sides),
            what="user_ids and item_ids")

    def recommend(self, side, rows, num, exclude=None, _columns=False, diversify=None):
        """Top-`num` of the other side for each of `rows` (int64 row indices
        into `side`'s factor matrix, every one in range): device (ids int64
        [n, kk], scores f32 [n, kk]), kk = min(num, size of the other side).
        side "user" ranks items for user rows, "item" ranks users for item
        rows. ids are raw ids. A score has the bits predict_pairs / transform
        gives for that pair (the JVM f32 chain); a list is descending, equal
        scores keep the smaller raw id first (the ids are sorted, the library
        breaks ties on the row index). Batches of RECOMMEND_BATCH rows go
        through hrec_als_score_topk_pruned on one workspace; for kk > 8 a
        batch whose overflow flag is set is redone through hrec_als_score +
        hrec_topk in sub-batches of at most RECOMMEND_FALLBACK_BYTES of
        scores (kk <= 8: the library resolves it on the device).
        exclude (optional, exclusion(side, ...)'s pair): each list is the full
        stable ranking with the row's excluded entries deleted, cut to num;
        returns (ids, scores, lens int32 [n]) with lens = min(kk, size of the
        other side - the row's excluded entries), and id 0 / score NaN past a
        list's length. Three levels, each answering only the batches the one
        before flagged: hrec_als_score_topk_pruned_excluding (the bf16 bound
        over the sample's items that stay, the exact chain for the pairs it
        keeps); at every kk hrec_als_score_topk_excluding (the exact chain
        over every pair); hrec_als_score + hrec_mask_rows_f32 + hrec_topk.
        One flag per batch and level; one host read after the last batch of
        the first level, a second only if that one found a flag.
        _columns (internal): return (row indices of the other side int64
        [n, kk], scores, lens or None) instead: the lists before the id gather.
        diversify (optional, side "user" only): a ranked_lists.MMR. The top
        max(pool, num) items are ranked as above (after exclude), then
        hrec_mmr_rerank picks num of them by greedy Maximal Marginal Relevance
        with cosines between item factors. The lists are in SELECTION order,
        no longer descending by score; a score keeps the bits the plain list
        has for that item."""
        num = ranked_lists.check_num(num, self.RECOMMEND_MAX)
        if diversify is not None:
            mmr = ranked_lists.check_mmr(diversify)
            if side != "user":
                raise ValueError("diversify re-ranks the item lists of users: side must be 'user'")
            pool = self.recommend(side, rows, max(num, mmr.pool), exclude, _columns=True)
            ids = self._recommend_operands(side)[4]
            picked = ranked_lists.diversify(*pool, self.V, None, self.k, mmr, num)
            out = ranked_lists.diversify_finish(ids, *picked, int(self.V.shape[0]), _columns, exclude is not None)
            return out if _columns or exclude is not None else out[:2]
        Q, F, Ft, bf, ids = self._recommend_operands(side)
        dev = Q.device
        excl = exclude is not None
        if excl:
            indptr, cols = exclude
            if indptr.numel() != Q.shape[0] + 1 or indptr.dtype != torch.int64 or cols.dtype != torch.int32:
                raise ValueError(f"recommend: exclude must be exclusion('{side}', ...)'s (indptr int64 "
                                 f"[{Q.shape[0] + 1}], cols int32)")
        rows = torch.as_tensor(rows, dtype=torch.int64, device=dev).reshape(-1).contiguous()
        n, n_other = rows.numel(), int(F.shape[0])
        kk = min(num, n_other)
        out_i = (torch.zeros if excl else torch.empty)((n, kk), dtype=torch.int64, device=dev)
        out_v = torch.empty((n, kk), dtype=torch.float32, device=dev)
        lens = torch.zeros(n, dtype=torch.int32, device=dev) if excl else None
        outs = (out_i, out_v, lens) if excl else (out_i, out_v)
        if n == 0 or kk == 0:
            return (out_i, out_v, lens) if _columns else outs
        if bool(((rows < 0) | (rows >= Q.shape[0])).any().item()):
            raise ValueError(f"recommend: a {side} row is outside [0, {Q.shape[0]})")
        B = int(self.RECOMMEND_BATCH)
        starts = range(0, n, B)
        flags = torch.zeros(len(starts), dtype=torch.int32, device=dev)
        # with an exclusion the pruned query covers the exact entry's need: one workspace for both levels
        lib = _hrec.lib()
        query = (lib.hrec_als_score_topk_pruned_excluding_workspace_bytes if excl
                 else lib.hrec_als_score_topk_pruned_workspace_bytes)
        ws = torch.empty(int(query(min(B, n), n_other, kk, self.k)), dtype=torch.uint8, device=dev)

        def batch(entry, b, *operands, **kw):
            sl = slice(starts[b], starts[b] + B)
            out = (out_i[sl], out_v[sl], lens[sl]) if excl else (out_i[sl], out_v[sl])
            entry(Q, rows[sl], Ft, *operands, overflow_out=flags[b: b + 1], workspace=ws, out=out, **kw)

        for b in range(len(starts)):
            if excl:
                batch(_hrec.als_score_topk_pruned_excluding, b, F, bf, n_other, self.k, kk, indptr, cols)
            else:
                batch(_hrec.als_score_topk_pruned, b, F, bf, n_other, self.k, kk, check_overflow=False)
        # one host read for all batches; a flagged batch is incomplete (without an exclusion only for kk > 8:
        # below, the library resolved it on the device)
        redo = torch.nonzero(flags).reshape(-1).tolist() if excl or kk > 8 else ()
        if excl:
            flags.zero_()
            for b in redo:  # the exact chain over every pair of that batch
                batch(_hrec.als_score_topk_excluding, b, n_other, self.k, kk, indptr, cols)
            redo = torch.nonzero(flags).reshape(-1).tolist() if redo else ()
        del ws
        for b in redo:  # the materialised scores
            _hrec.topk_materialised(lambda s, e: _hrec.als_score(Q, rows[s:e], Ft, None, n_other, self.k),
                                    starts[b], min(starts[b] + B, n), n_other, kk, self.RECOMMEND_FALLBACK_BYTES,
                                    out_i, out_v, lens, (rows, indptr, cols) if excl else None)
        if _columns:
            return out_i, out_v, lens
        if not excl:
            return ids[out_i], out_v
        return (*ranked_lists.pad_lists(ids, out_i, out_v, lens, n_other), lens)

    # Spark 3.5 ALSModel directory layout (MLWriter): metadata/part-00000 is
    # one JSON line with the model params and "rank"; userFactors/ and
    # itemFactors/ are parquet datasets of (id: int, features: array<float>).
    # A model saved here loads in Spark and vice versa.
    def save(self, path, params=None):
        import uuid

        import pyarrow as pa
        import pyarrow.parquet as pq

        meta = {"class": "org.apache.spark.ml.recommendation.ALSModel", "timestamp": int(time.time() * 1000),
                "sparkVersion": "3.5.1", "uid": f"ALS_{uuid.uuid4().hex[:12]}",
                "paramMap": dict(params or {}),
                "defaultParamMap": {"blockSize": 4096, "predictionCol": "prediction", "itemCol": "item",
                                    "userCol": "user", "coldStartStrategy": "nan"},
                "rank": self.k}
        os.makedirs(os.path.join(path, "metadata"), exist_ok=True)
        with open(os.path.join(path, "metadata", "part-00000"), "w") as f:
            f.write(json.dumps(meta, separators=(",", ":")) + "\n")
        open(os.path.join(path, "metadata", "_SUCCESS"), "w").close()
        feat_t = pa.list_(pa.field("element", pa.float32(), nullable=False))
        for name, ids, fac in (("userFactors", self.user_ids, self.U), ("itemFactors", self.item_ids, self.V)):
            d = os.path.join(path, name)
            os.makedirs(d, exist_ok=True)
            mat = fac[:, : self.k].cpu().numpy()
            feats = pa.FixedSizeListArray.from_arrays(pa.array(mat.reshape(-1), pa.float32()), self.k)
            table = pa.table({"id": pa.array(np.asarray(ids, np.int32), pa.int32()),
                              "features": feats.cast(feat_t)})
            pq.write_table(table, os.path.join(d, f"part-00000-{uuid.uuid4()}-c000.snappy.parquet"),
                           compression="snappy")
            open(os.path.join(d, "_SUCCESS"), "w").close()

    @classmethod
    def load(cls, path, device):
        import pyarrow.parquet as pq

        with open(os.path.join(path, "metadata", "part-00000")) as f:
            k = int(json.loads(f.readline())["rank"])
        kp = padded_k(k)

        def fac(name):
            t = pq.read_table(os.path.join(path, name))
            ids = np.asarray(t.column("id").to_numpy(), np.int64)
            flat = t.column("features").combine_chunks().flatten().to_numpy(zero_copy_only=False)
            mat = np.asarray(flat, np.float32).reshape(len(ids), k)
            order = np.argsort(ids, kind="stable")  # Spark writes partitions in any order
            out = torch.zeros((len(ids), kp), dtype=torch.float32, device=device)
            out[:, :k] = torch.as_tensor(mat[order], device=device)
            return ids[order], out

        user_ids, U = fac("userFactors")
        item_ids, V = fac("itemFactors")
        return cls(user_ids, item_ids, U, V, k)


class _PyInts:
    """Candidate ids from a pandas Index / Series: element i is the Python int
    the Series iteration yields (vals.item(i)); the list is built only if
    someone iterates (the per-item list path)."""

    def __init__(self, vals):
        self.vals = vals

    def __len__(self):
        return len(self.vals)

    def __getitem__(self, i):
        return self.vals.item(i)

    def __iter__(self):
        return iter(self.vals.tolist())


def build_csr(rows, cols, vals, n_rows, n_cols, alias=False, rows_in_order=None, indptr=None):
    """Device CSR of COO ratings (hrec_coo_to_csr): rows ascending, a row's
    entries in input order; duplicate (u, i) ratings stay separate terms, as
    in Spark. rows/cols int32, vals f32, all device tensors. alias: rows
    already in order hand back cols / vals themselves (no copy);
    rows_in_order / indptr: the rows' order and row pointer when known (from
    encode_ids(..., order=True); else checked / built on the device)."""
    indptr, indices, values = _hrec.coo_to_csr(rows, cols, vals, int(n_rows), alias=alias,
                                               rows_in_order=rows_in_order, indptr=indptr)
    return DeviceCSR(indptr, indices, values, 0, int(n_rows), int(n_cols))


def java_string_hash(s):
    """java.lang.String.hashCode (s[0] 31^(n-1) + ... + s[n-1], int32)."""
    h = 0
    for ch in s:
        h = (31 * h + ord(ch)) & 0xFFFFFFFF
    return h - (1 << 32) if h >= 1 << 31 else h


def default_seed():
    """Spark ALS's default seed, HasSeed's this.getClass.getName.hashCode:
    the same in every process (Python's str hash is salted per process, so a
    torchrun world would start each rank from other factors)."""
    return java_string_hash("org.apache.spark.ml.recommendation.ALS") & ((1 << 63) - 1)


class ALSModel:
    """src/als_model.py:21 — same constructor signature (+ optional seed)."""

    CHUNKS = 4  # W > 1: user-side row chunks per rank (overlapped all-gathers)

    def __init__(self, rank=10, max_iter=10, reg_param=0.1, cold_start_strategy="drop", seed=None,
                 implicit_prefs=False, alpha=1.0, nonnegative=False):
        """implicit_prefs / alpha: Spark ALS's implicitPrefs and alpha (the
        confidence 1 + alpha |r| of the implicit-feedback objective); rank
        <= 64 when set. nonnegative: Spark ALS's nonnegative (every factor
        row solved by NNLS, so all factors are >= 0); rank <= 64 when set."""
        self.nonnegative = nonnegative
        self.implicit_prefs = implicit_prefs
        self.alpha = alpha
        self.rank = rank
        self.max_iter = max_iter
        self.reg_param = reg_param
        self.cold_start_strategy = cold_start_strategy
        self.model = None
        self.spark = None
        self.global_mean = 3.0
        self.item_features = None
        self.seed = seed
        self.ingest_peak_bytes = None  # device bytes the last train's ingest peaked at (cuda only)

    @property
    def item_features(self):
        return self._item_features

    @item_features.setter
    def item_features(self, value):
        """Assigning the features (train, load_model, a caller) drops what was
        derived from them: the feature matrix and the cold-start fallback."""
        self._item_features = value
        self._feat_cache = None
        self._fb_cache = None
        self._fb_keys = None

    # -------------------------------------------------------- engine handle
    def initialize_spark(self):
        try:
            if self.spark is None:
                self.spark = DeviceSession()
            return True
        except Exception as e:
            print(f"Spark init error: {str(e)}")
            return False

    def stop_spark(self):
        if self.spark:
            self.spark.stop()

    # ---------------------------------------------------------------- train
    def _fit(self, data, U0=None):
        if self.cold_start_strategy not in ("drop", "nan"):
            raise ValueError(f"coldStartStrategy {self.cold_start_strategy!r} is not supported")
        dev = self.spark.device
        users_h = _int_ids(data["userId"], "userId")
        items_h = _int_ids(data["itemId"], "itemId")
        ratings_h = np.asarray(data["average_review_rating"], dtype=np.float32)
        k = int(self.rank)
        imp = {}
        if self.implicit_prefs:
            if padded_k(k) > 64:
                raise ValueError(f"implicit_prefs=True supports rank <= 64 (got rank {k})")
            if not float(self.alpha) >= 0.0:
                raise ValueError(f"alpha must be >= 0 (got {self.alpha})")
            imp = {"implicit": True, "alpha": float(self.alpha)}
        if self.nonnegative:
            if padded_k(k) > 64:
                raise ValueError(f"nonnegative=True supports rank <= 64 (got rank {k})")
            imp["nonnegative"] = True
        world, rank, group = process_group()
        track = dev.type == "cuda"
        if track:  # the ingest's peak device memory (tests: W = 2 holds about half of W = 1)
            torch.cuda.synchronize(dev)
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
        if world > 1:
            # this rank's slice of the frame only; ids encoded
            # over the whole frame, this rank's nnz-balanced row parts built
            # from the ratings exchanged to it (src/als_ingest.py)
            check_same_frame(frame_fingerprint(users_h, items_h, ratings_h), dev, group)
            user_ids, item_ids, csr, csc, ulay, ilay = sharded_ingest(users_h, items_h, ratings_h, world, rank, group,
                                                                      self.CHUNKS, dev)
            n_u, n_i = len(user_ids), len(item_ids)
        else:
            users, items = torch.as_tensor(users_h).to(dev), torch.as_tensor(items_h).to(dev)
            ratings = torch.as_tensor(ratings_h).to(dev)
            # ingest on the device (§8(f) row 1): dense codes + CSR (users) / CSC (items)
            rng = (lambda a: (int(a.min()), int(a.max())) if a.size else None)
            user_ids_t, urow, u_ord, u_ptr = _hrec.encode_ids(users, rng(users_h), order=True)
            item_ids_t, irow, i_ord, _ = _hrec.encode_ids(items, rng(items_h), order=True)
            user_ids, item_ids = user_ids_t.cpu().numpy(), item_ids_t.cpu().numpy()
            n_u, n_i = len(user_ids), len(item_ids)
            # ratings grouped by user: the row pointer came with the codes, the CSR is the input (no pass)
            csr = build_csr(urow, irow, ratings, n_u, n_i, alias=True, rows_in_order=u_ord, indptr=u_ptr)
            csc = build_csr(irow, urow, ratings, n_i, n_u, rows_in_order=i_ord)
            del urow, irow, ratings, users, items, user_ids_t, item_ids_t
        if track:
            torch.cuda.synchronize(dev)
            self.ingest_peak_bytes = int(torch.cuda.max_memory_allocated(dev) - base)
        if world > 1:
            eng = DeviceALS(n_u, n_i, k, float(self.reg_param), csr, csc, world=world, rank=rank, group=group,
                            chunks=self.CHUNKS, item_chunks=1, user_layout=ulay, item_layout=ilay, **imp)
        else:
            eng = DeviceALS(n_u, n_i, k, float(self.reg_param), csr, csc, **imp)
        if U0 is not None:
            eng.set_user_factors(U0)
        else:
            seed = default_seed() if self.seed is None else int(self.seed) & ((1 << 63) - 1)
            if world > 1:  # every rank starts from rank 0's factors
                t = torch.tensor([seed], dtype=torch.int64, device=dev)
                torch.distributed.broadcast(t, 0, group=group)
                seed = int(t.item())
            eng.init_user_factors(seed)
        eng.fit(int(self.max_iter))
        if world == 1:
            U, V = eng.U[:n_u].contiguous(), eng.V[:n_i].contiguous()
        else:  # every rank holds the replicated factors; back to global row order
            U = torch.zeros((n_u, eng.kp), dtype=torch.float32, device=dev)
            V = torch.zeros((n_i, eng.kp), dtype=torch.float32, device=dev)
            U[:, :k] = eng.user_factors
            V[:, :k] = eng.item_factors
        return DeviceALSFactors(user_ids, item_ids, U, V, k)

    def train(self, data, initial_user_factors=None):
        """src/als_model.py:43-66. `initial_user_factors` (optional, [n_users, rank]
        in sorted-userId order) injects Spark's random init for parity runs."""
        try:
            if not self.initialize_spark():
                return False
            self.item_features = get_item_features(data)
            self.global_mean = data["average_review_rating"].mean()
            model = self._fit(data, initial_user_factors)
            # A row whose normal equations are singular (reg_param 0 and fewer
            # independent ratings than the rank) comes out of the half-sweep
            # as NaN; Spark's CholeskySolver raises there and :62 fails.
            if not bool((torch.isfinite(model.U).all() & torch.isfinite(model.V).all()).item()):
                raise ArithmeticError("ALS factors are not finite: a row's normal equations are singular "
                                      "(reg_param = 0 needs at least rank independent ratings in every row)")
            self.model = model
            return True
        except Exception as e:
            print(f"Training error: {str(e)}")
            return False

    # --------------------------------------------------------------- predict
    @staticmethod
    def _check_int_ids(values):
        """Spark's createDataFrame(pairs, IntegerType schema) at :71-75
        rejects non-integer ids (e.g. the column names of a DataFrame, SURVEY
        D9). One pass over the distinct element types; the slow per-item scan
        only runs to name the offending value."""
        def ok(t):
            return issubclass(t, (int, np.integer)) and not issubclass(t, (bool, np.bool_))

        if all(ok(t) for t in set(map(type, values))):
            return
        for x in values:
            if not ok(type(x)):
                raise TypeError(f"field itemId: IntegerType() can not accept object {x!r} in type {type(x)}")

    @staticmethod
    def _id_array(all_items):
        """(items, int64 keys) for an integer numpy array / pandas Index /
        Series of candidate ids without a per-element Python pass, else None.
        `items` is indexable and iterates like `all_items` does in the
        reference's loop (:70): a numpy array yields numpy scalars, an Index or
        Series Python ints."""
        if isinstance(all_items, np.ndarray):
            if all_items.ndim == 1 and all_items.dtype.kind in "iu":
                return all_items, np.asarray(all_items).astype(np.int64, copy=False)
            return None
        import pandas as pd

        if isinstance(all_items, (pd.Index, pd.Series)) and all_items.dtype.kind in "iu":
            vals = all_items.to_numpy()
            return _PyInts(vals), vals.astype(np.int64, copy=False)
        return None

    def _score_device(self, user_id, all_items):
        """predict_for_user up to the transform: (items, int64 keys, f32 device
        scores [n] or None). Raises where the reference's createDataFrame /
        transform would."""
        self._check_int_ids([user_id])
        fast = self._id_array(all_items)
        if fast is not None:
            items, keys = fast
        else:
            items = list(all_items)
            self._check_int_ids(items)
            keys = np.fromiter(items, np.int64, len(items)) if items else None
        if len(items) == 0:
            return items, None, None
        return items, keys, self.model.score([user_id], keys)[0]

    def _predict_device(self, user_id, all_items):
        """For HybridRecommendationSystem's array path: (items, keys, f32
        device scores), else the predict_for_user list itself (same prints,
        same []). A user the model does not know (every row NaN: the
        reference protocol's test users) gets the fallback vector
        gathered for the candidates (f64, _cold_scores) when it applies; other
        NaN rows (unknown items) stay NaN, and the array path sends them to
        the list path, which applies the fallback through _predictions."""
        try:
            items, keys, scores = self._score_device(user_id, all_items)
            if scores is not None:
                if self.model._lookup(self.model.user_ids, [user_id])[0] < 0:
                    cold = self._cold_scores(keys)
                    if cold is not None:
                        scores = cold
                return items, keys, scores
            return self._predictions(items, scores)
        except Exception as e:
            print(f"Prediction error: {str(e)}")
            return []

    def predict_for_user(self, user_id, all_items):
        try:
            items, _, scores = self._score_device(user_id, all_items)
            return self._predictions(items, scores)
        except Exception as e:
            print(f"Prediction error: {str(e)}")
            return []

    def _predictions_guarded(self, items, scores):
        """_predictions under predict_for_user's own error contract (:68-91):
        a failing cold-start fallback prints 'Prediction error: ...' and gives
        [] for the ALS side only — for callers that took the scores through
        _predict_device and finish the list later (the hybrid's list path)."""
        try:
            return self._predictions(items, scores)
        except Exception as e:
            print(f"Prediction error: {str(e)}")
            return []

    def _predictions(self, items, scores):
        """The (item, prediction) list of :84 with the cold-start fallback
        (:78-86) for rows the transform left NaN: the per-item values of the
        precomputed fallback vector (_fallback), or — for features the kernel
        does not take — the per-call similarity search."""
        scores = scores.cpu().numpy() if scores is not None else np.zeros(0, np.float32)
        out = list(zip(items, scores.tolist()))  # (item, float(prediction)) as :84
        missing = np.flatnonzero(np.isnan(scores)).tolist()
        if not missing:
            return out
        # cold-start fallback (:78-86): mean rating of <= 3 similar items, else the global mean
        if self.item_features is not None:
            self._check_finite_features([items[n] for n in missing])
        fb = self._fallback() if self.item_features is not None else None
        if fb is not None:
            pos, mean, cnt = fb["pos"], fb["mean_h"], fb["cnt_h"]
            for n in missing:
                p = pos.get(items[n])  # the reference's item_features[item] (KeyError -> [] -> global mean)
                out[n] = (items[n], mean[p] if p is not None and cnt[p] > 0 else self.global_mean)
            return out
        sims = self._similar_batch([items[n] for n in missing])
        for n, sim in zip(missing, sims):
            out[n] = (items[n], np.mean([self.item_features[s]["rating"] for s in sim]) if sim
                      else self.global_mean)
        return out

    def _check_finite_features(self, query_items):
        """sklearn's cosine_similarity (:100) validates both arrays: a NaN or
        infinite feature vector anywhere in item_features raises ValueError
        from the reference's loop as soon as an item with features needs the
        fallback (and has another item to compare with)."""
        ids, pos, mat = self._feature_matrix()
        bad = self._feat_cache[4]
        if bad is None or len(ids) < 2 or not any(it in pos for it in query_items):
            return
        raise ValueError(bad)

    def _features_key(self):
        f = self.item_features
        return id(f), (len(f) if f is not None else -1)

    def _feature_matrix(self):
        key = self._features_key()
        if self._feat_cache is None or self._feat_cache[0] != key:
            feats = self.item_features or {}
            ids = list(feats.keys())
            bad = None
            if ids:
                mat = np.stack([np.asarray(feats[i]["features"], dtype=np.float64).ravel() for i in ids])
                dev_mat = torch.as_tensor(mat, device=self.spark.device if self.spark else "cuda")
                if not np.isfinite(mat).all():  # sklearn check_array's messages
                    bad = ("Input contains NaN." if np.isnan(mat).any() else
                           "Input contains infinity or a value too large for dtype('float64').")
            else:
                dev_mat = None
            self._feat_cache = (key, ids, {i: n for n, i in enumerate(ids)}, dev_mat, bad)
        return self._feat_cache[1:4]

    def _fallback(self):
        """The cold-start fallback of every item with features, computed once
        per item_features on the device (hrec_cold_fallback: the <= 3 most
        similar other items with cosine > 0.5 of :93-104 and np.mean of their
        ratings — the value of :84-85 for any user). A dict with "pos" (item
        -> row), "mean_h" (np.float64 per row), "cnt_h" (similar items kept)
        and their device copies; None when the features are outside the
        kernel (wider than 16, or ratings that are not Python / numpy f64
        floats, whose np.mean would run in another dtype), or absent."""
        key = self._features_key()
        if self._fb_cache is not None and self._fb_cache[0] == key:
            return self._fb_cache[1]
        ids, pos, mat = self._feature_matrix()
        fb = None
        feats = self.item_features
        if mat is not None and mat.shape[1] <= _hrec.COLD_MAX_DIM:
            r = [feats[i]["rating"] for i in ids]
            # np.mean converts ints (not bools) to f64 the same way; float32 etc. would sum in their dtype
            if all(type(x) in (float, int, np.float64, np.int64) for x in r):
                ratings = torch.as_tensor(np.asarray(r, np.float64), device=mat.device)
                mean, cnt, _ = _hrec.cold_fallback(mat, ratings)
                fb = {"ids": ids, "pos": pos, "mean": mean, "cnt": cnt, "mean_h": mean.cpu().numpy(),
                      "cnt_h": cnt.cpu().numpy()}
        self._fb_cache = (key, fb)
        self._fb_keys = None
        return fb

    def _cold_scores(self, keys):
        """For a cold user on the hybrid's array path: f64 device [n], the
        fallback value of each candidate key (global mean where the item has
        no features or no similar item), or None when _fallback is None, the
        features are not finite or the feature ids are not integers. Cached
        for the last candidate set."""
        if self.item_features is None:
            return None
        fb = self._fallback()
        if fb is None or self._feat_cache[4] is not None:  # non-finite features: the list path raises
            return None
        c = self._fb_keys
        if c is not None and c[0] is fb and c[1].shape == keys.shape and np.array_equal(c[1], keys):
            return c[2]
        if "sorted" not in fb:
            arr = np.asarray(fb["ids"])
            fb["sorted"] = None
            if arr.dtype.kind in "iu" and arr.dtype != np.uint64:
                order = np.argsort(arr, kind="stable")
                dev = fb["mean"].device
                fb["sorted"] = (torch.as_tensor(arr[order].astype(np.int64), device=dev),
                                torch.as_tensor(order.astype(np.int64), device=dev))
        if fb["sorted"] is None:
            return None
        sid, order = fb["sorted"]
        k = torch.as_tensor(np.asarray(keys, np.int64), device=sid.device)
        p = torch.searchsorted(sid, k).clamp_(max=sid.numel() - 1)
        row = order[p]
        hit = (sid[p] == k) & (fb["cnt"][row] > 0)
        gm = torch.full_like(fb["mean"][:1], float(self.global_mean))
        vals = torch.where(hit, fb["mean"][row], gm)
        self._fb_keys = (fb, np.array(keys, np.int64, copy=True), vals)
        return vals

    def _similar_batch(self, query_items, k=3):
        """_find_similar_items for many items at once on the device: cosine
        similarities (hrec_cosine_sim) + stable top-k (dict order breaks
        ties, like the reference's sorted()) + the sim > 0.5 filter."""
        if self.item_features is None:
            raise TypeError("'NoneType' object is not subscriptable")  # reference: None[item_id]
        ids, pos, mat = self._feature_matrix()
        res = [[] for _ in query_items]
        q = [(n, pos[it]) for n, it in enumerate(query_items) if it in pos]
        if not q or mat is None:
            return res
        dev = mat.device
        for s in range(0, len(q), 4096):
            chunk = q[s: s + 4096]
            qrows = torch.as_tensor([r for _, r in chunk], dtype=torch.int64, device=dev)
            sims = _hrec.cosine_sim(mat, qrows)
            idx, val = _hrec.topk(sims, k)
            idx, val = idx.cpu().numpy(), val.cpu().numpy()
            for (n, _), ii, vv in zip(chunk, idx, val):
                res[n] = [ids[j] for j, v in zip(ii, vv) if j >= 0 and v > 0.5]
        return res

    def _find_similar_items(self, item_id, k=3):
        try:
            self.item_features[item_id]
            return self._similar_batch([item_id], k)[0]
        except KeyError:
            return []

    # ------------------------------------------- transform / RegressionEvaluator
    # Spark's ALSModel.transform on a frame of (userId, itemId) rows and its
    # RegressionEvaluator over the result. Neither has a counterpart in the
    # reference, so failures raise instead of printing a sentinel.
    METRIC_NAMES = pair_metrics.METRIC_NAMES

    def _pair_ids(self, data):
        if self.model is None:
            raise RuntimeError("the ALS model is not trained or loaded")
        if self.cold_start_strategy not in ("drop", "nan"):
            raise ValueError(f"coldStartStrategy {self.cold_start_strategy!r} is not supported")
        return _int_ids(data["userId"], "userId"), _int_ids(data["itemId"], "itemId")

    def transform(self, data, prediction_col="prediction"):
        """A copy of `data` (columns userId, itemId) with the f32 prediction
        of every row in `prediction_col`; NaN where the user or the item is
        unknown to the model. cold_start_strategy "drop" removes those rows
        (order and index kept), "nan" keeps them."""
        users, items = self._pair_ids(data)
        pred = self.model.predict_pairs(users, items).cpu().numpy()
        out = data.copy()
        out[prediction_col] = pred
        if self.cold_start_strategy == "drop":
            out = out[~np.isnan(pred)]
        return out

    def regression_metrics(self, data, label_col="average_review_rating"):
        """Spark's RegressionMetrics of the predictions for `data` against
        `label_col` (unweighted, not through the origin), over the n rows
        kept: {"rmse", "mse", "mae", "r2", "var", "count", "dropped"} with
        mse = sum e^2 / n, mae = sum |e| / n, r2 = 1 - sum e^2 / sum (y -
        ybar)^2 and var = sum (p - ybar)^2 / n (ybar the label mean).
        cold_start_strategy "drop" leaves rows with a NaN prediction out and
        counts them in "dropped"; "nan" keeps them, and one such row makes
        every metric NaN. No row kept: NaN metrics, count 0. The predictions
        never leave the device (hrec_als_pair_metrics)."""
        users, items = self._pair_ids(data)
        s = self.model.pair_sums(users, items, np.asarray(data[label_col], np.float64))
        return pair_metrics.regression_metrics(s, drop_nan=self.cold_start_strategy != "nan")

    def evaluate(self, data, metric_name="rmse", label_col="average_review_rating"):
        """Spark's RegressionEvaluator(metricName=metric_name).evaluate of
        transform(data): one of rmse, mse, mae, r2, var (a float)."""
        ranked_lists.check_metric_name(metric_name, self.METRIC_NAMES)
        return float(self.regression_metrics(data, label_col)[metric_name])

    # ------------------------------------------------------------- fold-in
    # New users into a fitted model without a refit. No
    # counterpart in the reference or in Spark: failures raise.
    def _solve_user_rows(self, model, indptr, indices, values):
        """[n, kp] f32 device: the rows one user half-sweep of `train` gives
        the CSR (indptr int64 [n + 1], indices int32 item rows of model.V,
        values f32) against the fixed item factors: DeviceALS.user_half_sweep
        itself, on one rank, with this instance's reg_param, implicit_prefs /
        alpha and nonnegative, so the launch and its operands (the f64 source
        copy, YtY of model.V) are the ones DeviceALS._launcher forms in a fit."""
        n, n_items = int(indptr.numel()) - 1, int(model.V.shape[0])
        dev = model.V.device
        kw = {}
        if self.implicit_prefs:
            kw.update(implicit=True, alpha=float(self.alpha))
        if self.nonnegative:
            kw["nonnegative"] = True
        no_ratings = DeviceCSR(torch.zeros(n_items + 1, dtype=torch.int64, device=dev),
                               torch.empty(0, dtype=torch.int32, device=dev),
                               torch.empty(0, dtype=torch.float32, device=dev), 0, n_items, n)
        eng = DeviceALS(n, n_items, model.k, float(self.reg_param), DeviceCSR(indptr, indices, values, 0, n, n_items),
                        no_ratings, **kw)
        if eng.V.shape != model.V.shape:
            raise RuntimeError("fold_in_users: the model's item factors do not have the engine's layout")
        eng.V = eng.V_local = model.V  # the fit's source buffer, not a copy
        eng.user_half_sweep()
        return eng.U[:n]

    def fold_in_users(self, data, replace=False):
        """Give users the model has not seen a factor row from their ratings,
        without a refit: each user's normal equations are solved against the
        fixed item factors - exactly one row of train's user half-sweep, run
        by the same launch, so a folded row has the bits train would have
        produced for the same ratings against the same item factors. After the
        call every method serves and evaluates these users as known users.
        data: a frame with userId, itemId and average_review_rating, the
        columns train takes. Rows whose item the model does not know are
        dropped; within a user the remaining rows keep frame order (the f64
        Gramian sums depend on it). A user left without a row gets no factor
        row. replace=False: a user id the model already holds raises
        ValueError before any device work; replace=True: its row is
        overwritten by the solution from the given ratings alone. A row that
        is not finite (singular equations at reg_param = 0) raises ValueError
        and leaves the model as it was. Item factors, item ids, item_features
        and global_mean do not change. One GPU; under a torch.distributed
        world every rank does the same work, without collectives.
        Returns {"users_added", "users_replaced", "users_skipped",
        "ratings_used", "ratings_dropped"}."""
        model = self._trained()
        users, items = _int_ids(data["userId"], "userId"), _int_ids(data["itemId"], "itemId")
        ratings = np.ascontiguousarray(np.asarray(data["average_review_rating"], dtype=np.float32))
        uniq, inv = np.unique(users, return_inverse=True)
        known = model._lookup(model.user_ids, uniq) >= 0
        if known.any() and not replace:
            raise ValueError(f"fold_in_users: {int(known.sum())} user id(s) are already in the model (the first: "
                             f"{int(uniq[known][0])}); replace=True overwrites their rows")
        out = {"users_added": 0, "users_replaced": 0, "users_skipped": int(uniq.size), "ratings_used": 0,
               "ratings_dropped": int(users.size)}
        if users.size == 0 or len(model.item_ids) == 0:
            return out
        dev = model.U.device
        irow = model._lookup_device(items, "item")
        keep = irow >= 0
        inv_k = torch.as_tensor(np.ascontiguousarray(inv.reshape(-1)), device=dev)[keep]
        counts = torch.bincount(inv_k, minlength=int(uniq.size))
        has = (counts > 0).cpu().numpy()  # users with a rating on a known item
        used = int(inv_k.numel())
        out.update(users_skipped=int((~has).sum()), ratings_used=used, ratings_dropped=int(users.size) - used)
        if not has.any():
            return out
        order = torch.sort(inv_k, stable=True).indices  # grouped by user, frame order inside a user
        indptr = torch.zeros(int(has.sum()) + 1, dtype=torch.int64, device=dev)
        indptr[1:] = torch.cumsum(counts[counts > 0], 0)
        indices = irow[keep][order].to(torch.int32).contiguous()
        values = torch.as_tensor(ratings, device=dev)[keep][order].contiguous()
        rows = self._solve_user_rows(model, indptr, indices, values)
        if not bool(torch.isfinite(rows).all().item()):
            raise ValueError("fold_in_users: a new row is not finite: its normal equations are singular (reg_param = "
                             "0 needs at least rank independent ratings per user); the model is unchanged")
        new_ids = uniq[has]
        ids = np.union1d(np.asarray(model.user_ids, np.int64), new_ids)
        U = torch.zeros((ids.size, model.U.shape[1]), dtype=torch.float32, device=dev)
        U[torch.as_tensor(np.searchsorted(ids, np.asarray(model.user_ids, np.int64)), device=dev)] = model.U
        U[torch.as_tensor(np.searchsorted(ids, new_ids), device=dev)] = rows  # after the old rows: replace wins
        # a fresh model over the same item factors: nothing keyed on the user side survives
        self.model = DeviceALSFactors(ids.astype(np.asarray(model.user_ids).dtype, copy=False), model.item_ids, U,
                                      model.V, model.k, Vt=model.Vt)
        replaced = int((known & has).sum())
        out.update(users_added=int(has.sum()) - replaced, users_replaced=replaced)
        return out

    # --------------------------------------------------------- explanations
    # Why a prediction is what it is (Hu, Koren and Volinsky 2008,
    # section 5; `implicit`'s explain). A user row solves its normal equations,
    # x_u = A_u^-1 b_u, so y_i . x_u = sum_j beta_j (y_i^T A_u^-1 y_j) over the
    # user's history: one term per rated item. No counterpart in the reference
    # or in Spark: failures raise.
    @staticmethod
    def _explain_top(top):
        top = int(top)
        if not 1 <= top <= _hrec.EXPLAIN_MAX_TOP:
            raise ValueError(f"top must be in [1, {_hrec.EXPLAIN_MAX_TOP}] (got {top})")
        return top

    def _explain_setup(self, history, top):
        """(model, top, history CSR pieces, counts) of an explain call."""
        model = self._trained()
        if self.nonnegative:
            raise ValueError("explain: a nonnegative=True row is an NNLS solution, not A^-1 b: the prediction is not "
                             "a sum over the history")
        if int(model.U.shape[1]) > 64:
            raise ValueError(f"explain supports rank <= 64 (got rank {model.k})")
        top = self._explain_top(top)
        h_users, h_items = _int_ids(history["userId"], "userId"), _int_ids(history["itemId"], "itemId")
        ratings = np.asarray(history["average_review_rating"], dtype=np.float32)
        dev = model.U.device
        irow = model._lookup_device(h_items, "item") if h_items.size else torch.zeros(0, dtype=torch.int64, device=dev)
        uniq, indptr, cols, vals, dropped = ranked_lists.rated_history_csr(h_users, h_items, ratings, irow, dev)
        counts = (indptr[1:] - indptr[:-1]).cpu().numpy()
        entry_ids = np.asarray(model.item_ids, np.int64)[cols.cpu().numpy()] if cols.numel() else np.zeros(0, np.int64)
        yty = _hrec.als_gramian(model.V, model.k) if self.implicit_prefs and model.V.shape[0] else None
        info = {"ratings_used": int(cols.numel()), "ratings_dropped": int(dropped)}
        return model, top, uniq, indptr, cols, vals, counts, entry_ids, yty, info

    def _history_segment(self, uniq, counts, user_ids):
        """Each user id's row of the history CSR, -1 where it has no usable history (host int64)."""
        user_ids = np.asarray(user_ids, np.int64)
        if uniq.size == 0:
            return np.full(user_ids.shape, -1, np.int64)
        p = np.clip(np.searchsorted(uniq, user_ids), 0, uniq.size - 1)
        return np.where((uniq[p] == user_ids) & (counts[p] > 0), p, -1).astype(np.int64)

    def _explain_run(self, model, lists, list_len, hist_rows, u_rows, csr, yty, top):
        U_rows = model.U[u_rows.clamp(min=0)]
        return ranked_lists.explain_lists(lists, list_len, hist_rows, csr, model.V, model.k, float(self.reg_param), top,
                                          implicit=bool(self.implicit_prefs), alpha=float(self.alpha), yty=yty,
                                          U_rows=U_rows)

    def explain(self, data, history, top=5):
        """Explain the predictions of `data`'s (userId, itemId) pairs by the
        user's history. history: a frame with userId, itemId and
        average_review_rating, typically the training frame or the frame given
        to fold_in_users; its rows whose item the model does not know are
        dropped, the others keep frame order inside a user (as in
        fold_in_users). Returns a copy of `data` (every row kept) with
          prediction: transform's f32 prediction, with its bits;
          explained: f64, the sum of ALL the history's contributions - the
            prediction again, up to the f32 rounding of the stored user row,
            when `history` is what the row was fitted on;
          contributions: up to `top` (1 .. 32) (itemId, contribution) tuples of
            the user's own history, largest first; equal contributions keep
            the earlier history row first.
        A pair whose user or item the model does not know, or whose user has no
        usable history, gets explained NaN and an empty list. With this
        instance's reg_param, implicit_prefs / alpha (implicit: only ratings
        > 0 contribute). nonnegative=True and rank > 64 raise ValueError. The
        pairs are grouped per user on the device into lists of at most 1024
        (one kernel row each, hrec_als_explain).
        frame.attrs["explain"] = {"ratings_used", "ratings_dropped",
        "users_without_history", "max_refit_gap"}: max_refit_gap is the largest
        |A^-1 b - stored row| component over the explained users - f32 rounding
        when `history` is what the rows were fitted on, large when it is not.
        One GPU; under a torch.distributed world every rank does the same
        work, without collectives."""
        model, top, uniq, indptr, cols, vals, counts, entry_ids, yty, info = self._explain_setup(history, top)
        users, items = _int_ids(data["userId"], "userId"), _int_ids(data["itemId"], "itemId")
        dev = model.U.device
        n = int(users.size)
        pred = model.predict_pairs(users, items).cpu().numpy() if n else np.zeros(0, np.float32)
        urow, irow = (model._lookup(model.user_ids, users), model._lookup(model.item_ids, items))
        seg = self._history_segment(uniq, counts, users)
        known_users = np.unique(users[urow >= 0])
        info["users_without_history"] = int((self._history_segment(uniq, counts, known_users) < 0).sum())
        explained = np.full(n, np.nan, np.float64)
        contributions = [[] for _ in range(n)]
        ok = (urow >= 0) & (irow >= 0) & (seg >= 0)
        info["max_refit_gap"] = 0.0
        if ok.any():
            L_MAX = _hrec.EXPLAIN_LIST_MAX
            idx = torch.as_tensor(np.nonzero(ok)[0], device=dev)
            seg_d = torch.as_tensor(seg, device=dev)[idx]
            order = torch.sort(seg_d, stable=True).indices  # grouped by user, frame order inside a user
            idx, seg_s = idx[order], seg_d[order]
            useg, cnt = torch.unique_consecutive(seg_s, return_counts=True)
            start = torch.cumsum(cnt, 0) - cnt
            rows_per = (cnt + L_MAX - 1) // L_MAX  # kernel rows of each user
            row0 = torch.cumsum(rows_per, 0) - rows_per
            group = torch.repeat_interleave(torch.arange(useg.numel(), device=dev), cnt)
            within = torch.arange(idx.numel(), device=dev) - start[group]
            krow = row0[group] + within // L_MAX
            slot = within % L_MAX
            R, L = int(rows_per.sum().item()), int(min(L_MAX, int(cnt.max().item())))
            lists = torch.full((R, L), -1, dtype=torch.int64, device=dev)
            lists[krow, slot] = torch.as_tensor(irow, device=dev)[idx]
            hist_rows = torch.repeat_interleave(useg, rows_per)
            u_rows = torch.zeros(R, dtype=torch.int64, device=dev)
            u_rows[krow] = torch.as_tensor(urow, device=dev)[idx]
            total, pos, val, length, gap = self._explain_run(model, lists, None, hist_rows, u_rows,
                                                             (indptr, cols, vals), yty, top)
            at = idx.cpu().numpy()
            explained[at] = total[krow, slot].cpu().numpy()
            seg_start = indptr[seg_s].cpu().numpy()
            tuples = ranked_lists.explain_tuples(pos[krow, slot].cpu().numpy(), val[krow, slot].cpu().numpy(),
                                                 length[krow, slot].cpu().numpy(), seg_start, entry_ids)
            for p, t in zip(at.tolist(), tuples):
                contributions[p] = t
            info["max_refit_gap"] = float(gap.item())
        out = data.copy()
        out["prediction"] = pred
        out["explained"] = explained
        out["contributions"] = contributions
        out.attrs["explain"] = info
        return out

    def explain_recommendations(self, users, num_items, history, top=5, exclude=None):
        """recommend_for_user_subset with the reasons: a DataFrame with one
        row per known user of `users`, `userId` ascending, `recommendations`:
        (itemId, rating, [(itemId, contribution), ...]) tuples - the ids and
        rating bits of recommend_for_user_subset(users, num_items, exclude),
        each with explain's contributions for that pair - and `explained`: per
        list entry explain's f64 sum (NaN for a user without usable history,
        whose tuples carry empty lists). history, top and
        frame.attrs["explain"] are explain's; exclude works as everywhere else
        (exclude=history is the usual call). The top-k's column matrix goes
        into hrec_als_explain without leaving the device."""
        import pandas as pd

        model, top, uniq, indptr, cols, vals, counts, entry_ids, yty, info = self._explain_setup(history, top)
        ids = np.asarray(model.user_ids, np.int64)
        if isinstance(users, pd.DataFrame):
            users = users["userId"]
        keys = np.unique(_int_ids(np.asarray(users).reshape(-1), "userId"))
        rows = model._lookup(ids, keys)
        rows = rows[rows >= 0]
        dev = model.U.device
        excl = None if exclude is None else self._exclusion("user", exclude)
        lists, scores, lens = model.recommend("user", rows, num_items, exclude=excl, _columns=True)
        seg = self._history_segment(uniq, counts, ids[rows])
        info["users_without_history"] = int((seg < 0).sum())
        info["max_refit_gap"] = 0.0
        n, kk = int(lists.shape[0]), int(lists.shape[1])
        lens_h = np.full(n, kk, np.int64) if lens is None else lens.cpu().numpy().astype(np.int64)
        item_ids = np.asarray(model.item_ids, np.int64)
        recs, expl = [[] for _ in range(n)], [[] for _ in range(n)]
        if n and kk:
            total, pos, val, length, gap = self._explain_run(
                model, lists, lens, torch.as_tensor(seg, device=dev), torch.as_tensor(rows, device=dev),
                (indptr, cols, vals), yty, top)
            info["max_refit_gap"] = float(gap.item())
            seg_start = np.repeat(indptr[torch.as_tensor(np.maximum(seg, 0), device=dev)].cpu().numpy(), kk)
            tuples = ranked_lists.explain_tuples(pos.reshape(n * kk, top).cpu().numpy(),
                                                 val.reshape(n * kk, top).cpu().numpy(),
                                                 length.reshape(n * kk).cpu().numpy(), seg_start, entry_ids)
            cols_h = lists.cpu().numpy()
            rec_ids = item_ids[np.clip(cols_h, 0, max(item_ids.size - 1, 0))].tolist()
            sc, tot = scores.cpu().numpy().tolist(), total.cpu().numpy().tolist()
            for r in range(n):
                m = int(lens_h[r])
                recs[r] = [(rec_ids[r][e], sc[r][e], tuples[r * kk + e]) for e in range(m)]
                expl[r] = tot[r][:m]
        out = pd.DataFrame({"userId": ids[rows], "recommendations": recs, "explained": expl})
        out.attrs["explain"] = info
        return out

    # ------------------------------------------------ recommendForAll / Subset
    # Spark's ALSModel.recommendForAllUsers / recommendForAllItems /
    # recommendForUserSubset / recommendForItemSubset. No counterpart in the
    # reference: failures raise. After a fit in a torch.distributed world of
    # W > 1 ranks every rank holds the full model, and each rank that calls
    # these computes the whole answer (the recommendation is not sharded).
    def _trained(self):
        if self.model is None:
            raise RuntimeError("the ALS model is not trained or loaded")
        return self.model

    def _exclusion(self, side, exclude):
        """The device exclusion CSR of an `exclude` frame (columns userId, itemId)."""
        return self.model.exclusion(side, _int_ids(exclude["userId"], "userId"), _int_ids(exclude["itemId"], "itemId"))

    def _recommend_frame(self, side, subset, num, exclude=None, diversify=None):
        import pandas as pd

        model = self._trained()
        if diversify is not None and side != "user":
            raise ValueError("diversify re-ranks the item lists of users; the user lists of items are not diversified")
        col, ids = ("userId", model.user_ids) if side == "user" else ("itemId", model.item_ids)
        ids = np.asarray(ids, np.int64)
        if subset is None:
            rows = np.arange(len(ids), dtype=np.int64)
        else:
            if isinstance(subset, pd.DataFrame):
                subset = subset[col]
            keys = np.unique(_int_ids(np.asarray(subset).reshape(-1), col))
            rows = model._lookup(ids, keys)
            rows = rows[rows >= 0]  # ids the model does not know are left out (Spark's join)
        if exclude is None:
            (rec_ids, scores), lens = model.recommend(side, rows, num, diversify=diversify), None
        else:
            rec_ids, scores, lens = model.recommend(side, rows, num, exclude=self._exclusion(side, exclude),
                                                    diversify=diversify)
        return ranked_lists.lists_frame(col, ids[rows], rec_ids, scores, lens)

    def recommend_for_all_users(self, num_items, exclude=None, diversify=None):
        """Spark's recommendForAllUsers: a DataFrame with one row per user
        of the model, `userId` ascending, and `recommendations`: the user's
        top num_items (1 .. 1024) items as (itemId: int, rating: float)
        tuples, best first; equal ratings keep the smaller itemId first. A
        rating is transform's f32 prediction for that pair. Scored and ranked
        on the device (DeviceALSFactors.recommend); on every rank of a
        multi-GPU world the whole answer.
        exclude (optional; here and in the three methods below): a DataFrame
        with userId and itemId columns, typically the training frame. Its
        pairs never appear in a list (the left-anti join Spark users apply to
        the exploded recommendations, done while ranking): each list is the
        full ranking without them, cut to num_items, so it is shorter than
        num_items only when fewer entries remain; a row with everything
        excluded keeps its row with an empty list. Pairs with an id the model
        does not know, and repeated pairs, change nothing.
        diversify (optional; here, in recommend_for_user_subset and in the
        ranking and list-quality metrics below): a ranked_lists.MMR(lambda_,
        pool). The model ranks max(pool, num_items) items (after exclude) and
        greedy Maximal Marginal Relevance picks num_items of them, each pick
        trading its rating (min-max scaled over the pool) against its largest
        cosine, between item factors, to the picks before. The lists are then
        in SELECTION order, no longer descending by rating; a tuple keeps the
        rating bits the plain list has for that item. None: the plain ranking."""
        return self._recommend_frame("user", None, num_items, exclude, diversify)

    def recommend_for_all_items(self, num_users, exclude=None, diversify=None):
        """Spark's recommendForAllItems: per item (`itemId` ascending) its
        top num_users users as (userId, rating) tuples. diversify is not
        supported on the item side: anything but None raises ValueError."""
        return self._recommend_frame("item", None, num_users, exclude, diversify)

    def recommend_for_user_subset(self, users, num_items, exclude=None, diversify=None):
        """Spark's recommendForUserSubset: recommend_for_all_users for the
        distinct ids of `users` (a DataFrame with a userId column, or an
        array-like of ids); ids unknown to the model are left out."""
        return self._recommend_frame("user", users, num_items, exclude, diversify)

    def recommend_for_item_subset(self, items, num_users, exclude=None, diversify=None):
        """Spark's recommendForItemSubset (a DataFrame with an itemId column,
        or an array-like of ids). diversify is not supported on the item side:
        anything but None raises ValueError."""
        return self._recommend_frame("item", items, num_users, exclude, diversify)

    # ------------------------------------------------ cosine neighbours
    # implicit's similar_items / similar_users ("more like this"): the rows
    # of one factor matrix ranked by cosine (hrec_cosine_topk).
    def _similar_frame(self, side, subset, num, min_similarity):
        model = self._trained()
        col, ids, F = ("userId", model.user_ids, model.U) if side == "user" else ("itemId", model.item_ids, model.V)
        # the ids ascend: "the earlier row first" is "the smaller id first"
        return ranked_lists.similar_rows_frame(col, ids, F, model.k, subset, num, min_similarity,
                                               ids_dev=model._ids_device(side))

    def similar_items(self, items=None, num=10, min_similarity=None):
        """implicit's similar_items: a DataFrame with one row per item
        (`itemId` ascending; None: every item of the model; a DataFrame with
        an itemId column or an array-like of ids otherwise: its distinct ids,
        unknown ones left out) and `recommendations`: the item's `num` (1 ..
        1024) nearest other items by the cosine between item factors, as
        (itemId: int, similarity: float) tuples, best first. Equal
        similarities keep the smaller itemId first; the item itself never
        appears; min_similarity (None: no cut) keeps the similarities above
        it (the reference's _find_similar_items: num=3, min_similarity=0.5).
        A similarity is the f64 cosine of hrec_cosine_topk: the same bits on
        every call. An item with a zero factor row has similarity 0.0 to
        everything. Ranked on the device; on every rank of a multi-GPU world
        the whole answer."""
        return self._similar_frame("item", items, num, min_similarity)

    def similar_users(self, users=None, num=10, min_similarity=None):
        """implicit's similar_users: similar_items over the user factors
        (`userId`, (userId, similarity) tuples)."""
        return self._similar_frame("user", users, num, min_similarity)

    # ----------------------------------------- RankingEvaluator / RankingMetrics
    RANKING_METRIC_NAMES = ("meanAveragePrecision", "meanAveragePrecisionAtK", "precisionAtK", "recallAtK",
                            "ndcgAtK")
    RANKING_HOST_ROWS = 1 << 16  # frames up to this many rows: the label CSR is built on the host

    def ranking_metrics(self, data, k=10, label_col=None, min_rating=None, exclude=None, diversify=None):
        """Spark's RankingMetrics (binary relevance) of the model's top-k item
        lists against `data` (columns userId, itemId): {"meanAveragePrecision",
        "meanAveragePrecisionAtK", "precisionAtK", "recallAtK", "ndcgAtK",
        "count", "dropped"}. A user's ground truth is the set of its itemIds
        in `data` — with min_rating, of the rows whose label_col (default
        average_review_rating) is >= min_rating; a user left with no row does
        not appear. Items unknown to the model stay in the set: never hit,
        counted in its size. Each metric is the mean over the `count` users
        evaluated (NaN when count is 0). cold_start_strategy "drop" leaves
        users unknown to the model out and counts them in "dropped"; "nan"
        keeps them with an empty list (every metric 0 for them, as Spark gives
        for an empty prediction array). The lists never leave the device
        (DeviceALSFactors.recommend -> hrec_ranking_metrics).
        exclude (optional): a DataFrame with userId and itemId columns,
        typically the training frame of a held-out split; the lists are
        ranked without its pairs (recommend_for_all_users' exclude), each
        evaluated at its own length. An item of `data` that is also excluded
        can never be hit and still counts in its user's set size.
        diversify (optional): recommend_for_all_users' MMR; the metrics are
        those of the diversified lists, in selection order, which go from
        hrec_mmr_rerank into hrec_ranking_metrics on the device."""
        k = ranked_lists.check_num(k, _hrec.RANK_MAX, "k")
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        users, items = self._pair_ids(data)
        if min_rating is not None:
            keep = np.asarray(data[label_col or "average_review_rating"], np.float64) >= float(min_rating)
            users, items = users[keep], items[keep]
        model, dev = self.model, self.model.U.device
        dropped = 0
        if self.cold_start_strategy == "drop":  # pairs of unknown users go before the CSR is built
            if users.size > model.PAIR_DEVICE_LOOKUP:
                known = (model._lookup_device(users, "user") >= 0).cpu().numpy()
            else:
                known = model._lookup(model.user_ids, users) >= 0
            dropped = int(np.unique(users[~known]).size)
            users, items = users[known], items[known]
        uniq, indptr, labels = ranked_lists.label_csr(users, items, dev, self.RANKING_HOST_ROWS)
        n = int(uniq.numel())
        res = {name: float("nan") for name in self.RANKING_METRIC_NAMES}
        res.update(count=n, dropped=dropped)
        if n == 0:
            return res
        rows = model._lookup_device(uniq, "user")
        known = rows >= 0
        n_known = n if self.cold_start_strategy == "drop" else int(known.sum().item())
        pred_len = None
        excl = self._exclusion("user", exclude) if exclude is not None else None

        def lists(r):
            """(ids, lens) of the rows' lists; lens None: every list is full."""
            if excl is None:
                return model.recommend("user", r, k, diversify=diversify)[0], None
            top, _, lens = model.recommend("user", r, k, exclude=excl, diversify=diversify)
            return top, lens

        if n_known == n:
            pred, pred_len = lists(rows)
        else:  # "nan": an unknown user keeps its row, with an empty list
            top, top_len = lists(rows[known])
            pred = torch.zeros((n, max(int(top.shape[1]), 1)), dtype=torch.int64, device=dev)
            pred[known, : top.shape[1]] = top
            pred_len = torch.zeros(n, dtype=torch.int32, device=dev)
            pred_len[known] = int(top.shape[1]) if top_len is None else top_len
        res.update(ranked_lists.ranking_means(pred, pred_len, indptr, labels, k, n, self.RANKING_METRIC_NAMES))
        return res

    def evaluate_ranking(self, data, metric_name="meanAveragePrecision", k=10, label_col=None, min_rating=None,
                         exclude=None, diversify=None):
        """Spark's RankingEvaluator(metricName=metric_name, k=k).evaluate of
        the model's lists for the users of `data` (a float); exclude and
        diversify as in ranking_metrics."""
        ranked_lists.check_metric_name(metric_name, self.RANKING_METRIC_NAMES)
        return float(self.ranking_metrics(data, k, label_col, min_rating, exclude, diversify)[metric_name])

    # ------------------------------------------------------------ list quality
    # What the served lists look like as a whole: coverage, concentration,
    # novelty, diversity. No labels and no counterpart in the reference:
    # failures raise.
    LIST_QUALITY_METRIC_NAMES = ranked_lists.LIST_QUALITY_NAMES
    LIST_QUALITY_ROWS = 1 << 16  # users of one recommend + hrec_list_quality sub-batch

    def list_quality_metrics(self, k=10, users=None, exclude=None, history=None, diversify=None):
        """The beyond-accuracy measures of the model's top-k item lists
        (recommend_for_all_users(k, exclude) / recommend_for_user_subset(users,
        k, exclude)), which never leave the device: {"catalogCoverage",
        "distributionalCoverage", "gini", "personalization",
        "intraListDiversity", "unexpectedness", "novelty", "averagePopularity",
        "count", "novelty_unseen", "dropped"} (ranked_lists.list_quality has
        the definitions). Cosines are taken between item factors. users: None
        (every user of the model), a DataFrame with a userId column or an
        array-like; ids the model does not know are left out and counted in
        "dropped". history (optional): a DataFrame with userId and itemId
        columns, typically the training frame (and the same one as exclude):
        novelty = the mean self-information log2(Hsum / h_i) of the listed
        items, h_i the frame's distinct pairs of item i; averagePopularity =
        the mean of h_i / the frame's distinct users; unexpectedness = one
        minus the mean cosine between a listed item and an item of the user's
        own history. Without it those three are NaN. diversify (optional):
        recommend_for_all_users' MMR; the measures are those of the
        diversified lists, which stay on the device."""
        import pandas as pd

        model = self._trained()
        if diversify is not None:
            ranked_lists.check_mmr(diversify)
        dev = model.U.device
        k = ranked_lists.check_num(k, model.RECOMMEND_MAX, "k")
        ids = np.asarray(model.user_ids, np.int64)
        dropped = 0
        if users is None:
            rows = np.arange(ids.size, dtype=np.int64)
        else:
            if isinstance(users, pd.DataFrame):
                users = users["userId"]
            rows = model._lookup(ids, np.unique(_int_ids(np.asarray(users).reshape(-1), "userId")))
            dropped = int((rows < 0).sum())
            rows = rows[rows >= 0]
        excl = self._exclusion("user", exclude) if exclude is not None else None
        hist = tables = None
        if history is not None:
            hist = excl if history is exclude else self._exclusion("user", history)
            tables = ranked_lists.history_tables(*ranked_lists.history_frame(history), model.item_ids, dev,
                                                 cols_sorted=True)

        def batches():
            for lo in range(0, rows.size, self.LIST_QUALITY_ROWS):
                r = torch.as_tensor(rows[lo: lo + self.LIST_QUALITY_ROWS], device=dev)
                cols, _, lens = model.recommend("user", r, k, exclude=excl, _columns=True, diversify=diversify)
                yield cols, lens, None if hist is None else (r, *hist)

        res = ranked_lists.list_quality(batches, model.V, model.k, k, tables)
        res["dropped"] = dropped
        return res

    def evaluate_list_quality(self, metric_name="catalogCoverage", k=10, users=None, exclude=None, history=None,
                              diversify=None):
        """One of list_quality_metrics' eight measures (a float)."""
        ranked_lists.check_metric_name(metric_name, self.LIST_QUALITY_METRIC_NAMES)
        return float(self.list_quality_metrics(k, users, exclude, history, diversify)[metric_name])

    # --------------------------------- positions in the full catalogue
    # Where every held-out item stands among ALL items of the model: what the
    # lists above, cut at 1024, cannot say. Expected percentile rank is the
    # measure of Hu, Koren and Volinsky's paper (Spark's implicitPrefs), AUC
    # and the uncut reciprocal rank the usual companions. No counterpart in the
    # reference: failures raise.
    FULL_RANKING_METRIC_NAMES = ranked_lists.FULL_RANK_NAMES

    def _full_rank(self, users, items, weights, exclude):
        """(rank per pair, metrics with "dropped") of ranked_lists.full_rank_metrics over the model's items."""
        model, dev = self._trained(), self.model.U.device
        if self.cold_start_strategy not in ("drop", "nan"):
            raise ValueError(f"coldStartStrategy {self.cold_start_strategy!r} is not supported")
        item_ids = np.asarray(model.item_ids, np.int64)
        user_ids = np.asarray(model.user_ids, np.int64)
        n_items = int(item_ids.size)
        excl = self._exclusion("user", exclude) if exclude is not None else None

        def scores(uids):
            urows = torch.as_tensor(model._lookup(user_ids, uids), device=dev)
            kw = dict(scores=_hrec.als_score(model.U, urows, model.Vt, None, n_items, model.k), source="f32")
            if excl is not None:
                kw["excl"] = (urows, *excl)
            return kw

        rank, res = ranked_lists.full_rank_metrics(
            users, items, weights, item_ids, dev, scores, 4, model.RECOMMEND_FALLBACK_BYTES,
            known=lambda uniq: model._lookup(user_ids, uniq) >= 0, cols_sorted=True,
            host_rows=self.RANKING_HOST_ROWS)
        return rank, res

    def _known_users(self, users):
        """bool per entry of `users` (int64 numpy): the model knows the id (long lists: looked up on the device)."""
        model = self.model
        if users.size > model.PAIR_DEVICE_LOOKUP:
            return (model._lookup_device(users, "user") >= 0).cpu().numpy()
        return model._lookup(np.asarray(model.user_ids, np.int64), users) >= 0

    def rank_of(self, data, exclude=None):
        """A copy of `data` (columns userId, itemId) with an int64 `rank`
        column: the 0-based position of the row's item among ALL items of the
        model in the user's ranking — larger transform prediction first, equal
        predictions by smaller itemId — without the pairs of `exclude` (a frame
        with userId and itemId, typically the training frame). For any n <=
        1024, rank < n holds exactly when the item stands at position rank of
        the user's list from recommend_for_user_subset(n, exclude). -1: the
        pair cannot be ranked (the user or the item is unknown to the model,
        or the pair is excluded). cold_start_strategy "drop" removes the rows
        of unknown users (order and index kept), "nan" keeps them. The scores
        (hrec_als_score, transform's bits) and the counting (hrec_rank_positions)
        stay on the device."""
        users, items = self._pair_ids(data)
        rank, _ = self._full_rank(users, items, None, exclude)
        out = ranked_lists.rank_frame(data, rank)
        if self.cold_start_strategy == "drop":
            out = out[self._known_users(users)]
        return out

    def full_ranking_metrics(self, data, weight_col=None, min_rating=None, label_col=None, exclude=None):
        """The ranking measures that need every position, of the pairs of
        `data` (columns userId, itemId; with min_rating the rows whose
        label_col, default average_review_rating, is >= it) among ALL items of
        the model: {"meanPercentileRank", "auc", "meanReciprocalRank", "count",
        "pairs", "unranked", "dropped"}.
        meanPercentileRank: Hu, Koren and Volinsky's expected percentile rank,
        sum w * rank / (live - 1) / sum w over the ranked pairs, w = weight_col
        (finite and >= 0, else ValueError; 1 without) and live the user's items
        left after `exclude`; in [0, 1], lower is better, 0.5 is random. auc:
        the mean over users of the fraction of (held-out, other) item pairs
        ranked in the right order; meanReciprocalRank: the mean of 1 / (1 + the
        user's best rank), with no cut-off; both over the users where they are
        defined, `count` = the users with a ranked pair. Ties are resolved by
        the list order (smaller itemId first), not counted as 1/2: the AUC of
        the ranking that is served. `pairs` / `unranked`: the pairs that entered
        / could not enter. Unlike ranking_metrics' set size, an item the model
        does not know (or an excluded pair) cannot be ranked and enters no
        statistic. Users unknown to the model: cold_start_strategy "drop"
        leaves them out and counts them in `dropped`, "nan" keeps them with
        every pair unranked. Nothing ranked: NaN metrics."""
        self._pair_ids(data)
        users, items, weights = ranked_lists.full_rank_frame(data, weight_col, min_rating, label_col)
        dropped = 0
        if self.cold_start_strategy == "drop":
            known = self._known_users(users)
            dropped = int(np.unique(users[~known]).size)
            users, items = users[known], items[known]
            weights = None if weights is None else weights[known]
        _, res = self._full_rank(users, items, weights, exclude)
        res["dropped"] = dropped
        return res

    def evaluate_full_ranking(self, data, metric_name="meanPercentileRank", weight_col=None, min_rating=None,
                              label_col=None, exclude=None):
        """One of full_ranking_metrics' meanPercentileRank, auc,
        meanReciprocalRank (a float)."""
        ranked_lists.check_metric_name(metric_name, self.FULL_RANKING_METRIC_NAMES)
        return float(self.full_ranking_metrics(data, weight_col, min_rating, label_col, exclude)[metric_name])

    # ----------------------------------------------------------- persistence
    def save_model(self, model_path="models/als"):
        try:
            os.makedirs(os.path.dirname(model_path) or ".", exist_ok=True)
            self.model.save(model_path, {"userCol": "userId", "itemCol": "itemId", "predictionCol": "prediction",
                                         "coldStartStrategy": self.cold_start_strategy, "blockSize": 4096})
            metadata = {
                "rank": self.rank,
                "max_iter": self.max_iter,
                "reg_param": self.reg_param,
                "global_mean": self.global_mean,
                "item_features": self.item_features,
                "implicit_prefs": bool(self.implicit_prefs),
                "alpha": float(self.alpha),
                "nonnegative": bool(self.nonnegative),
            }
            with open(f"{model_path}_metadata.pkl", "wb") as f:
                pickle.dump(metadata, f)
            print(f"Model saved to {model_path}")
        except Exception as e:
            print(f"Saving error: {str(e)}")

    def load_model(self, model_path="models/als"):
        try:
            if not self.initialize_spark():
                raise RuntimeError("no device session")
            self.model = DeviceALSFactors.load(model_path, self.spark.device)
            with open(f"{model_path}_metadata.pkl", "rb") as f:
                metadata = pickle.load(f)  # written by save_model above (own format)
                self.rank = metadata["rank"]
                self.max_iter = metadata["max_iter"]
                self.reg_param = metadata["reg_param"]
                self.global_mean = metadata["global_mean"]
                self.item_features = metadata["item_features"]
                self.implicit_prefs = metadata.get("implicit_prefs", False)  # absent in older pickles
                self.alpha = metadata.get("alpha", 1.0)
                self.nonnegative = metadata.get("nonnegative", False)
            return self
        except Exception as e:
            print(f"Loading error: {str(e)}")
            return None


def hyperparameter_tuning(train_data, val_data, param_grid):
    """src/als_model.py:142-169 (driver loop over the device ALS)."""
    best_params = None
    best_f1 = 0.0
    for params in param_grid:
        model = ALSModel(**params)
        if not model.train(train_data):
            continue
        f1_scores = []
        for user_id in val_data["userId"].sample(50).unique():
            sel = val_data[val_data["userId"] == user_id]
            actual = dict(zip(sel["itemId"], sel["average_review_rating"]))
            preds = model.predict_for_user(user_id, val_data["itemId"].unique())
            f1_scores.append(compute_f1_score(actual, {item: score for item, score in preds}))
        avg_f1 = np.mean(f1_scores)
        if avg_f1 > best_f1:
            best_f1 = avg_f1
            best_params = params.copy()
        model.stop_spark()
    return best_params


def compute_f1_score(actual, pred, k=10):
    """src/als_model.py:171-177 (k = 0 raises ZeroDivisionError, as there)."""
    actual_items = set(actual.keys())
    pred_items = set(item for item, _ in sorted(pred.items(), key=lambda x: x[1], reverse=True)[:k])
    tp = len(actual_items & pred_items)
    precision = tp / k
    recall = tp / len(actual_items) if actual_items else 0
    return 2 * (precision * recall) / (precision + recall) if (precision + recall) > 0 else 0
