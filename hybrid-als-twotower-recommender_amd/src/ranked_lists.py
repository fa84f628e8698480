"""What the ALS, the two-tower and the hybrid model share around their ranked
lists: the exclusion CSR of seen pairs, the label CSR, the ranking metrics of
a frame (ranking_metrics: the two-tower and hybrid body) and their tail, list
finishing (padding, the DataFrame of tuples) and the argument checks. Plain functions over numpy arrays and device tensors; the models keep
their own operands, thresholds (passed in, read at call time) and scoring
routes. The materialised top-k of the last resort is _hrec.topk_materialised.
"""
import numpy as np
import torch

from . import _hrec


def check_num(num, limit, name="num"):
    """int(num), in [1, limit]."""
    num = int(num)
    if not 1 <= num <= limit:
        raise ValueError(f"{name} must be in [1, {limit}] (got {num})")
    return num


def int_ids(col, name):
    a = np.asarray(col)
    if a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or not np.all(a == np.floor(a)):
            raise ValueError(f"{name} must hold integer ids (Spark casts them to Int)")
        a = a.astype(np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integer ids, got dtype {a.dtype}")
    a = a.astype(np.int64)
    if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
        raise ValueError(f"{name} ids must fit a 32-bit Int (Spark ALS)")
    return a


def check_metric_name(metric_name, names):
    if metric_name not in names:
        raise ValueError(f"metric_name must be one of {', '.join(names)} (got {metric_name!r})")


# ------------------------------------------------------------ exclusion CSR
# (row_keys, col_keys, excl_rows, excl_cols) -> (indptr int64 [len(row_keys) +
# 1], cols int32): row q holds the positions in col_keys of the ids paired
# with row_keys[q], ascending and distinct. row_keys: int64, ascending,
# distinct. col_keys: int64, distinct, in any order (cols_sorted: ascending,
# which saves the sort). Pairs with a key outside either list are dropped.
def exclusion_csr_host(row_keys, col_keys, excl_rows, excl_cols, cols_sorted=False, what="excl_rows and excl_cols"):
    """Pure numpy."""
    row_keys, col_keys, er, ec = (np.asarray(a, np.int64).reshape(-1)
                                  for a in (row_keys, col_keys, excl_rows, excl_cols))
    if er.size != ec.size:
        raise ValueError(f"{what} must have the same length")
    n_rows, n_cols = row_keys.size, col_keys.size
    indptr = np.zeros(n_rows + 1, np.int64)
    if n_rows == 0 or n_cols == 0 or er.size == 0:
        return indptr, np.zeros(0, np.int32)
    order = None if cols_sorted else np.argsort(col_keys, kind="stable")  # sorted position -> position in col_keys
    sorted_cols = col_keys if cols_sorted else col_keys[order]
    pc = np.minimum(np.searchsorted(sorted_cols, ec), n_cols - 1)
    pr = np.minimum(np.searchsorted(row_keys, er), n_rows - 1)
    ok = (sorted_cols[pc] == ec) & (row_keys[pr] == er)
    key = np.unique(pr[ok] * n_cols + (pc[ok] if cols_sorted else order[pc[ok]]))  # ascending: by row, then by column
    np.cumsum(np.bincount(key // n_cols, minlength=n_rows), out=indptr[1:])
    return indptr, (key % n_cols).astype(np.int32)


def exclusion_csr_device(row_keys, col_keys, excl_rows, excl_cols, dev, cols_sorted=False,
                         what="excl_rows and excl_cols"):
    """exclusion_csr_host on the device (one sort of 64-bit keys, and one of
    col_keys unless cols_sorted); any of the four may already be a device
    tensor."""
    row_keys, col_keys, er, ec = (torch.as_tensor(a, dtype=torch.int64, device=dev).reshape(-1)
                                  for a in (row_keys, col_keys, excl_rows, excl_cols))
    if er.numel() != ec.numel():
        raise ValueError(f"{what} must have the same length")
    n_rows, n_cols = row_keys.numel(), col_keys.numel()
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    if n_rows == 0 or n_cols == 0 or er.numel() == 0:
        return indptr, torch.zeros(0, dtype=torch.int32, device=dev)
    sorted_cols, order = (col_keys, None) if cols_sorted else torch.sort(col_keys, stable=True)
    pc = torch.searchsorted(sorted_cols, ec).clamp_(max=n_cols - 1)
    pr = torch.searchsorted(row_keys, er).clamp_(max=n_rows - 1)
    ok = (sorted_cols[pc] == ec) & (row_keys[pr] == er)
    key = torch.unique(pr[ok] * n_cols + (pc[ok] if cols_sorted else order[pc[ok]]))  # sorted
    del pc, pr, ok
    if key.numel():
        torch.cumsum(torch.bincount(torch.div(key, n_cols, rounding_mode="floor"), minlength=n_rows), 0,
                     out=indptr[1:])
    return indptr, torch.remainder(key, n_cols).to(torch.int32)


def exclusion_csr(row_keys, col_keys, excl_rows, excl_cols, dev, host_pairs, cols_sorted=False, device_keys=None,
                  what="excl_rows and excl_cols"):
    """The device (indptr, cols): built on the host up to host_pairs pairs,
    on the device above or when the pairs are device tensors already.
    device_keys (optional): the (row_keys, col_keys) copies a caller keeps on
    the device."""
    on_dev = isinstance(excl_rows, torch.Tensor) or isinstance(excl_cols, torch.Tensor)
    if not on_dev and np.asarray(excl_rows).size <= host_pairs:
        indptr, cols = exclusion_csr_host(row_keys, col_keys, excl_rows, excl_cols, cols_sorted, what)
        return torch.as_tensor(indptr, device=dev), torch.as_tensor(cols, device=dev)
    if device_keys is not None:
        row_keys, col_keys = device_keys()
    return exclusion_csr_device(row_keys, col_keys, excl_rows, excl_cols, dev, cols_sorted, what)


def distinct_counts(row_keys, pair_rows, pair_items, dev, host_rows):
    """int32 device [len(row_keys)]: how many distinct items the (row, item)
    pairs give row_keys[q] (int64, ascending, distinct; items fit 32 bits:
    int_ids'). Pairs with a row outside row_keys are dropped. On the host up
    to host_rows pairs, on the device above."""
    n = int(np.asarray(row_keys).size)
    if n == 0 or np.asarray(pair_rows).size == 0:
        return torch.zeros(n, dtype=torch.int32, device=dev)
    if np.asarray(pair_rows).size <= host_rows:
        rk, pr, pi = (np.asarray(a, np.int64).reshape(-1) for a in (row_keys, pair_rows, pair_items))
        pos = np.minimum(np.searchsorted(rk, pr), n - 1)
        ok = rk[pos] == pr
        key = np.unique((pos[ok] << 32) | (pi[ok] + (1 << 31)))  # one key per distinct (row, item)
        return torch.as_tensor(np.bincount(key >> 32, minlength=n).astype(np.int32), device=dev)
    rk, pr, pi = (torch.as_tensor(a, dtype=torch.int64, device=dev).reshape(-1)
                  for a in (row_keys, pair_rows, pair_items))
    pos = torch.searchsorted(rk, pr).clamp_(max=n - 1)
    ok = rk[pos] == pr
    key = torch.unique((pos[ok] << 32) | (pi[ok] + (1 << 31)))
    return torch.bincount(key >> 32, minlength=n).to(torch.int32)


# ---------------------------------------------------------------- label CSR
def label_csr_host(users, items, dev):
    """(distinct users, indptr, labels) of the (user, item) rows, int64
    device tensors: users ascending, a user's items ascending (duplicates
    stay; the kernel counts them once)."""
    order = np.lexsort((items, users))
    u, labels = users[order], items[order]
    first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]]) if len(u) else np.zeros(0, np.int64)
    indptr = np.r_[first, len(u)].astype(np.int64)
    return tuple(torch.as_tensor(np.ascontiguousarray(a, np.int64), device=dev) for a in (u[first], indptr, labels))


def label_csr_device(users, items, dev):
    """label_csr_host with the sorts on the device (two stable sorts)."""
    u, it = torch.as_tensor(users, device=dev), torch.as_tensor(items, device=dev)
    it, order = torch.sort(it, stable=True)
    u, order = torch.sort(u[order], stable=True)
    uniq, counts = torch.unique_consecutive(u, return_counts=True)
    indptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=indptr[1:])
    return uniq, indptr, it[order].contiguous()


def label_csr(users, items, dev, host_rows):
    """On the host for frames up to host_rows rows, on the device above."""
    return (label_csr_host if users.size <= host_rows else label_csr_device)(users, items, dev)


# -------------------------------------------------------------- metric tail
def ranking_means(pred, pred_len, indptr, labels, k, n, names):
    """{name: mean over the n label rows} of Spark's five ranking metrics
    (names in the order MAP, MAP@k, precision@k, recall@k, NDCG@k) for the
    device lists pred (lens pred_len, None: all full) against the label CSR:
    hrec_ranking_metrics and one host read."""
    sums, unsorted, _ = _hrec.ranking_metrics(pred, indptr, labels, k, pred_len=pred_len,
                                              pred_len_max=int(pred.shape[1]) if pred.numel() else 0)
    s = torch.cat([sums, unsorted.to(torch.float64)]).tolist()  # one host read
    if s[-1] != 0.0:
        raise RuntimeError("ranking_metrics: a label row is not sorted ascending")
    s = dict(zip(_hrec.RANK_SUMS, s))
    if int(s["n_rows"]) != n:
        raise RuntimeError(f"ranking_metrics: {int(s['n_rows'])} rows evaluated, {n} expected")
    return {name: s[slot] / n
            for name, slot in zip(names, ("sum_ap", "sum_ap_k", "sum_precision", "sum_recall", "sum_ndcg"))}


def ranking_metrics(data, k, label_col, min_rating, dev, host_rows, names, lists):
    """{name: mean, "count": n} over the frame `data` (userId, itemId; with
    min_rating, the rows whose label_col is >= it): the label CSR, the device
    lists(users, k) -> (pred, pred_len) of its n distinct users (ascending),
    ranking_means. n == 0: NaN metrics, `lists` is not called."""
    k = check_num(k, _hrec.RANK_MAX, "k")
    users, items = int_ids(data["userId"], "userId"), int_ids(data["itemId"], "itemId")
    if min_rating is not None:
        keep = np.asarray(data[label_col or "average_review_rating"], np.float64) >= float(min_rating)
        users, items = users[keep], items[keep]
    uniq, indptr, labels = label_csr(users, items, dev, host_rows)
    n = int(uniq.numel())
    res = dict({name: float("nan") for name in names}, count=n)
    if n:
        res.update(ranking_means(*lists(uniq.cpu().numpy(), k), indptr, labels, k, n, names))
    return res


# ------------------------------------------- positions in the full catalogue
# What a list cut at 1024 cannot say: where every held-out item stands among
# ALL candidates (hrec_rank_positions), and the three measures that need it.
FULL_RANK_NAMES = ("meanPercentileRank", "auc", "meanReciprocalRank")


def full_rank_frame(data, weight_col=None, min_rating=None, label_col=None):
    """(users, items int64, weights f64 or None) of a frame with userId and
    itemId: the rows whose label_col (default average_review_rating) is >=
    min_rating when given. Weights must be finite and >= 0."""
    users, items = int_ids(data["userId"], "userId"), int_ids(data["itemId"], "itemId")
    weights = None if weight_col is None else np.asarray(data[weight_col], np.float64).reshape(-1)
    if weights is not None and (not np.all(np.isfinite(weights)) or np.any(weights < 0)):
        raise ValueError(f"{weight_col} must hold finite weights >= 0")
    if min_rating is not None:
        keep = np.asarray(data[label_col or "average_review_rating"], np.float64) >= float(min_rating)
        users, items = users[keep], items[keep]
        weights = None if weights is None else weights[keep]
    return users, items, weights


def _full_rank_csr_host(users, items, weights, col_keys, cols_sorted, dev):
    """The label CSR of full_rank_metrics, sorted on the host: (distinct users
    ascending (numpy), indptr int64, cols int32 (-1: not a candidate), weights
    f64 or None on the device, unsort: device ranks in CSR order -> numpy int64
    in frame order). A user's entries keep frame order (a stable sort)."""
    n_pairs, n = int(users.size), int(col_keys.size)
    order = np.argsort(users, kind="stable")
    u = users[order]
    first = np.flatnonzero(np.r_[True, u[1:] != u[:-1]])
    indptr = np.r_[first, n_pairs].astype(np.int64)
    if cols_sorted:
        sorted_keys, back = col_keys, None
    else:
        back = np.argsort(col_keys, kind="stable")
        sorted_keys = col_keys[back]
    it = items[order]
    pos = np.minimum(np.searchsorted(sorted_keys, it), n - 1)
    cols = np.where(sorted_keys[pos] == it, pos if back is None else back[pos], -1).astype(np.int32)
    d_weight = None if weights is None else torch.as_tensor(np.ascontiguousarray(weights[order], np.float64), device=dev)

    def unsort(d_rank):
        rank = np.empty(n_pairs, np.int64)
        rank[order] = d_rank.cpu().numpy()
        return rank

    return u[first], torch.as_tensor(indptr, device=dev), torch.as_tensor(cols, device=dev), d_weight, unsort


def _full_rank_csr_device(users, items, weights, col_keys, cols_sorted, dev):
    """_full_rank_csr_host with the sort and the searches on the device."""
    n_pairs, n = int(users.size), int(col_keys.size)
    u, order = torch.sort(torch.as_tensor(users, device=dev), stable=True)
    uniq, counts = torch.unique_consecutive(u, return_counts=True)
    indptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=indptr[1:])
    keys = torch.as_tensor(col_keys, device=dev)
    sorted_keys, back = (keys, None) if cols_sorted else torch.sort(keys, stable=True)
    it = torch.as_tensor(items, device=dev)[order]
    pos = torch.searchsorted(sorted_keys, it).clamp_(max=n - 1)
    cols = torch.where(sorted_keys[pos] == it, pos if back is None else back[pos], torch.full_like(pos, -1))
    d_weight = None if weights is None else torch.as_tensor(weights, dtype=torch.float64, device=dev)[order].contiguous()

    def unsort(d_rank):
        rank = torch.empty(n_pairs, dtype=torch.int64, device=dev)
        rank[order] = d_rank.to(torch.int64)
        return rank.cpu().numpy()

    return uniq.cpu().numpy(), indptr, cols.to(torch.int32).contiguous(), d_weight, unsort


def full_rank_metrics(users, items, weights, col_keys, dev, scores, row_bytes, max_bytes, known=None,
                      cols_sorted=False, max_rows=1 << 20, host_rows=1 << 16):
    """The positions of the (users[p], items[p]) pairs among all candidates,
    and their metrics. col_keys: the candidates' ids (int64, distinct), position
    = score column; an item outside them is unranked. The label CSR holds one
    row per distinct user (ascending), a user's entries in frame order with
    their weights; it is built on the host for frames up to host_rows rows, on
    the device above. The users with known(uniq) true (None: all) go in
    sub-batches of at most max_bytes // (row_bytes * n) rows through
    scores(user_ids) -> the keyword arguments of _hrec.rank_positions for those
    rows (scores, source, ..., excl with one excl_rows entry per row); the
    other users' pairs are unranked. The sums stay on the device until one
    host read at the end. Returns (rank int64 per pair (-1: unranked),
    {"meanPercentileRank", "auc", "meanReciprocalRank", "count", "pairs",
    "unranked"}): meanPercentileRank = sum w * rank / (live - 1) / sum w over
    the ranked pairs (Hu, Koren and Volinsky's expected percentile rank: 0 is
    best, 0.5 random), auc and meanReciprocalRank the means over the users
    where they are defined, count those users (of the reciprocal rank: the
    users with a ranked pair), pairs the ranked pairs. Ties are resolved by the
    list order, not counted as 1/2. Nothing ranked: NaN metrics."""
    users, items = np.asarray(users, np.int64).reshape(-1), np.asarray(items, np.int64).reshape(-1)
    col_keys = np.asarray(col_keys, np.int64).reshape(-1)
    n_pairs, n = int(users.size), int(col_keys.size)
    res = dict({name: float("nan") for name in FULL_RANK_NAMES}, count=0, pairs=0, unranked=n_pairs)
    rank = np.full(n_pairs, -1, np.int64)
    if n_pairs == 0 or n == 0:
        return rank, res
    build = _full_rank_csr_host if n_pairs <= host_rows else _full_rank_csr_device
    uniq, d_indptr, d_cols, d_weight, unsort = build(users, items, weights, col_keys, cols_sorted, dev)
    rows = np.arange(uniq.size, dtype=np.int64)
    if known is not None:
        rows = rows[np.asarray(known(uniq), bool)]
    d_rank = torch.full((n_pairs,), -1, dtype=torch.int32, device=dev)
    total = torch.zeros(len(_hrec.RP_SUMS), dtype=torch.float64, device=dev)
    sub = int(max(1, min(max_rows, max_bytes // (row_bytes * n))))
    for lo in range(0, rows.size, sub):
        q = rows[lo: lo + sub]
        kw = scores(uniq[q])
        _, _, _, sums = _hrec.rank_positions(labels=(torch.as_tensor(q, device=dev), d_indptr, d_cols),
                                             weight=d_weight, out_rank=d_rank, **kw)
        total += sums
    s = dict(zip(_hrec.RP_SUMS, total.tolist()))  # one host read
    rank = unsort(d_rank)
    res.update(count=int(s["n_reciprocal_rank"]), pairs=int(s["ranked"]), unranked=n_pairs - int(s["ranked"]))
    if s["ranked"] > 0:
        res["meanPercentileRank"] = s["sum_w_pr"] / s["sum_w"] if s["sum_w"] > 0 else float("nan")
        res["auc"] = s["sum_auc"] / s["n_auc"] if s["n_auc"] > 0 else float("nan")
        res["meanReciprocalRank"] = s["sum_reciprocal_rank"] / s["n_reciprocal_rank"]
    return rank, res


def rank_frame(data, rank):
    """A copy of `data` with the int64 `rank` column (-1: unranked)."""
    out = data.copy()
    out["rank"] = np.asarray(rank, np.int64)
    return out


# ------------------------------------------------------------- list quality
# What the served lists look like as a whole (hrec_list_quality): how much of
# the catalogue they reach, how concentrated the exposure is, how novel, how
# diverse and how unexpected the lists are. No labels: nothing here says whether
# a list is right.
LIST_QUALITY_NAMES = ("catalogCoverage", "distributionalCoverage", "gini", "personalization", "intraListDiversity",
                      "unexpectedness", "novelty", "averagePopularity")


def history_frame(history):
    """(users, items) int64 of a history frame (columns userId, itemId)."""
    return int_ids(history["userId"], "userId"), int_ids(history["itemId"], "itemId")


def history_tables(users, items, col_keys, dev, cols_sorted=False):
    """The two per-candidate tables of a history frame's (users[p], items[p])
    pairs, f64 device [2, n]: with h_i the distinct pairs of candidate i
    (col_keys[i]; over all users of the frame) and Hsum their total, row 0 =
    log2(Hsum / h_i) (the self-information of i; NaN where h_i = 0), row 1 =
    h_i / the frame's distinct users. One sort of 64-bit keys on the device."""
    n = int(np.asarray(col_keys).size)
    u = torch.as_tensor(np.asarray(users, np.int64).reshape(-1), device=dev)
    it = torch.as_tensor(np.asarray(items, np.int64).reshape(-1), device=dev)
    h = torch.zeros(n, dtype=torch.int64, device=dev)
    n_users = 0
    if n and u.numel():
        keys = torch.as_tensor(np.asarray(col_keys, np.int64).reshape(-1), device=dev)
        sorted_keys, back = (keys, None) if cols_sorted else torch.sort(keys, stable=True)
        pos = torch.searchsorted(sorted_keys, it).clamp_(max=n - 1)
        ok = sorted_keys[pos] == it
        uniq, urank = torch.unique(u, return_inverse=True)
        n_users = int(uniq.numel())
        col = pos[ok] if back is None else back[pos[ok]]
        pair = torch.unique(urank[ok] * n + col)  # one key per distinct (user, candidate)
        if pair.numel():
            h = torch.bincount(torch.remainder(pair, n), minlength=n)
    hf = h.to(torch.float64)
    novelty = torch.where(h > 0, torch.log2(hf.sum() / hf.clamp(min=1.0)), torch.full_like(hf, float("nan")))
    return torch.stack([novelty, hf / max(n_users, 1)]).contiguous()


def list_quality(batches, vectors, d, k, tables=None):
    """The list-quality measures of the lists batches() yields, one sub-batch
    at a time: (columns int64 device [b, L <= 1024]: candidate columns, what a
    top-k returns before the id gather; lens int32 [b] or None: every list
    full; history: (rows int64 [b] (-1: none), indptr, cols) of an exclusion
    CSR, or None). vectors f32 device [n, >= d]: the candidates' vectors, the
    first d columns; tables: history_tables' pair or None; k: the list length
    asked for. hrec_row_inv_norms once, hrec_list_quality per sub-batch with
    the exposure counters and the sums accumulating on the device, then torch
    ops on the [n] exposure vector and ONE host read. With c_i the exposure of
    candidate i, T their total, U the lists with an entry and N = n:
      catalogCoverage = #{c_i > 0} / N;
      distributionalCoverage = -sum_{c_i > 0} (c_i / T) log2(c_i / T) (bits);
      gini = sum_j (2 j - N - 1) c_(j) / (N T), c ascending, j = 1 .. N: 0 for
        equal exposure, (N - 1) / N with all of it on one item;
      personalization = 1 - [sum_i c_i (c_i - 1) / 2] / [U (U - 1) / 2 * k]: one
        minus the mean overlap of two users' lists (NaN when U < 2);
      intraListDiversity, unexpectedness, novelty, averagePopularity: the means
        of the kernel's per-list columns over the lists where each is defined
        (the last three NaN without history / tables);
      count = U; novelty_unseen = the list entries whose item has no history
        pair (left out of novelty).
    The integer sums are exact (below 2^53). Nothing recommended: NaN metrics."""
    dev = vectors.device
    n = int(vectors.shape[0])
    res = dict({name: float("nan") for name in LIST_QUALITY_NAMES}, count=0, novelty_unseen=0)
    if n == 0:
        return res
    n_tab = 0 if tables is None else int(tables.shape[0])
    ncol = 2 + n_tab
    inv = _hrec.row_inv_norms(vectors, d)
    exposure = torch.zeros(n, dtype=torch.int64, device=dev)
    sums = torch.zeros(2 * ncol, dtype=torch.float64, device=dev)
    users = torch.zeros((), dtype=torch.int64, device=dev)
    for cols, lens, hist in batches():
        if cols.shape[0] == 0:
            continue
        _, row_n, _, _ = _hrec.list_quality(cols, vectors, inv, list_len=lens, history=hist, tables=tables,
                                            exposure=exposure, sums=sums, d=d)
        users += (row_n[:, 0] > 0).sum()
    c = exposure
    total = c.sum()
    j = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
    gini_num = ((2 * j - n - 1) * torch.sort(c).values).sum()
    p = c[c > 0].to(torch.float64) / total.to(torch.float64)
    entropy = -(p * torch.log2(p)).sum()
    pairs = torch.div(c * (c - 1), 2, rounding_mode="floor").to(torch.float64).sum()
    unseen = (c * torch.isnan(tables[0])).sum() if n_tab else torch.zeros_like(total)
    ints = torch.stack([users, total, (c > 0).sum(), gini_num, unseen]).to(torch.float64)
    host = torch.cat([ints, torch.stack([entropy, pairs]), sums]).tolist()  # one host read
    n_users, total, reached, gini_num, unseen = (int(x) for x in host[:5])
    entropy, pairs = host[5:7]
    s = host[7:]
    if n_users == 0:
        return res
    means = [s[i] / s[ncol + i] if s[ncol + i] > 0 else float("nan") for i in range(ncol)]
    res.update(catalogCoverage=reached / n, distributionalCoverage=entropy, gini=gini_num / (n * total),
               personalization=1.0 - pairs / (n_users * (n_users - 1) / 2 * k) if n_users >= 2 else float("nan"),
               intraListDiversity=means[0], unexpectedness=means[1], count=n_users, novelty_unseen=unseen)
    if n_tab >= 2:
        res.update(novelty=means[2], averagePopularity=means[3])
    return res


def lists_frame_columns(lists, item_ids):
    """(columns int64 numpy [n_lists, L], lens int32 numpy) of a lists frame's
    `recommendations` column (lists of (itemId, rating) tuples) over the
    candidates item_ids (int64, distinct): an id outside them becomes -1."""
    recs = list(lists["recommendations"])
    item_ids = np.asarray(item_ids, np.int64).reshape(-1)
    width = max([len(r) for r in recs], default=0)
    cols = np.full((len(recs), width), -1, np.int64)
    lens = np.array([len(r) for r in recs], np.int32)
    if width and item_ids.size:
        order = np.argsort(item_ids, kind="stable")
        sorted_ids = item_ids[order]
        flat = np.array([int(i) for r in recs for i, _ in r], np.int64)
        pos = np.minimum(np.searchsorted(sorted_ids, flat), item_ids.size - 1)
        col = np.where(sorted_ids[pos] == flat, order[pos], -1)
        cols[np.arange(width)[None, :] < lens[:, None]] = col
    return cols, lens


# ------------------------------------------------- diversity-aware re-ranking
# Greedy Maximal Marginal Relevance (Carbonell and Goldstein 1998): the model
# ranks a longer pool, hrec_mmr_rerank picks the final list from it so that
# each pick trades its relevance against its similarity to the picks before.
class MMR:
    """The `diversify=` argument of the list APIs. lambda_ in [0, 1]: 1 keeps
    the model's ranking, 0 looks at similarity alone (after the first pick);
    pool in [1, 1024]: how many of the model's best candidates the selection
    chooses from (at least the list length asked for is always ranked)."""

    POOL_MAX = _hrec.MMR_POOL_MAX

    def __init__(self, lambda_=0.7, pool=100):
        lambda_ = float(lambda_)
        if not 0.0 <= lambda_ <= 1.0:  # NaN fails too
            raise ValueError(f"lambda_ must be in [0, 1] (got {lambda_})")
        self.lambda_ = lambda_
        self.pool = check_num(pool, self.POOL_MAX, "pool")

    def __repr__(self):
        return f"MMR(lambda_={self.lambda_}, pool={self.pool})"


def check_mmr(mmr):
    if not isinstance(mmr, MMR):
        raise TypeError(f"diversify must be an MMR (got {type(mmr).__name__})")
    return mmr


def diversify(cols, scores, lens, vectors, inv, d, mmr, num):
    """The MMR selection of `num` entries from every row's pool: cols int64
    device [n, P <= 1024] candidate columns best first (what a top-k returns
    before the id gather), scores f32 / f64 [n, P] their ratings, lens int32
    [n] or None (every pool full). vectors f32 device [candidates, >= d], inv
    = _hrec.row_inv_norms(vectors, d) (None: made here). Returns (cols [n,
    kk], scores [n, kk], lens int32 [n]), kk = min(num, P), in SELECTION order
    (not descending by score); a score keeps its bits; past a list's length
    column -1 and score NaN. hrec_mmr_rerank, then two torch.gather."""
    mmr = check_mmr(mmr)
    n, pool_n = int(cols.shape[0]), int(cols.shape[1])
    kk = min(int(num), pool_n)
    if n == 0 or kk == 0:
        return cols[:, :kk], scores[:, :kk], torch.zeros(n, dtype=torch.int32, device=cols.device)
    if inv is None:
        inv = _hrec.row_inv_norms(vectors, d)
    pos, out_len, _ = _hrec.mmr_rerank(cols, scores, vectors, inv, mmr.lambda_, kk, pool_len=lens, d=d)
    live = pos >= 0
    at = pos.clamp(min=0).to(torch.int64)
    out_cols = torch.where(live, torch.gather(cols, 1, at), torch.full_like(at, -1))
    out_scores = torch.gather(scores, 1, at)
    return out_cols, torch.where(live, out_scores, torch.full_like(out_scores, float("nan"))), out_len


def diversify_finish(id_table, cols, scores, lens, n_cols, columns, with_lens):
    """What a model's recommend returns for diversify()'s lists: the triple as
    it is (columns), or (raw ids, scores, lens or None), padded as pad_lists
    does."""
    if columns:
        return cols, scores, lens
    ids, scores = pad_lists(id_table, cols.clone(), scores, lens, n_cols)
    return ids, scores, (lens if with_lens else None)


# ----------------------------------------------------------- list finishing
def empty_lists(n, kk, dtype, dev, with_lens):
    """The (ids, scores, lens) of n lists of kk entries when either is 0."""
    return (torch.zeros((n, kk), dtype=torch.int64, device=dev), torch.zeros((n, kk), dtype=dtype, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev) if with_lens else None)


def pad_lists(id_table, idx, val, lens, n_cols):
    """(raw ids, scores) of the lists idx / val with id 0 and score NaN past
    each list's length (what the library left there is unspecified)."""
    kk = idx.shape[1]
    live = torch.arange(kk, device=idx.device).unsqueeze(0) < lens.unsqueeze(1)
    ids = torch.where(live, id_table[idx.clamp_(0, n_cols - 1)], torch.zeros_like(idx))
    return ids, torch.where(live, val, torch.full_like(val, float("nan")))


def lists_frame(key_col, keys, ids, val, lens=None):
    """The DataFrame (key_col, recommendations): per key its list of (id,
    rating) tuples from the device lists ids / val, cut to lens when given."""
    import pandas as pd

    ids, val = ids.cpu().numpy().tolist(), val.cpu().numpy().tolist()
    recs = [list(zip(i, s)) for i, s in zip(ids, val)]
    if lens is not None:  # each list cut to its length
        recs = [rec[:m] for rec, m in zip(recs, lens.cpu().numpy().tolist())]
    return pd.DataFrame({key_col: keys, "recommendations": recs})


# -------------------------------------------------------- cosine neighbours
# "More like this" (hrec_cosine_topk): the rows of one matrix
# ranked by their cosine to a query row of the same matrix.
SIMILAR_BATCH = 4096  # queries of one hrec_cosine_topk call
SIMILAR_WS_BYTES = 1 << 30  # a call's workspace stays below this (while a batch of one query allows)
SIMILAR_MAX = _hrec.COSINE_TOP_MAX


def similar(vectors, d, query_rows, num, min_similarity=None, skip_self=True, mode=0, stats=None):
    """The `num` nearest rows of `vectors` (f32 device [n, >= d], the first d
    columns) by cosine for every query row (int64, numpy or device: rows of
    the same matrix; outside [0, n): no list): device (columns int64 [n_q,
    num] best first, -1 past a list's length; sims f64, NaN there; lens int32
    [n_q]). Equal cosines keep the smaller column, the query itself is left
    out (skip_self), min_similarity (None: no cut) keeps cosines above it.
    hrec_row_inv_norms and the pruned arm's operand once, then sub-batches of
    SIMILAR_BATCH queries (fewer where the workspace would pass
    SIMILAR_WS_BYTES); a batch whose pruned arm raised its flag is redone in
    the exhaustive arm, in the same workspace, and under mode 0 (auto) every
    batch after it takes the exhaustive arm directly: at most one pruned pass
    is wasted on vectors the margin cannot prune. mode: 0 / "auto", 1 /
    "exhaustive", 2 / "pruned". stats (a dict, optional) counts batches and
    flagged."""
    num = check_num(num, SIMILAR_MAX)
    dev = vectors.device
    q = torch.as_tensor(query_rows, dtype=torch.int64, device=dev).reshape(-1).contiguous()
    n, n_q = int(vectors.shape[0]), int(q.numel())
    cols = torch.full((n_q, num), -1, dtype=torch.int64, device=dev)
    sims = torch.full((n_q, num), float("nan"), dtype=torch.float64, device=dev)
    lens = torch.zeros(n_q, dtype=torch.int32, device=dev)
    if n == 0 or n_q == 0:
        return cols, sims, lens
    mode = _hrec.COSINE_MODES.get(mode, mode)
    min_sim = float("-inf") if min_similarity is None else float(min_similarity)
    inv = _hrec.row_inv_norms(vectors, d)
    items = _hrec.cosine_items(vectors, inv, d) if mode != 1 else None
    def need(b):  # one workspace serves the arm asked for and the exhaustive redo of a flagged batch
        return max(_hrec.cosine_topk_workspace_bytes(b, n, num, d, mode),
                   _hrec.cosine_topk_workspace_bytes(b, n, num, d, 1))

    batch = min(SIMILAR_BATCH, n_q)
    while batch > 1 and need(batch) > SIMILAR_WS_BYTES:
        batch = (batch + 1) // 2
    ws = torch.empty(need(batch), dtype=torch.uint8, device=dev)
    for lo in range(0, n_q, batch):
        hi = min(lo + batch, n_q)
        i, v, m, raised = _hrec.cosine_topk(vectors, inv, q[lo:hi], num, skip_self=skip_self, min_sim=min_sim,
                                            mode=mode, items=items, d=d, ws=ws, want_overflow=True)
        cols[lo:hi], sims[lo:hi], lens[lo:hi] = i, v, m
        if stats is not None:
            stats["batches"] = stats.get("batches", 0) + 1
            stats["flagged"] = stats.get("flagged", 0) + int(raised)
        if raised and mode == 0:
            # vectors too concentrated for the margin to prune: the bound would cost every later batch a wasted
            # pass too, so the rest goes through the exhaustive arm (the same bits); an explicit mode 2 is kept
            mode = 1
    return cols, sims, lens


def similar_frame(key_col, keys, id_table, vectors, d, query_rows, num, min_similarity=None, mode=0):
    """similar() as a lists frame: per key its [(id, similarity: float)], best
    first, the ids gathered from id_table (int64 device, one per row of
    vectors) on the device."""
    cols, sims, lens = similar(vectors, d, query_rows, num, min_similarity, mode=mode)
    n = int(vectors.shape[0])
    if cols.numel() == 0 or n == 0:
        return lists_frame(key_col, keys, cols, sims, lens)
    ids, sims = pad_lists(id_table, cols, sims, lens, n)
    return lists_frame(key_col, keys, ids, sims, lens)


def similar_rows_frame(key_col, ids, vectors, d, queries, num, min_similarity=None, ids_dev=None):
    """similar_frame over the rows of `vectors` named by `ids` (int64,
    distinct, one per row, in any order). queries None: every row, in row
    order; a DataFrame with a key_col column or an array-like of ids: its
    distinct ids ascending, those outside `ids` left out. Equal similarities
    keep the earlier ROW first (the smaller id where ids ascend)."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    if int(vectors.shape[0]) != ids.size:
        raise ValueError(f"ids must name every row of vectors ({ids.size} ids, {int(vectors.shape[0])} rows)")
    num = check_num(num, SIMILAR_MAX)
    if queries is None:
        rows = np.arange(ids.size, dtype=np.int64)
    else:
        if hasattr(queries, "columns"):
            queries = queries[key_col]
        keys = np.unique(int_ids(np.asarray(queries).reshape(-1), key_col))
        order = np.argsort(ids, kind="stable")
        pos = np.minimum(np.searchsorted(ids[order], keys), max(ids.size - 1, 0))
        rows = order[pos][ids[order][pos] == keys] if ids.size else np.zeros(0, np.int64)
    if ids_dev is None:
        ids_dev = torch.as_tensor(ids, device=vectors.device)
    return similar_frame(key_col, ids[rows], ids_dev, vectors, d, rows, num, min_similarity)


# ------------------------------------------------------- ALS explanations
# Why an ALS prediction is what it is (hrec_als_explain): a user
# row solves its normal equations, so a prediction is a sum of one term per
# entry of the user's history.
EXPLAIN_ROWS = 1 << 16  # kernel rows of one hrec_als_explain call


def rated_history_csr(users, items, ratings, item_rows, dev):
    """The rated history of a frame as a CSR over its distinct users: (user
    ids int64 numpy, sorted; indptr int64 device [n_users + 1]; cols int32
    device: item-factor rows; vals f32 device; dropped: the rows whose item is
    unknown). item_rows: int64 device, each row's item-factor row or -1. Rows
    of an unknown item are dropped; inside a user the others keep frame order,
    as in ALSModel.fold_in_users (the f64 sums depend on it)."""
    uniq, inv = np.unique(np.asarray(users, np.int64).reshape(-1), return_inverse=True)
    keep = item_rows >= 0
    inv_k = torch.as_tensor(np.ascontiguousarray(inv.reshape(-1)), device=dev)[keep]
    counts = torch.bincount(inv_k, minlength=int(uniq.size)) if uniq.size else torch.zeros(0, dtype=torch.int64,
                                                                                          device=dev)
    order = torch.sort(inv_k, stable=True).indices
    indptr = torch.zeros(int(uniq.size) + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(counts, 0)
    cols = item_rows[keep][order].to(torch.int32).contiguous()
    vals = torch.as_tensor(np.ascontiguousarray(np.asarray(ratings, np.float32).reshape(-1)),
                           device=dev)[keep][order].contiguous()
    return uniq, indptr, cols, vals, int(item_rows.numel()) - int(inv_k.numel())


def explain_lists(lists, list_len, hist_rows, csr, V, k, reg_param, top, implicit=False, alpha=0.0, yty=None,
                  U_rows=None):
    """hrec_als_explain over the rows of `lists` (int64 device [R, L <= 1024]
    item-factor rows; list_len int32 [R] or None) in sub-batches of
    EXPLAIN_ROWS: device (total f64 [R, L], pos int32 [R, L, top], val f64,
    len int32 [R, L], gap). hist_rows int64 [R]: each row's segment of csr =
    (indptr, cols, vals), -1: none. U_rows (optional, f32 [R, kp]): the stored
    factor row of each kernel row's user; gap is then the largest |row's own
    solve - stored row| over the rows with an explanation (a device scalar,
    0 when there is none)."""
    dev = V.device
    R, L = int(lists.shape[0]), int(lists.shape[1])
    total = torch.empty((R, L), dtype=torch.float64, device=dev)
    pos = torch.empty((R, L, top), dtype=torch.int32, device=dev)
    val = torch.empty((R, L, top), dtype=torch.float64, device=dev)
    length = torch.empty((R, L), dtype=torch.int32, device=dev)
    gap = torch.zeros((), dtype=torch.float32, device=dev)
    for s in range(0, R, EXPLAIN_ROWS):
        sl = slice(s, min(s + EXPLAIN_ROWS, R))
        t, p, v, n, row = _hrec.als_explain(
            lists[sl], (hist_rows[sl].contiguous(), *csr), V, k, reg_param, top, implicit=implicit, alpha=alpha,
            yty=yty, list_len=None if list_len is None else list_len[sl].contiguous(), want_row=U_rows is not None)
        total[sl], pos[sl], val[sl], length[sl] = t, p, v, n
        if U_rows is not None and L:
            used = (n > 0).any(dim=1)
            d = (row - U_rows[sl]).abs().amax(dim=1)
            d = torch.where(used, d, torch.zeros_like(d))
            if d.numel():
                gap = torch.maximum(gap, d.max())
    return total, pos, val, length, gap


def explain_tuples(pos, val, length, seg_start, entry_ids):
    """Host: per list entry its [(itemId, contribution), ...], largest first.
    pos / val / length: numpy [n, top] / [n, top] / [n] of n list entries;
    seg_start int64 [n]: where the entry's history segment starts in entry_ids
    (the raw item id of every history entry, int64 numpy)."""
    n, top = pos.shape
    live = np.arange(top)[None, :] < length[:, None]
    where = np.where(live, seg_start[:, None] + pos, 0)
    ids = entry_ids[where] if entry_ids.size else np.zeros_like(where)
    ids_l, val_l, len_l = ids.tolist(), val.tolist(), length.tolist()
    return [list(zip(i[:m], v[:m])) for i, v, m in zip(ids_l, val_l, len_l)]
