"""Quick timing of the list-quality pass (list_quality_metrics ->
hrec_row_inv_norms + hrec_list_quality) at the shape of the README's c2-like
rows: 65,536 users x 100k candidates, top 10, ALS rank 64 (factors from
hrec_als_init_factors), two-tower d = 64 and d = 50 (build_model's weights);
the history of a user is its own unfiltered ALS top 500; one device. One run
reports
 - hrec_list_quality alone on one sub-batch (HIP events, the median of 5),
   per vector width, with and without the histories, against the bytes it
   must read (the lists, the histories, ld * 4 bytes and one inverse norm per
   gathered row, two table values per list entry) and the 6.29 TB/s HBM copy
   rate. The item table (n * ld * 4 bytes) is read many times over: the
   script prints its size against the 4 MiB L2 of an XCD and the 256 MiB
   Infinity Cache;
 - the same call when every user is given the same list: the worst case of
   the exposure atomics (ten counters take every increment);
 - the torch formulation on the same sub-batch in the same run, in f32:
   vectors[cols], normalise, bmm, bincount (and vectors[history] and a second
   bmm with the histories);
 - end to end list_quality_metrics against recommend_for_users /
   recommend_for_user_subset alone for the same users, for the three models
   (wall clock with a device sync, the median of REPS after a warm-up call),
   without a history frame, and once with the 500-per-user history frame for
   the ALS model (its CSR and tables are built on the device).
Arguments: [n_users n_items]."""
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch
from sklearn.preprocessing import MinMaxScaler

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src.als_model import ALSModel, DeviceALSFactors, DeviceSession  # noqa: E402
from src.hybrid_system import HybridRecommendationSystem  # noqa: E402
from src.two_tower_model import TwoTowerModel  # noqa: E402

a = sys.argv[1:]
n_users, n_items = (int(a[0]), int(a[1])) if len(a) > 1 else (65_536, 100_000)
K, TOP, HIST, REPS = 64, 10, min(500, n_items), 2
HBM_COPY = 6.29e12
dev = torch.device("cuda", torch.cuda.current_device())


def say(*args):
    print(*args, flush=True)


U = torch.zeros((n_users, K), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, K), dtype=torch.float32, device=dev)
h.als_init_factors(11, 0, n_users, K, K, U)
h.als_init_factors(12, 0, n_items, K, K, V)
als = ALSModel(rank=K)
als.spark = DeviceSession()
als.model = DeviceALSFactors(np.arange(n_users), np.arange(n_items), U, V, K)
rng = np.random.default_rng(9)
items = pd.DataFrame({"itemId": np.arange(n_items), "manufacturer_id": rng.integers(0, 2651, n_items),
                      "category_id": rng.integers(0, 255, n_items), "price": rng.random(n_items) * 100,
                      "average_review_rating": rng.integers(0, 19, n_items).astype(np.float64)})
towers = {}
for d in (64, 50):
    tt = TwoTowerModel(n_users, n_items, 2651, 255, embedding_size=d, seed=4)
    tt.build_model()
    tt.scaler = MinMaxScaler().fit(items[["price", "average_review_rating"]])
    towers[d] = (tt, tt.candidates(items))
hyb = HybridRecommendationSystem()
hyb.als_model, hyb.twotower_model, hyb.models_loaded = als, towers[64][0], True
hyb.als_f1_score, hyb.twotower_f1_score = 0.5, 0.1
users = np.arange(n_users, dtype=np.int64)


def wall(fn, reps=REPS, warm=True):
    """Median ms of `reps` calls (device synchronised), after one warm-up call."""
    ms = []
    for rep in range(reps + (1 if warm else 0)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep or not warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def events(fn, reps=5):
    ms = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def rate(ms, nbytes):
    return (f"{ms:.3f} ms, {nbytes / 1e6:.1f} MB to read -> {nbytes / (ms / 1e3) / 1e12:.3f} TB/s = "
            f"{nbytes / (ms / 1e3) / HBM_COPY:.3f} of the {HBM_COPY / 1e12:.2f} TB/s copy rate")


m = min(als.LIST_QUALITY_ROWS, n_users)
rows = torch.arange(m, dtype=torch.int64, device=dev)
say(f"{n_users} users x {n_items} candidates, top {TOP}, history {HIST} per user; one sub-batch = {m} users")
# the lists and the histories: the ALS model's own top 10 and top 500 (unfiltered), as columns
lists = als.model.recommend("user", rows, TOP, _columns=True)[0]
hist_cols = torch.sort(als.model.recommend("user", rows, HIST, _columns=True)[0], dim=1).values
hist = (rows, torch.arange(0, (m + 1) * HIST, HIST, dtype=torch.int64, device=dev),
        hist_cols.to(torch.int32).reshape(-1).contiguous())
tables = torch.rand((2, n_items), dtype=torch.float64, device=dev)
same_lists = lists[:1].expand(m, TOP).contiguous()


def need(ld, with_hist):
    """The bytes one call must read: lists, histories (and their segment bounds), one vector row and one inverse
    norm per gathered entry, two table values and one exposure counter per list entry."""
    per_list = TOP * (8 + ld * 4 + 8 + 2 * 8 + 8)
    per_hist = (HIST * (4 + ld * 4 + 8) + 2 * 8) if with_hist else 0
    return m * (per_list + per_hist)


def torch_way(vec, cols, hcols):
    """What a user would write: gather, normalise, bmm, bincount (f32)."""
    x = torch.nn.functional.normalize(vec[cols], dim=2)
    g = torch.bmm(x, x.transpose(1, 2))
    k = cols.shape[1]
    ild = 1 - (g.sum((1, 2)) - g.diagonal(dim1=1, dim2=2).sum(1)) / (k * (k - 1))
    exposure = torch.bincount(cols.reshape(-1), minlength=vec.shape[0])
    unx = None
    if hcols is not None:
        xh = torch.nn.functional.normalize(vec[hcols], dim=2)
        unx = 1 - torch.bmm(x, xh.transpose(1, 2)).mean((1, 2))
    return ild, unx, exposure


for name, vec, d in (("ALS item factors, d 64 (ld 64)", V, K),
                     ("two-tower vectors, d 64", towers[64][1].vectors, 64),
                     ("two-tower vectors, d 50 (200-byte rows)", towers[50][1].vectors, 50)):
    ld = int(vec.stride(0))
    table_mb = n_items * ld * 4 / 2 ** 20
    say(f"{name}: item table {table_mb:.1f} MiB ({'above' if table_mb > 4 else 'inside'} one XCD's 4 MiB L2, "
        f"{'inside' if table_mb < 256 else 'above'} the 256 MiB Infinity Cache)")
    inv = h.row_inv_norms(vec, d)
    ms_inv = events(lambda: h.row_inv_norms(vec, d))
    say(f"    hrec_row_inv_norms, {n_items} rows: {ms_inv:.3f} ms")
    for with_hist in (False, True):
        hs = hist if with_hist else None
        ms = events(lambda: h.list_quality(lists, vec, inv, history=hs, tables=tables, d=d))
        say(f"    hrec_list_quality alone, {'with' if with_hist else 'no'} histories: {rate(ms, need(ld, with_hist))}")
        ms_same = events(lambda: h.list_quality(same_lists, vec, inv, history=hs, tables=tables, d=d))
        say(f"        every user the same list (contended exposure):  {ms_same:.3f} ms = {ms_same / ms:.2f} x")
        hc = hist_cols if with_hist else None
        ms_t = events(lambda: torch_way(vec, lists, hc), reps=3)
        say(f"        torch gather + normalise + bmm + bincount (f32): {ms_t:.3f} ms = {ms_t / ms:.1f} x")
    per_row, _, expo, _ = h.list_quality(lists, vec, inv, history=hist, tables=tables, d=d)
    ild, unx, expo_t = torch_way(vec, lists, hist_cols)
    say(f"    against the f32 torch values: diversity max |diff| {float((per_row[:, 0] - ild).abs().max()):.2e}, "
        f"unexpectedness {float((per_row[:, 1] - unx).abs().max()):.2e}, exposure equal: "
        f"{bool((expo == expo_t).all().item())}")
    del inv, per_row, ild, unx
del hist_cols, hist, same_lists, tables

tt64, cand64 = towers[64]
tt50, cand50 = towers[50]
for name, rec, met in (
        ("ALSModel", lambda: als.model.recommend("user", torch.as_tensor(users, device=dev), TOP),
         lambda: als.list_quality_metrics(TOP)),
        ("TwoTowerModel d 64", lambda: tt64._recommend_device(users, cand64, TOP),
         lambda: tt64.list_quality_metrics(cand64, TOP)),
        ("TwoTowerModel d 50", lambda: tt50._recommend_device(users, cand50, TOP),
         lambda: tt50.list_quality_metrics(cand50, TOP)),
        ("HybridRecommendationSystem d 64", lambda: hyb._recommend_device(users, cand64, TOP),
         lambda: hyb.list_quality_metrics(cand64, TOP))):
    ms_rec, ms_met = wall(rec), wall(met)
    res = met()
    shown = ("catalogCoverage", "distributionalCoverage", "gini", "personalization", "intraListDiversity")
    say(f"{name}: the device lists alone {ms_rec:.1f} ms, list_quality_metrics {ms_met:.1f} ms: "
        f"+{ms_met - ms_rec:.1f} ms ({(ms_met - ms_rec) / n_users * 1e3:.3f} us per user); "
        + ", ".join(f"{k} {res[k]:.5f}" for k in shown))

top = als.model.recommend("user", torch.as_tensor(users, device=dev), HIST, _columns=True)[0]
frame = pd.DataFrame({"userId": np.repeat(users, HIST), "itemId": top.cpu().numpy().reshape(-1)})
del top
ms = wall(lambda: als.list_quality_metrics(TOP, history=frame), reps=1, warm=False)
res = als.list_quality_metrics(TOP, history=frame)
say(f"ALSModel.list_quality_metrics with a history frame of {len(frame)} rows (one call; CSR and tables built on the "
    f"device): {ms:.1f} ms; "
    + ", ".join(f"{k} {res[k]:.5f}" for k in ("unexpectedness", "novelty", "averagePopularity")))
