"""Quick timing of the hybrid top-n lists (HybridRecommendationSystem.
recommend_for_users -> hrec_hybrid_lists) at the c2 shape: 65,536 users x
100k candidates, ALS rank 64 (factors from hrec_als_init_factors), two-tower
d = 64 (build_model's weights), top 10, one device. Two runs: nothing
excluded, and each user's own unfiltered top 500 excluded (what a fitted
model's training frame looks like). Each reports
 - the end-to-end time of _recommend_device over every user (scores of both
   models per sub-batch, hrec_hybrid_lists, the overflow route, list
   finishing; with an exclusion also the CSR of its pairs), wall clock with a
   device sync, the median of REPS after a warm-up call;
 - the bare hrec_hybrid_lists time for one sub-batch (HIP events, the median
   of 5) and the fraction of the 6.29 TB/s HBM copy rate that is, against the
   bytes the entry must read (both matrices, twice: extremes, then the pass);
 - the sub-batches whose overflow flag was set (redone in mode 1);
 - get_hybrid_recommendations looped over 256 of the same users in the same
   run, per user, and the ratio per user to the batched lists.
Arguments: [n_users n_items]."""
import contextlib
import io
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
K, D, TOP, SEEN, REPS, LOOP = 64, 64, 10, 500, 2, 256
HBM_COPY = 6.29e12
dev = torch.device("cuda", torch.cuda.current_device())

U = torch.zeros((n_users, K), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, K), dtype=torch.float32, device=dev)
h.als_init_factors(11, 0, n_users, K, K, U)
h.als_init_factors(12, 0, n_items, K, K, V)
als = ALSModel(rank=K)
als.spark = DeviceSession()
als.model = DeviceALSFactors(np.arange(n_users), np.arange(n_items), U, V, K)
tt = TwoTowerModel(n_users, n_items, 2651, 255, embedding_size=D, seed=4)
tt.build_model()
rng = np.random.default_rng(9)
items = pd.DataFrame({"itemId": np.arange(n_items), "manufacturer_id": rng.integers(0, 2651, n_items),
                      "category_id": rng.integers(0, 255, n_items), "price": rng.random(n_items) * 100,
                      "average_review_rating": rng.integers(0, 19, n_items).astype(np.float64)})
tt.scaler = MinMaxScaler().fit(items[["price", "average_review_rating"]])
hyb = HybridRecommendationSystem()
hyb.als_model, hyb.twotower_model, hyb.models_loaded = als, tt, True
hyb.als_f1_score, hyb.twotower_f1_score = 0.5, 0.1
cand = tt.candidates(items)
users = np.arange(n_users, dtype=np.int64)
sub = max(1, min(hyb.RECOMMEND_ROWS, hyb.RECOMMEND_SCORE_BYTES // (8 * n_items)))
print(f"{n_users} users x {n_items} candidates, ALS rank {K}, two-tower d {D}, top {TOP}; sub-batches of {sub} users "
      f"({-(-n_users // sub)} of them)")

flags = []
real = h.hybrid_lists


def counting(*args, **kw):
    res = real(*args, **kw)
    if kw.get("mode", 0) == 0:
        flags.append(res[3])
    return res


h.hybrid_lists = counting


def wall(fn, reps=REPS):
    """Median ms of `reps` calls (device synchronised), one warm-up call first."""
    ms = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep:
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


# the per-user loop, over candidates both models can score (bench.py's id array)
class IdArray(np.ndarray):
    def __getitem__(self, key):
        if isinstance(key, (str, list)):
            return items[key]
        return super().__getitem__(key)


arr = items["itemId"].to_numpy().view(IdArray)
loop_users = [int(u) for u in np.linspace(0, n_users - 1, LOOP).astype(np.int64)]
with contextlib.redirect_stdout(io.StringIO()):
    hyb.get_hybrid_recommendations(loop_users[0], arr, top_k=TOP)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for u in loop_users:
        hyb.get_hybrid_recommendations(u, arr, top_k=TOP)
    torch.cuda.synchronize()
loop_ms = (time.perf_counter() - t0) * 1e3 / LOOP
print(f"get_hybrid_recommendations looped over {LOOP} users: {loop_ms:.3f} ms per user")

# each user's own unfiltered top SEEN, as an exclude frame
ids, _, _ = hyb._recommend_device(users, cand, min(SEEN, n_items))
own = pd.DataFrame({"userId": np.repeat(users, ids.shape[1]), "itemId": ids.cpu().numpy().reshape(-1)})
del ids

for tag, exclude in (("nothing excluded", None), (f"own top {SEEN} excluded", own)):
    flags.clear()
    ms = wall(lambda: hyb._recommend_device(users, cand, TOP, exclude))
    n_calls = len(flags) // (REPS + 1)
    n_flag = int(torch.cat(flags[-n_calls:]).sum().item())
    # one sub-batch, the entry alone
    s_users = users[:sub]
    A = als.model.score(s_users, cand.item_ids)
    T = h.tt_score(tt.model.user_vectors(torch.as_tensor(s_users.astype(np.int32), device=dev)), cand.vectors)
    excl = None
    if exclude is not None:
        rows = torch.arange(len(s_users), dtype=torch.int64, device=dev)
        excl = (rows, *tt._exclusion(s_users, cand, exclude[exclude["userId"] < len(s_users)]))
    bare = events(lambda: real(A, T, TOP, True, excl=excl))
    over = int(real(A, T, TOP, True, excl=excl)[3].item())
    must = 2 * 2 * A.numel() * 4
    print(f"({tag}) end to end {ms:.1f} ms ({n_users / ms * 1e3:.0f} users/s, {ms / n_users:.4f} ms per user; the "
          f"per-user loop / this = {loop_ms / (ms / n_users):.0f}); {n_flag} of {n_calls} sub-batches flagged")
    print(f"    hrec_hybrid_lists alone, one sub-batch of {len(s_users)} users: {bare:.3f} ms, {must / 1e9:.3f} GB "
          f"to read -> {must / (bare / 1e3) / 1e12:.2f} TB/s = {must / (bare / 1e3) / HBM_COPY:.2f} of the "
          f"{HBM_COPY / 1e12:.2f} TB/s copy rate (overflow flag {over})")
    del A, T
