"""Quick timing of the cosine neighbours (ranked_lists.similar ->
hrec_cosine_topk) at the shape of the README's c2-like rows: the top 10 for
all 100k items, ALS rank 64 (factors from hrec_als_init_factors) and two-tower
item vectors at d = 64 and d = 50 (build_model's weights), and the all-users
case on 65,536 users; one device. One run reports
 - end to end: similar() over every row in each arm (wall clock with a device
   sync, the median of REPS after a warm-up call), the batches the pruned arm
   flagged and the mean rows per query its filter kept;
 - hrec_cosine_topk alone on one batch of BATCH queries in each arm (HIP
   events, one warm-up, the median of 5), whether both arms return the same
   bits, and the torch formulation on the same batch in the same run:
   normalise in f64, mm, topk (and whether it finds the same columns);
 - both arms on one batch over the first n rows for a ladder of n: where auto
   (mode 0) should change arms.
The lines are printed and written to the file named by the first argument
(default profiles/similar_quick_c2.txt). Arguments: [out [n_users n_items]]."""
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch
from sklearn.preprocessing import MinMaxScaler

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src import ranked_lists  # noqa: E402
from src.two_tower_model import TwoTowerModel  # noqa: E402

a = sys.argv[1:]
out_path = a[0] if a else os.path.join(ROOT, "profiles", "similar_quick_c2.txt")
n_users, n_items = (int(a[1]), int(a[2])) if len(a) > 2 else (65_536, 100_000)
K, TOP, REPS, BATCH = 64, 10, 2, ranked_lists.SIMILAR_BATCH
LADDER = (1024, 2048, 3072, 4096, 6144, 8192, 16384, 32768, 65536)
dev = torch.device("cuda", torch.cuda.current_device())
lines = []


def say(*args):
    line = " ".join(str(x) for x in args)
    lines.append(line)
    print(line, flush=True)


def wall(fn, reps=REPS):
    """Median ms of `reps` calls (device synchronised), after one warm-up call."""
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


def torch_way(vec, d, q, top):
    """What a user would write: normalise in f64, mm, mask the diagonal, topk."""
    x = vec[:, :d].double()
    x = x / x.norm(dim=1, keepdim=True).clamp_min(1e-300)
    s = x[q] @ x.t()
    s[torch.arange(q.numel(), device=q.device), q] = float("-inf")
    return torch.topk(s, top, dim=1)


def kept_rows(vec, d, inv, items, q):
    """(mean, max) rows per query the pruned arm's matrix-core filter kept (hrec_cosine_topk_counts)."""
    n = int(vec.shape[0])
    ws = torch.empty(h.cosine_topk_workspace_bytes(q.numel(), n, TOP, d, 2), dtype=torch.uint8, device=vec.device)
    h.cosine_topk(vec, inv, q, TOP, mode=2, items=items, d=d, ws=ws, redo=False)
    cnt = h.cosine_topk_counts(ws, q.numel(), n, TOP, d)
    return float(cnt.double().mean().item()), int(cnt.max().item()), int((cnt > 4096).sum().item())


U = torch.zeros((n_users, K), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, K), dtype=torch.float32, device=dev)
h.als_init_factors(11, 0, n_users, K, K, U)
h.als_init_factors(12, 0, n_items, K, K, V)
rng = np.random.default_rng(9)
items_frame = pd.DataFrame({"itemId": np.arange(n_items), "manufacturer_id": rng.integers(0, 2651, n_items),
                            "category_id": rng.integers(0, 255, n_items), "price": rng.random(n_items) * 100,
                            "average_review_rating": rng.integers(0, 19, n_items).astype(np.float64)})
towers = {}
for d in (64, 50):
    tt = TwoTowerModel(1024, n_items, 2651, 255, embedding_size=d, seed=4)
    tt.build_model()
    tt.scaler = MinMaxScaler().fit(items_frame[["price", "average_review_rating"]])
    towers[d] = tt.candidates(items_frame).vectors

say(f"top {TOP} cosine neighbours; auto cut {h.COSINE_AUTO_CUT} rows; batches of {BATCH} queries")
for name, vec, d in (("ALS item factors, rank 64", V, K), ("two-tower item vectors, d 64", towers[64], 64),
                     ("two-tower item vectors, d 50 (200-byte rows)", towers[50], 50),
                     ("ALS user factors, rank 64", U, K)):
    n = int(vec.shape[0])
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    say(f"{name}: every one of {n} rows a query")
    res = {}
    for mode in ("auto", "pruned", "exhaustive"):
        stats = {}
        ms = wall(lambda: res.__setitem__(mode, ranked_lists.similar(vec, d, rows, TOP, mode=mode, stats=stats)))
        per = REPS + 1
        say(f"    similar(), mode {mode}, end to end: {ms:.1f} ms = {ms / n * 1e3:.2f} us per query; "
            f"{stats['batches'] // per} batches, {stats['flagged'] // per} flagged and redone exhaustively")
    same = all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x,
                           y.view(torch.int64) if y.dtype == torch.float64 else y)
               for other in ("auto", "pruned") for x, y in zip(res[other], res["exhaustive"]))
    say(f"    auto and both arms return the same bits: {same}")
    del res
    inv = h.row_inv_norms(vec, d)
    op = h.cosine_items(vec, inv, d)
    q = rows[:BATCH].contiguous()
    ms_p = events(lambda: h.cosine_topk(vec, inv, q, TOP, mode=2, items=op, d=d))
    ms_e = events(lambda: h.cosine_topk(vec, inv, q, TOP, mode=1, d=d))
    ms_t = events(lambda: torch_way(vec, d, q, TOP), reps=3)
    idx = h.cosine_topk(vec, inv, q, TOP, mode=2, items=op, d=d)[0]
    same_cols = int((idx == torch_way(vec, d, q, TOP).indices).all(1).sum().item())
    say(f"    hrec_cosine_topk alone, the first {q.numel()} queries: pruned {ms_p:.3f} ms, exhaustive {ms_e:.3f} ms "
        f"({ms_e / ms_p:.2f} x the pruned arm); torch normalise (f64) + mm + topk {ms_t:.3f} ms = "
        f"{ms_t / ms_p:.2f} x pruned, {ms_t / ms_e:.2f} x exhaustive; identical columns: {same_cols} of {q.numel()}")
    mean_kept, max_kept, over = kept_rows(vec, d, inv, op, q)
    say(f"    rows per query the matrix-core filter kept for the exact chain: mean {mean_kept:.1f}, max {max_kept}; "
        f"{over} of {q.numel()} lists past the capacity of 4096 (an overflowed list counts at least 4097)")
    del inv, op

say(f"one batch of {BATCH} queries over the first n ALS item rows (rank 64), top {TOP}: where auto changes arms")
for n in LADDER + (n_items,):
    if n > n_items:
        continue
    vec = V[:n]
    inv = h.row_inv_norms(vec, K)
    op = h.cosine_items(vec, inv, K)
    q = torch.arange(min(BATCH, n), dtype=torch.int64, device=dev)
    ms_p = events(lambda: h.cosine_topk(vec, inv, q, TOP, mode=2, items=op, d=K))
    ms_e = events(lambda: h.cosine_topk(vec, inv, q, TOP, mode=1, d=K))
    say(f"    n {n}: pruned {ms_p:.3f} ms, exhaustive {ms_e:.3f} ms -> {'pruned' if ms_p < ms_e else 'exhaustive'}"
        f" (auto takes {'pruned' if n >= h.COSINE_AUTO_CUT else 'exhaustive'})")

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
