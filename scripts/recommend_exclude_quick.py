"""Quick timing of the recommendation driver under a seen-item exclusion at the
c2 shape (1M users x 100k items, density 0.5 %, rank 64; one device): the
factors are hrec_als_init_factors', the raw ids the row numbers. HIP events
around each call, the median of 5 after a warm-up call. One run measures
 (0) DeviceALSFactors.exclusion("user", ...) from the synthetic CSR's pairs
     (device id tensors): the time to build the exclusion CSR;
 (a) recommend("user", every row, 10, exclude=that CSR): about 500 excluded
     items per user, unrelated to the scores;
 (b) the same for the first 65,536 users with each user's own unfiltered top
     500 (from recommend(..., 500)) as its exclusion: what a fitted model
     looks like, the excluded items are the best-scored ones;
 (c) the unfiltered recommend("user", every row, 10) in the same run (the
     bf16-pruned path);
 (d) one batch of RECOMMEND_BATCH rows through the fallback sequence alone:
     als_score, mask_rows (NaN), topk; beside it one batch through
     als_score_topk_excluding alone.
It prints the four times, (a) / (c), the per-batch ratio of (a) to (d), and
the share of batches whose overflow flag was set in (a) and in (b).
Arguments: [n_users n_items density rank]."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src import synthetic  # noqa: E402
from src.als_engine import padded_k  # noqa: E402
from src.als_model import DeviceALSFactors  # noqa: E402

a = sys.argv[1:]
n_users, n_items = (int(a[0]), int(a[1])) if len(a) > 1 else (1_000_000, 100_000)
density = float(a[2]) if len(a) > 2 else 0.005
k = int(a[3]) if len(a) > 3 else 64
REPS, TOP, SEEN, N_B = 5, 10, 500, 65_536
kp = padded_k(k)
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fn, reps=REPS):
    """Median ms of `reps` event-timed calls, one warm-up call first."""
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


def flagged(model, rows, excl):
    """Share of recommend's batches whose overflow flag the library set."""
    Q, F, Ft, _, _ = model._recommend_operands("user")
    B = model.RECOMMEND_BATCH
    starts = range(0, rows.numel(), B)
    flags = torch.zeros(len(starts), dtype=torch.int32, device=dev)
    need = int(h.lib().hrec_als_score_topk_excluding_workspace_bytes(min(B, rows.numel()), n_items, TOP))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for b, s in enumerate(starts):
        h.als_score_topk_excluding(Q, rows[s: s + B], Ft, n_items, k, TOP, *excl, overflow_out=flags[b: b + 1],
                                   workspace=ws)
    return int(flags.sum().item()), len(starts)


U = torch.zeros((n_users, kp), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, kp), dtype=torch.float32, device=dev)
h.als_init_factors(synthetic.SEED_INIT, 0, n_users, k, kp, U)
h.als_init_factors(synthetic.SEED_INIT + 1, 0, n_items, k, kp, V)
model = DeviceALSFactors(np.arange(n_users), np.arange(n_items), U, V, k)
B = model.RECOMMEND_BATCH
print(f"{n_users} users x {n_items} items, rank {k} (kp {kp}); top {TOP}, batches of {B} rows")
rows = torch.arange(n_users, device=dev)
Q, F, Ft, _, _ = model._recommend_operands("user")  # built once, outside the timing

# (0) the exclusion CSR from the synthetic frame's pairs
csr = synthetic.generate(n_users, n_items, density, False)
counts = csr.indptr[1:] - csr.indptr[:-1]
pair_users = torch.repeat_interleave(rows, counts)
pair_items = csr.indices.to(torch.int64)
nnz = pair_items.numel()
torch.cuda.synchronize()
ms0 = timed(lambda: model.exclusion("user", pair_users, pair_items), reps=3)
excl_a = model.exclusion("user", pair_users, pair_items)
assert torch.equal(excl_a[0], csr.indptr) and torch.equal(excl_a[1], csr.indices.to(torch.int32))
del pair_users, pair_items, csr
print(f"(0) exclusion('user') from {nnz} pairs ({nnz / n_users:.0f} per user), device ids: {ms0:.1f} ms")

# (a) every user, the synthetic rows excluded
ms_a = timed(lambda: model.recommend("user", rows, TOP, exclude=excl_a))
fl_a, nb_a = flagged(model, rows, excl_a)
pairs = n_users * n_items
print(f"(a) recommend('user', {n_users} rows, {TOP}, exclude = {nnz / n_users:.0f} per user): {ms_a:.1f} ms end to "
      f"end, {pairs / ms_a / 1e9:.3f}e12 pairs/s; {fl_a} of {nb_a} batches flagged ({fl_a / nb_a:.3f})")

# (b) the first N_B users, each user's own top SEEN excluded
nb_users = min(N_B, n_users)
rows_b = rows[:nb_users]
seen = min(SEEN, n_items)
top_ids, _ = model.recommend("user", rows_b, seen)
excl_b = model.exclusion("user", torch.repeat_interleave(rows_b, seen), top_ids.reshape(-1))
del top_ids
assert int(excl_b[0][nb_users].item()) == nb_users * seen == excl_b[1].numel()
ms_b = timed(lambda: model.recommend("user", rows_b, TOP, exclude=excl_b))
fl_b, nb_b = flagged(model, rows_b, excl_b)
print(f"(b) recommend('user', {nb_users} rows, {TOP}, exclude = own top {seen}): {ms_b:.1f} ms end to end, "
      f"{nb_users * n_items / ms_b / 1e9:.3f}e12 pairs/s, x {n_users / nb_users:.2f} = {ms_b * n_users / nb_users:.1f} "
      f"ms per {n_users} users; {fl_b} of {nb_b} batches flagged ({fl_b / nb_b:.3f})")

# (c) the unfiltered path in the same run
ms_c = timed(lambda: model.recommend("user", rows, TOP))
print(f"(c) recommend('user', {n_users} rows, {TOP}), no exclusion (the pruned path): {ms_c:.1f} ms end to end, "
      f"{pairs / ms_c / 1e9:.3f}e12 pairs/s; (a) / (c) = {ms_a / ms_c:.2f}")

# (d) one batch: the fallback sequence, and the excluding call
b = min(B, n_users)
rows_d = rows[:b]
scores = torch.empty((b, n_items), dtype=torch.float32, device=dev)


def fallback():
    h.als_score(Q, rows_d, Ft, None, n_items, k, out=scores)
    h.mask_rows(scores, rows_d, *excl_a)
    h.topk(scores, TOP)


ms_d = timed(fallback)
need = int(h.lib().hrec_als_score_topk_excluding_workspace_bytes(b, n_items, TOP))
ws = torch.empty(need, dtype=torch.uint8, device=dev)
flag = torch.zeros(1, dtype=torch.int32, device=dev)
ms_e = timed(lambda: h.als_score_topk_excluding(Q, rows_d, Ft, n_items, k, TOP, *excl_a, overflow_out=flag,
                                                workspace=ws))
per_batch_a = ms_a * b / n_users
print(f"(d) one batch of {b} rows, als_score + mask_rows + topk: {ms_d:.3f} ms ({b * n_items / ms_d / 1e9:.3f}e12 "
      f"pairs/s); bare als_score_topk_excluding: {ms_e:.3f} ms ({b * n_items / ms_e / 1e9:.3f}e12 pairs/s)")
print(f"    (a) per batch = {per_batch_a:.3f} ms; (a) / (d) per batch = {per_batch_a / ms_d:.3f}; "
      f"bare excluding / (d) = {ms_e / ms_d:.3f}")
