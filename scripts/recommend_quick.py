"""Quick timing of the recommendation driver and the ranking-metrics kernel at
the c2 shape (1M users x 100k items, density 0.5 %, rank 64; one device): the
factors are hrec_als_init_factors', the raw ids the row numbers, the ground
truth the synthetic CSR's rows. HIP events around each call, the median of 5
after a warm-up call.
 (a) DeviceALSFactors.recommend("user", every row, 10) end to end (batches of
     RECOMMEND_BATCH rows, the id gather included), and beside it the bare
     als_score_topk_pruned call for one batch of 4096 rows, top 10: the ratio
     of (a) to the bare call times the number of batches is the driver's
     overhead;
 (b) the same for side="item": the top 10 users of every item;
 (c) hrec_ranking_metrics over (a)'s lists, k = 10, labels = the CSR's rows:
     ms, the algorithmic bytes (labels, lists, row pointer) and their rate as
     a fraction of the 6.29 TB/s measured HBM copy rate.
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
REPS, HBM, TOP, BARE = 5, 6.29e12, 10, 4096
kp = padded_k(k)
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fn):
    """Median ms of REPS event-timed calls, one warm-up call first."""
    ms = []
    for rep in range(REPS + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


U = torch.zeros((n_users, kp), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, kp), dtype=torch.float32, device=dev)
h.als_init_factors(synthetic.SEED_INIT, 0, n_users, k, kp, U)
h.als_init_factors(synthetic.SEED_INIT + 1, 0, n_items, k, kp, V)
model = DeviceALSFactors(np.arange(n_users), np.arange(n_items), U, V, k)
print(f"{n_users} users x {n_items} items, rank {k} (kp {kp}); top {TOP}, batches of {model.RECOMMEND_BATCH} rows")

lists = None
for tag, side, n_own, n_other in (("(a)", "user", n_users, n_items), ("(b)", "item", n_items, n_users)):
    rows = torch.arange(n_own, device=dev)
    Q, F, Ft, bf, _ = model._recommend_operands(side)  # built once per side, outside the timing
    torch.cuda.synchronize()
    ms = timed(lambda: model.recommend(side, rows, TOP))
    pairs = n_own * n_other
    print(f"{tag} recommend('{side}', {n_own} rows, {TOP}): {ms:.1f} ms end to end, {pairs / ms / 1e9:.3f}e12 pairs/s")
    b = min(BARE, n_own)
    need = int(h.lib().hrec_als_score_topk_pruned_workspace_bytes(b, n_other, TOP, k))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    bare = timed(lambda: h.als_score_topk_pruned(Q, rows[:b], Ft, F, bf, n_other, k, TOP, check_overflow=False,
                                                 overflow_out=flag, workspace=ws))
    n_batches = -(-n_own // model.RECOMMEND_BATCH)
    print(f"{tag} bare als_score_topk_pruned, B = {b}: {bare:.3f} ms, {b * n_other / bare / 1e9:.3f}e12 pairs/s; "
          f"x {n_own / b:.1f} batches = {bare * n_own / b:.1f} ms; end to end / that = {ms / (bare * n_own / b):.3f} "
          f"({n_batches} driver batches)")
    if side == "user":
        lists = model.recommend(side, rows, TOP)[0]
    del ws, rows

csr = synthetic.generate(n_users, n_items, density, False)
labels = csr.indices.to(torch.int64)
indptr = csr.indptr
nnz = labels.numel()
sums, unsorted, _ = h.ranking_metrics(lists, indptr, labels, TOP)
ms = timed(lambda: h.ranking_metrics(lists, indptr, labels, TOP))
nbytes = 8 * nnz + 8 * TOP * n_users + 8 * (n_users + 1)
s = dict(zip(h.RANK_SUMS, sums.tolist()))
print(f"(c) ranking_metrics, {n_users} rows, k = {TOP}, {nnz} labels ({nnz / n_users:.0f} per row): {ms:.3f} ms, "
      f"{nbytes / 1e9:.2f} GB algorithmic, {nbytes / ms / 1e9:.2f} TB/s = {nbytes / (ms * 1e-3) / HBM:.2f} of the "
      f"HBM copy rate")
print(f"    unsorted flag {int(unsorted.item())}, rows {int(s['n_rows'])}, empty {int(s['n_empty'])}, hits "
      f"{int(s['hits'])}, precision@{TOP} {s['sum_precision'] / n_users:.6f}, ndcg@{TOP} "
      f"{s['sum_ndcg'] / n_users:.6f}")
