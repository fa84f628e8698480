"""Quick timing of the pairwise ALS kernels (Spark ALSModel.transform on a pair
frame / RegressionEvaluator) at the c2 shape (1M users x 100k items, density
0.5 %, rank 64; one device): the factors are hrec_als_init_factors', the
pairs the synthetic CSR's ratings, the labels its values. HIP events around
each call, the median of 5 after a warm-up call.
 (a) als_pair_metrics over the training pairs in CSR order (a user's row
     repeats across neighbouring pairs);
 (b) the same pairs in a random permutation;
 (c) als_predict_pairs writing the predictions (both orders).
Per line: ms, the algorithmic bytes (two factor rows + two int64 ids per pair,
+ the f64 label for the metrics, + the f32 output for the predictions) and
their rate as a fraction of the 6.29 TB/s measured HBM copy rate. Rows served
from the caches make a fraction above 1 possible.
 (d) the plain torch formulation (U[ur] * V[ir]).sum(1) over a slice that fits
     in memory (it writes and re-reads two gathered n x kp copies), and the
     kernel on the same slice: ns per pair of each.
Arguments: [n_users n_items density rank slice_pairs]."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src import synthetic  # noqa: E402
from src.als_engine import padded_k  # noqa: E402

a = sys.argv[1:]
n_users, n_items = (int(a[0]), int(a[1])) if len(a) > 1 else (1_000_000, 100_000)
density = float(a[2]) if len(a) > 2 else 0.005
k = int(a[3]) if len(a) > 3 else 64
n_slice = int(a[4]) if len(a) > 4 else 1 << 24
REPS, HBM = 5, 6.29e12
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


def line(name, ms, n, extra_bytes):
    nbytes = n * (2 * kp * 4 + 16 + extra_bytes)
    print(f"{name}: {ms:.2f} ms, {n} pairs, {nbytes / 1e9:.1f} GB algorithmic, {nbytes / ms / 1e9:.2f} TB/s = "
          f"{nbytes / (ms * 1e-3) / HBM:.2f} of the HBM copy rate, {ms * 1e6 / n:.3f} ns per pair")


csr = synthetic.generate(n_users, n_items, density, False)
n = csr.nnz
U = torch.zeros((n_users, kp), dtype=torch.float32, device=dev)
V = torch.zeros((n_items, kp), dtype=torch.float32, device=dev)
h.als_init_factors(synthetic.SEED_INIT, 0, n_users, k, kp, U)
h.als_init_factors(synthetic.SEED_INIT + 1, 0, n_items, k, kp, V)
ur = torch.repeat_interleave(torch.arange(n_users, device=dev), csr.indptr[1:] - csr.indptr[:-1])
ir = csr.indices.to(torch.int64)
y = csr.values.to(torch.float64)
print(f"{n_users} users x {n_items} items, rank {k} (kp {kp}), {n} pairs; U {U.numel() * 4 / 1e6:.0f} MB, "
      f"V {V.numel() * 4 / 1e6:.0f} MB")
out = torch.empty(n, dtype=torch.float32, device=dev)

sums = h.als_pair_metrics(U, V, ur, ir, k, y)
line("(a) als_pair_metrics, CSR order", timed(lambda: h.als_pair_metrics(U, V, ur, ir, k, y)), n, 8)
line("(c) als_predict_pairs, CSR order", timed(lambda: h.als_predict_pairs(U, V, ur, ir, k, out=out)), n, 4)
perm = torch.randperm(n, device=dev)
ur_p, ir_p, y_p = ur[perm], ir[perm], y[perm]
del perm
sums_p = h.als_pair_metrics(U, V, ur_p, ir_p, k, y_p)
line("(b) als_pair_metrics, random order", timed(lambda: h.als_pair_metrics(U, V, ur_p, ir_p, k, y_p)), n, 8)
line("(c) als_predict_pairs, random order", timed(lambda: h.als_predict_pairs(U, V, ur_p, ir_p, k, out=out)), n, 4)
s, sp = sums.tolist(), sums_p.tolist()
print(f"rmse over the training pairs {(s[4] / s[0]) ** 0.5:.6f} (CSR order), {(sp[4] / sp[0]) ** 0.5:.6f} (random "
      f"order); pairs kept {int(s[0])} / {int(sp[0])}, NaN {int(s[1])} / {int(sp[1])}")
del out, y_p

m = min(n_slice, n)
for name, su, si in (("CSR order", ur[:m].clone(), ir[:m].clone()), ("random order", ur_p[:m].clone(), ir_p[:m].clone())):
    o = torch.empty(m, dtype=torch.float32, device=dev)
    t_k = timed(lambda: h.als_predict_pairs(U, V, su, si, k, out=o))
    t_t = timed(lambda: (U[su] * V[si]).sum(1))
    close = torch.allclose(o, (U[su] * V[si]).sum(1), rtol=1e-4, atol=1e-6)
    print(f"(d) {m} pairs, {name}: als_predict_pairs {t_k * 1e6 / m:.3f} ns per pair, torch (U[ur] * V[ir]).sum(1) "
          f"{t_t * 1e6 / m:.3f} ns per pair, torch / kernel {t_t / t_k:.2f}, results close: {close}")
