"""Quick timing of the fold-in calls at the shape of the README's c2-like
rows: 65,536 new users x 20 ratings each against 100k items; one device. One
run reports
 - ALSModel.fold_in_users at rank 64 and rank 10, on a model that already
   holds 1M users (factors from hrec_als_init_factors): end to end (wall clock
   with a device sync, the median of REPS after a warm-up call; the frame is
   built outside the clock, the model is reset to the 1M users before every
   call) and the bare hrec_als_half_sweep launch on the same CSR (HIP events);
 - hrec_tt_fold_in_users at d = 64 and d = 50, 100 steps: all 65,536 users in
   one launch (HIP events), against the bytes a step reads from the caches and
   its multiply-adds; and on a sub-batch of 8,192 users against the
   formulation available before, a torch implementation on the device of the
   same recurrence over padded histories (gather of the history's item vectors
   once, then per step the LayerNorm, two bmm and the Adam update as
   elementwise ops), with the largest difference between the two results;
 - for scale only, the same 65,536 users through DeviceTwoTower.train_step (c2
   tables, d = 64, batch 256): train_step cannot freeze the other variables
   and every step sweeps all four tables, so this is a DIFFERENT computation;
   100 passes over the 1,310,720 ratings in batches of 256 are 512,000 steps,
   projected from the measured step.
Arguments: [n_new n_items ratings_per_user]."""
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src.als_model import ALSModel, DeviceALSFactors, DeviceSession  # noqa: E402
from src.als_engine import padded_k  # noqa: E402
from src.tt_engine import AdamConfig, DeviceTwoTower  # noqa: E402

a = sys.argv[1:]
n_new, n_items, per_user = (int(a[0]), int(a[1]), int(a[2])) if len(a) > 2 else (65_536, 100_000, 20)
N_OLD, STEPS, LR, SUB, REPS = 1_000_000, 100, 1e-2, 8192, 3
dev = torch.device("cuda", torch.cuda.current_device())


def say(*args):
    print(*args, flush=True)


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


rng = np.random.default_rng(3)
nnz = n_new * per_user
item_of = rng.integers(0, n_items, nnz).astype(np.int64)
rating_of = (rng.integers(2, 11, nnz) / 2).astype(np.float32)
data = pd.DataFrame({"userId": np.repeat(np.arange(N_OLD, N_OLD + n_new, dtype=np.int64), per_user),
                     "itemId": item_of, "average_review_rating": rating_of.astype(np.float64)})
indptr = torch.arange(0, nnz + 1, per_user, dtype=torch.int64, device=dev)
say(f"{n_new} new users x {per_user} ratings = {nnz} ratings against {n_items} items")

# ------------------------------------------------------------------- ALS
for k in (64, 10):
    kp = padded_k(k)
    U = torch.zeros((N_OLD, kp), dtype=torch.float32, device=dev)
    V = torch.zeros((n_items, kp), dtype=torch.float32, device=dev)
    h.als_init_factors(11, 0, N_OLD, k, kp, U)
    h.als_init_factors(12, 0, n_items, k, kp, V)
    als = ALSModel(rank=k, reg_param=0.1)
    als.spark = DeviceSession()
    base = DeviceALSFactors(np.arange(N_OLD), np.arange(n_items), U, V, k)

    def fold():
        als.model = base
        return als.fold_in_users(data)

    ms_e2e = wall(fold)
    res = fold()
    assert res["users_added"] == n_new and res["ratings_used"] == nnz and len(als.model.user_ids) == N_OLD + n_new
    ix = torch.as_tensor(item_of.astype(np.int32), device=dev)
    vals = torch.as_tensor(rating_of, device=dev)
    dst = torch.zeros((n_new, kp), dtype=torch.float32, device=dev)
    ms_sweep = events(lambda: h.als_half_sweep(indptr, ix, vals, V, k, 0.1, dst))
    say(f"ALS rank {k}: fold_in_users end to end {ms_e2e:.1f} ms ({ms_e2e / n_new * 1e3:.2f} us per user; the model "
        f"holds {N_OLD} users before, {N_OLD + n_new} after); the bare hrec_als_half_sweep launch on the same CSR "
        f"{ms_sweep:.3f} ms = {ms_sweep / ms_e2e:.3f} of it")
    del als, base, U, V, dst

# ------------------------------------------------------------- two-tower
def torch_way(emb, gamma, beta, vec, rows, ratings, lr, b1, omb1, b2, omb2, eps):
    """The recurrence in torch ops, f32, histories padded to one length (mask: the usable entries)."""
    mask = ((rows >= 0) & (rows < vec.shape[0])).float()
    n = mask.sum(1, keepdim=True)
    vr = vec[rows.clamp(0, vec.shape[0] - 1)] * mask.unsqueeze(2)  # [n, h, d], gathered once
    e = emb.clone()
    m, v = torch.zeros_like(e), torch.zeros_like(e)
    for t in range(lr.numel()):
        xc = e - e.mean(1, keepdim=True)
        rstd = torch.rsqrt((xc * xc).mean(1, keepdim=True) + 1e-3)
        xh = xc * rstd
        u = xh * gamma + beta
        err = (torch.bmm(vr, u.unsqueeze(2)).squeeze(2) - ratings) * mask
        du = (2.0 / n) * torch.bmm(err.unsqueeze(1), vr).squeeze(1)
        dxh = du * gamma
        g = rstd * (dxh - dxh.mean(1, keepdim=True) - xh * (dxh * xh).mean(1, keepdim=True))
        m = m * b1 + g * omb1
        v = v * b2 + (g * g) * omb2
        e = e - (lr[t] * m) / (v.sqrt() + eps)
    return e


opt = AdamConfig(LR)
c0 = opt.coefficients(0)
adam = (float(opt.b1), float(c0["omb1"]), float(opt.b2), float(c0["omb2"]), float(opt.eps))
lr = torch.as_tensor(np.array([opt.coefficients(t)["sparse_lr"] for t in range(STEPS)], np.float32), device=dev)
rows = torch.as_tensor(item_of, device=dev)
ratings = torch.as_tensor(rating_of, device=dev)
for d in (64, 50):
    g = torch.Generator(device=dev).manual_seed(d)
    emb0 = torch.empty((n_new, d), dtype=torch.float32, device=dev).uniform_(-0.05, 0.05, generator=g)
    vec = torch.randn((n_items, d), dtype=torch.float32, device=dev, generator=g)
    gamma = 1.0 + 0.1 * torch.randn(d, dtype=torch.float32, device=dev, generator=g)
    beta = 0.1 * torch.randn(d, dtype=torch.float32, device=dev, generator=g)

    def kernel(n):
        emb = emb0[:n].clone()
        loss = h.tt_fold_in_users(emb, gamma, beta, vec, indptr[: n + 1], rows, ratings, lr, *adam)
        return emb, loss

    ms_all = events(lambda: kernel(n_new))
    fma = 2.0 * n_new * per_user * d * (STEPS + 1) + 0.0  # the dots and the gradient sums
    row_bytes = n_new * per_user * d * 4.0 * (STEPS + 1)
    emb, loss = kernel(n_new)
    say(f"hrec_tt_fold_in_users d {d}, {STEPS} steps, all {n_new} users in one launch: {ms_all:.2f} ms "
        f"({ms_all / n_new * 1e3:.3f} us per user, clone of the start rows included); {2 * fma / 1e9:.0f} GFLOP f32 -> "
        f"{2 * fma / (ms_all / 1e3) / 1e12:.2f} TFLOP/s; {row_bytes / 1e9:.1f} GB of item-vector rows read (from the "
        f"caches after the first step) -> {row_bytes / (ms_all / 1e3) / 1e12:.2f} TB/s; mean loss "
        f"{float(loss[:, 0].mean()):.4f} -> {float(loss[:, 1].mean()):.4f}")
    sub = min(SUB, n_new)
    r2, y2 = rows[: sub * per_user].view(sub, per_user), ratings[: sub * per_user].view(sub, per_user)
    ms_k = events(lambda: kernel(sub))
    ms_t = events(lambda: torch_way(emb0[:sub], gamma, beta, vec, r2, y2, lr, *adam), reps=3)
    diff = float((kernel(sub)[0] - torch_way(emb0[:sub], gamma, beta, vec, r2, y2, lr, *adam)).abs().max())
    say(f"    the first {sub} users: kernel {ms_k:.3f} ms; the torch formulation (gather once, then {STEPS} steps of "
        f"LayerNorm, two bmm and Adam as elementwise ops, f32): {ms_t:.2f} ms = {ms_t / ms_k:.1f} x; largest "
        f"|difference| between the fitted rows {diff:.3g}")
    del emb0, vec, emb, loss

# ---------------------------------- the same users through train_step (scale only)
eng = DeviceTwoTower(N_OLD + n_new, n_items, 2651, 255, 64, learning_rate=LR, seed=4, device_init=True)
B = 256
bu = torch.as_tensor(rng.integers(N_OLD, N_OLD + n_new, B).astype(np.int32), device=dev)
bi = torch.as_tensor(rng.integers(0, n_items, B).astype(np.int32), device=dev)
bm = torch.as_tensor(rng.integers(0, 2651, B).astype(np.int32), device=dev)
bc = torch.as_tensor(rng.integers(0, 255, B).astype(np.int32), device=dev)
bn = torch.as_tensor(rng.random((B, 2)).astype(np.float32), device=dev)
by = torch.as_tensor((rng.integers(2, 11, B) / 2).astype(np.float32), device=dev)
ms_step = wall(lambda: [eng.train_step(bu, bi, bm, bc, bn, by) for _ in range(20)], reps=3) / 20
n_steps = -(-nnz // B) * STEPS
say(f"for scale only (a different computation: train_step moves every variable and sweeps all four tables): one "
    f"train_step at batch {B} on tables of {N_OLD + n_new} users x {n_items} items, d 64: {ms_step:.3f} ms; "
    f"{STEPS} passes over the {nnz} ratings are {n_steps} steps = {ms_step * n_steps / 1e3:.1f} s projected")
