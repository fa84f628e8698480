"""Quick timing of the pairwise two-tower kernels (TwoTowerModel.transform /
regression_metrics) at the c2 tables (1M users, 100k candidate items; one
device), embedding sizes 64 and 50, 2^24 pairs: users and candidate rows drawn
uniformly, labels uniform in [0, 5]; the weights are the engine's device init.
Each pair list is timed once sorted by user (a user's row repeats across
neighbouring pairs) and once in a random permutation. HIP events around each
call; per order the calls are warmed up once, then timed REPS times in
alternation (new, parent, new, ...), the median reported.
 (a) tt_pair_sums: the kernel over the distinct users' vectors (hrec_tt_pair_metrics);
 (b) tt_predict_pairs: the same, writing the predictions;
 (c) DeviceTwoTower.pair_sums from user ids: torch.unique + the user tower over
     the distinct users + (a);
 (d) the formulation before this kernel: user_vectors(user) per row, then
     hrec_tt_pair_score over the rows torch gathers from the candidate vectors,
     then the ten sums in torch (f64).
Per kernel line: ms, ns per pair, the algorithmic bytes (two d-float rows + two
int64 row indices per pair, + the f64 label for the sums, + the f32 output for
the predictions) and their rate as a fraction of the 6.29 TB/s measured HBM
copy rate. Rows served from the caches make a fraction above 1 possible.
Arguments: [n_users n_items n_pairs]."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src.tt_engine import DeviceTwoTower  # noqa: E402

a = sys.argv[1:]
n_users, n_items = (int(a[0]), int(a[1])) if len(a) > 1 else (1_000_000, 100_000)
n = int(a[2]) if len(a) > 2 else 1 << 24
REPS, HBM = 5, 6.29e12
dev = torch.device("cuda", torch.cuda.current_device())


def timed(fns):
    """Median ms of each of fns: one warm-up call each, then REPS rounds that
    time them in turn."""
    ms = [[] for _ in fns]
    for rep in range(REPS + 1):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep:
                ms[j].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def torch_sums(pred, y):
    """The ten HREC_PAIR_* sums by torch reductions (f64)."""
    ok = ~torch.isnan(pred)
    p = torch.where(ok, pred, torch.zeros_like(pred)).double()
    yy = torch.where(ok, y, torch.zeros_like(y))
    e = yy - p
    return torch.stack([ok.sum().double(), (~ok).sum().double(), e.sum(), e.abs().sum(), (e * e).sum(), yy.sum(),
                        (yy * yy).sum(), p.sum(), (p * p).sum(), (yy * p).sum()])


for d in (64, 50):
    eng = DeviceTwoTower(n_users, n_items, 30, 10, d, seed=d, device_init=True)
    g = torch.Generator(device=dev).manual_seed(d)
    cand = eng.item_vectors(torch.arange(n_items, dtype=torch.int32, device=dev),
                            torch.randint(0, 30, (n_items,), generator=g, dtype=torch.int32, device=dev),
                            torch.randint(0, 10, (n_items,), generator=g, dtype=torch.int32, device=dev),
                            torch.rand((n_items, 2), generator=g, dtype=torch.float32, device=dev))
    users = torch.randint(0, n_users, (n,), generator=g, dtype=torch.int32, device=dev)
    items = torch.randint(0, n_items, (n,), generator=g, dtype=torch.int64, device=dev)
    y = torch.rand(n, generator=g, dtype=torch.float64, device=dev) * 5.0
    order = torch.argsort(users)
    print(f"d = {d}: {n_users} users x {n_items} candidates, {n} pairs; user vectors "
          f"{n_users * d * 4 / 1e6:.0f} MB, candidate vectors {n_items * d * 4 / 1e6:.0f} MB")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    for name, sel in (("sorted by user", order), ("random order", None)):
        us, it, yy = (users, items, y) if sel is None else (users[sel], items[sel], y[sel])
        uniq, urows = torch.unique(us, return_inverse=True)
        uvec = eng.user_vectors(uniq.to(torch.int32))

        def parent():
            return torch_sums(h.tt_pair_score(eng.user_vectors(us), cand[it]), yy)

        t_sums, t_pred, t_eng, t_par = timed([lambda: h.tt_pair_sums(uvec, urows, cand, it, yy),
                                              lambda: h.tt_predict_pairs(uvec, urows, cand, it, out=out),
                                              lambda: eng.pair_sums(us, cand, it, yy), parent])
        for label, ms, extra in (("(a) tt_pair_sums", t_sums, 8), ("(b) tt_predict_pairs", t_pred, 4)):
            nbytes = n * (2 * d * 4 + 16 + extra)
            print(f"  {label}, {name}: {ms:.2f} ms, {ms * 1e6 / n:.3f} ns per pair, {nbytes / 1e9:.1f} GB algorithmic, "
                  f"{nbytes / ms / 1e9:.2f} TB/s = {nbytes / (ms * 1e-3) / HBM:.2f} of the HBM copy rate")
        print(f"  (c) engine pair_sums from ids ({uniq.numel()} distinct users), {name}: {t_eng:.2f} ms, "
              f"{t_eng * 1e6 / n:.3f} ns per pair")
        print(f"  (d) user tower per row + tt_pair_score on gathered rows + torch sums, {name}: {t_par:.2f} ms, "
              f"{t_par * 1e6 / n:.3f} ns per pair; (d) / (c) = {t_par / t_eng:.2f}, (d) / (a) = {t_par / t_sums:.2f}")
        new, old = eng.pair_sums(us, cand, it, yy), parent()
        same_pred = torch.equal(out.view(torch.int32),
                                h.tt_pair_score(eng.user_vectors(us), cand[it]).view(torch.int32))
        print(f"  predictions bit-equal to (d)'s: {same_pred}; largest relative difference of the ten sums: "
              f"{((new - old).abs() / old.abs().clamp_min(1e-300)).max().item():.2e}; "
              f"rmse {(new[4] / new[0]).sqrt().item():.6f}")
        del uvec, urows, uniq
    del eng, cand, out
