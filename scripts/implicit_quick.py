"""Quick timing of the implicit-feedback ALS epoch against the explicit one at
the c2 shape (1M users x 100k items, density 0.5 %, rank 64; one device):
HIP events around each of EPOCHS epochs after a warm-up epoch, medians, and
the two source Gramians (hrec_als_gramian) on their own with their fraction
of the HBM peak. Arguments: [n_users n_items density rank]."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hybrid-als-twotower-recommender_amd"))
from src import _hrec as h  # noqa: E402
from src import synthetic  # noqa: E402
from src.als_engine import DeviceALS  # noqa: E402

a = sys.argv[1:]
n_users, n_items = (int(a[0]), int(a[1])) if len(a) > 1 else (1_000_000, 100_000)
density = float(a[2]) if len(a) > 2 else 0.005
k = int(a[3]) if len(a) > 3 else 64
EPOCHS, HBM_PEAK = 5, 8.0e12  # MI355X: 8 TB/s

csr = synthetic.generate(n_users, n_items, density, False)
csc = synthetic.generate(n_users, n_items, density, True)


def timed(fn, reps):
    """Median ms of `reps` event-timed calls after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


res = {}
for name, kw in (("explicit", {}), ("implicit", {"implicit": True, "alpha": 40.0})):
    eng = DeviceALS(n_users, n_items, k, 0.1, csr, csc, **kw)
    eng.init_user_factors(synthetic.SEED_INIT)
    res[name] = timed(eng.epoch, EPOCHS)
    if kw:
        for side, src in (("users", eng.U), ("items", eng.V)):
            ms = timed(lambda: h.als_gramian(src, k), 20)
            res["gramian_" + side] = ms
            print(f"gramian {side}: {src.shape[0]} x {src.shape[1]} f32, {ms * 1e3:.1f} us, "
                  f"{src.numel() * 4 / (ms * 1e-3) / HBM_PEAK:.3f} of the HBM peak")
    del eng
print(f"explicit epoch {res['explicit']:.2f} ms, implicit epoch {res['implicit']:.2f} ms, "
      f"implicit / explicit {res['implicit'] / res['explicit']:.3f}")
