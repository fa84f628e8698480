"""The c2 half-sweeps per side and kernel (0 = one wave per row, 1 = pooled),
interleaved in one process and event-timed: item side (f32 sources), user
side (f64 sources) and user side with f32 sources; the first round checks
that both kernels give the same bits.
usage: python scripts/als_sides.py [reps] [out.json]
(HREC_LIB selects an A/B library of scripts/build_als_variants.sh; ALS_SIDES_SMALL=1 runs c2s)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as g  # noqa: E402

g._paths()
import torch  # noqa: E402
from src import _hrec, synthetic  # noqa: E402
from src.als_engine import DeviceALS  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out = sys.argv[2] if len(sys.argv) > 2 else None
n_users, n_items, dens, k = 1_000_000, 100_000, 0.005, 64
if os.environ.get("ALS_SIDES_SMALL"):
    n_users, n_items = 100_000, 20_000
csr = synthetic.generate(n_users, n_items, dens, False)
csc = synthetic.generate(n_users, n_items, dens, True)
eng = DeviceALS(n_users, n_items, k, 0.1, csr, csc)
eng.init_user_factors(synthetic.SEED_INIT)
eng.epoch()
torch.cuda.synchronize()
print("setup done", flush=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


V64 = _hrec.f32_to_f64(eng.V)
res = {"item": {0: [], 1: []}, "user": {0: [], 1: []}, "user32": {0: [], 1: []}}
ref = {}
for r in range(reps + 1):
    for kern in (0, 1):
        dst_i = torch.empty_like(eng.V)
        ti = timed(lambda: _hrec.als_half_sweep(csc.indptr, csc.indices, csc.values, eng.U, k, 0.1, dst_i, kernel=kern))
        dst_u = torch.empty_like(eng.U)
        tu = timed(lambda: _hrec.als_half_sweep(csr.indptr, csr.indices, csr.values, eng.V, k, 0.1, dst_u, src64=V64,
                                                kernel=kern))
        dst_w = torch.empty_like(eng.U)
        tw = timed(lambda: _hrec.als_half_sweep(csr.indptr, csr.indices, csr.values, eng.V, k, 0.1, dst_w, kernel=kern))
        if r == 0:  # warm-up round: check the bits instead
            if kern == 0:
                ref = {"i": dst_i, "u": dst_u}
            else:
                print("bit-identical item", torch.equal(ref["i"], dst_i), "user", torch.equal(ref["u"], dst_u), flush=True)
            continue
        res["item"][kern].append(round(ti, 3))
        res["user"][kern].append(round(tu, 3))
        res["user32"][kern].append(round(tw, 3))
        print(r, kern, "item", round(ti, 3), "user", round(tu, 3), "user32", round(tw, 3), flush=True)
print(json.dumps(res))
if out:
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f)
