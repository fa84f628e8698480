"""GPU: bench.py's plain run and --dump-outputs on the quick configuration
(c2s: 100,000 users x 20,000 items, 0.5 %, rank 64).

* a plain run prints one JSON line with the headline keys, `steps` timed
  epochs, and none of the --full sub-lines;
* --dump-outputs writes the factors the LAST timed epoch left (not a later
  epoch's), float32, whole when they fit, else the same seeded row sample in
  every run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUB_LINES = ("cpu_baseline", "scoring", "hybrid_top5", "ingest", "tt_item_vectors_c4", "tt_scoring_c4",
             "hybrid_top5_c5", "tt_train", "api_hybrid_call", "als_rank256", "als_c3")


def _fit(cfg, epochs):
    from src import synthetic
    from src.als_engine import DeviceALS

    csr = synthetic.generate(cfg["users"], cfg["items"], cfg["density"], False)
    csc = synthetic.generate(cfg["users"], cfg["items"], cfg["density"], True)
    eng = DeviceALS(cfg["users"], cfg["items"], cfg["rank"], 0.1, csr, csc)
    eng.init_user_factors(synthetic.SEED_INIT)
    eng.fit(epochs)
    torch.cuda.synchronize()
    return eng


@pytest.mark.gpu
def test_plain_run_line_and_dumped_factors(device, tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "c2s", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "epochs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"])
    for key in SUB_LINES:
        assert line[key] is None, key
    assert sorted(os.listdir(out)) == ["item_factors.npy", "user_factors.npy"]
    cfg = bench.CONFIGS["c2s"]
    V = np.load(out / "item_factors.npy")
    U = np.load(out / "user_factors.npy")
    assert V.dtype == np.float32 and U.dtype == np.float32
    assert V.shape == (cfg["items"], cfg["rank"])
    assert V.nbytes + U.nbytes <= 64_000_000
    # 1 warmup + 2 timed epochs of the same fit, nothing after them
    eng = _fit(cfg, 3)
    assert np.array_equal(V, eng.item_factors.cpu().numpy())
    # the user side (25.6 MB) fits whole
    assert np.array_equal(U, eng.user_factors.cpu().numpy())


@pytest.mark.gpu
def test_dump_samples_a_large_matrix_with_fixed_rows(device, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    cfg = dict(users=3001, items=517, density=0.05, rank=16)
    eng = _fit(cfg, 1)
    monkeypatch.setattr(bench, "DUMP_BYTES_PER_ARRAY", 1000 * 16 * 4)  # 1000 rows of rank 16
    bench.dump_outputs(eng, str(tmp_path))
    V, U = np.load(tmp_path / "item_factors.npy"), np.load(tmp_path / "user_factors.npy")
    assert np.array_equal(V, eng.item_factors.cpu().numpy())  # 517 rows: whole
    rows = np.sort(np.random.default_rng(2).choice(3001, 1000, replace=False))
    assert U.shape == (1000, 16) and U.dtype == np.float32
    assert np.array_equal(U, eng.user_factors.cpu().numpy()[rows])
    bench.dump_outputs(eng, str(tmp_path / "again"))
    assert np.array_equal(U, np.load(tmp_path / "again" / "user_factors.npy"))
