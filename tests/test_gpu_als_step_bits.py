"""The rank-64 ALS half-sweep keeps every factor bit.

The other half-sweep suites compare kernels built from the same gram_row /
factor_row with each other and with the oracle at a tolerance, on integer
ratings 0..18: a change of bits shared by all kernels would pass them. Here
the factors are compared word for word (float32 bit patterns, NaN payloads
included) with tests/golden/als_half_sweep_bits.npz, recorded on an MI355X
before the instruction trim of the step loop and the solve, over

* the window-boundary row lengths of test_half_sweep_window_boundaries plus
  2047, 2048 and 2049, at k 64 and 50, reg_param 0.1 and 0.0 (at 0.0 every
  row shorter than k has a singular Gramian: whatever the unpivoted LDL^T
  makes of it is part of the expected output, any NaN included — in the
  record rounding leaves small pivots, and no word of it is a NaN);
* ratings that exercise the f32 -> f64 conversion of the step (fractions,
  negatives, +-0, f32 denormals, 2^-126, 3e38);
* the non-negative half-sweep, which runs the same gram_row.

The inputs are regenerated from the seeds stored in the file; all four paths
(one wave per row / pooled, f32 / f64 sources) must give the recorded words.
make_cases() is also what the recording script ran."""
import os

import numpy as np
import pytest
import torch
from conftest import GOLDEN

from oracle import build as obuild

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "als_half_sweep_bits.npz")
KP, N_SRC = 64, 301
DEG = np.array([0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 67, 95, 96, 97,
                127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 1000, 1023, 1024, 1025,
                2047, 2048, 2049])
SEEDS = {"boundary": 2101, "frac": 2102, "mixed": 2103, "nonneg": 2104}
SPECIAL = np.array([0.0, -0.0, 1e-40, -3e-42, 2.0 ** -126, 3e38], np.float64).astype(np.float32)
PATHS = [(0, False), (1, False), (0, True), (1, True)]  # (kernel, f64 sources)


def _csr(rng, deg):
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, N_SRC, indptr[-1]).astype(np.int32)
    indices[::7] = N_SRC - 1
    indices[3::11] = 0
    return indptr, indices


def _frac(rng, n):
    return (3.0 * rng.normal(size=n)).astype(np.float32)


def _sources(rng, k):
    src = np.zeros((N_SRC, KP), np.float32)
    src[:, :k] = rng.normal(size=(N_SRC, k)).astype(np.float32)
    return src


def make_cases(seeds):
    """name -> (indptr, indices, values, src, k, reg_param); `nonneg` is the
    non-negative solver's problem, the others the Cholesky half-sweep's."""
    cases = {}
    for k in (64, 50):
        rng = np.random.default_rng(int(seeds["boundary"]) + k)
        indptr, indices = _csr(rng, DEG)
        values = rng.integers(0, 19, indptr[-1]).astype(np.float32)
        src = _sources(rng, k)
        for reg in (0.1, 0.0):
            cases[f"boundary_k{k}_reg{reg}"] = (indptr, indices, values, src, k, reg)
    rng = np.random.default_rng(int(seeds["frac"]))
    indptr, indices = _csr(rng, DEG)
    cases["frac"] = (indptr, indices, _frac(rng, indptr[-1]), _sources(rng, 64), 64, 0.1)
    rng = np.random.default_rng(int(seeds["mixed"]))
    indptr, indices = _csr(rng, DEG)
    values = _frac(rng, indptr[-1])
    pick = rng.integers(0, 2 * len(SPECIAL), indptr[-1])  # half fractions, half the special values
    values = np.where(pick < len(SPECIAL), SPECIAL[pick % len(SPECIAL)], values).astype(np.float32)
    cases["mixed"] = (indptr, indices, values, _sources(rng, 64), 64, 0.1)
    rng = np.random.default_rng(int(seeds["nonneg"]))
    deg = rng.integers(1, 150, 70)
    deg[0], deg[1], deg[2] = 0, 1, 3 * 64 + 5
    indptr, indices = _csr(rng, deg)
    cases["nonneg"] = (indptr, indices, _frac(rng, indptr[-1]), _sources(rng, 64), 64, 0.1)
    return cases


def run_paths(h, device, case, nonneg=False):
    """The factors of every path as uint32 words: [(label, array)]."""
    indptr, indices, values, src, k, reg = case
    d_ip = torch.as_tensor(indptr, dtype=torch.int64, device=device)
    d_ix = torch.as_tensor(indices, dtype=torch.int32, device=device)
    d_v = torch.as_tensor(values, dtype=torch.float32, device=device)
    d_src = torch.as_tensor(src, device=device)
    n_rows = len(indptr) - 1
    out = []
    if nonneg:
        dst = torch.full((n_rows, KP), 3.0, device=device)
        h.als_half_sweep_nonneg(d_ip, d_ix, d_v, d_src, k, reg, dst)
        return [("nonneg", dst.cpu().numpy().view(np.uint32))]
    s64 = h.f32_to_f64(d_src)
    for kernel, f64src in PATHS:
        dst = torch.full((n_rows, KP), 3.0, device=device)
        h.als_half_sweep(d_ip, d_ix, d_v, d_src, k, reg, dst, kernel=kernel, src64=s64 if f64src else None)
        out.append((f"kernel={kernel} src64={f64src}", dst.cpu().numpy().view(np.uint32)))
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(FIXTURE) as z:
        fx = {name: z[name] for name in z.files}
    seeds = {name[len("seed_"):]: int(fx[name]) for name in fx if name.startswith("seed_")}
    assert seeds == SEEDS
    return fx, make_cases(seeds)


def _assert_words(got, exp, what):
    assert got.dtype == np.uint32 and got.shape == exp.shape
    nan_got, nan_exp = np.isnan(got.view(np.float32)), np.isnan(exp.view(np.float32))
    assert np.array_equal(nan_got, nan_exp), f"{what}: NaN positions differ"
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} differ from the recorded bits"


@pytest.mark.parametrize("name", ["boundary_k64_reg0.1", "boundary_k64_reg0.0", "boundary_k50_reg0.1",
                                  "boundary_k50_reg0.0", "frac", "mixed"])
def test_half_sweep_bits_match_recorded(device, golden, name):
    from src import _hrec as h

    fx, cases = golden
    exp = fx[name]
    assert exp.nbytes == 4 * KP * len(DEG)
    if name.endswith("reg0.0"):  # the singular rows are in the record
        nan_rows = np.isnan(exp.view(np.float32)).all(axis=1)
        print(name, "all-NaN rows of lengths", DEG[nan_rows].tolist())
    for label, got in run_paths(h, device, cases[name]):
        _assert_words(got, exp, f"{name} {label}")


def test_half_sweep_fractional_ratings_match_oracle(device, golden):
    from src import _hrec as h

    _, cases = golden
    indptr, indices, values, src, k, reg = cases["frac"]
    exp = obuild.half_sweep(indptr, indices, values, src, k, reg)
    for label, got in run_paths(h, device, cases["frac"]):
        np.testing.assert_allclose(got.view(np.float32), exp, rtol=1e-5, atol=1e-6, err_msg=label)


def test_nonneg_half_sweep_bits_match_recorded(device, golden):
    from src import _hrec as h

    fx, cases = golden
    (label, got), = run_paths(h, device, cases["nonneg"], nonneg=True)
    _assert_words(got, fx["nonneg"], label)
