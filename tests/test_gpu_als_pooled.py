"""GPU: the pooled half-sweep kernel (kp 64, f64 accumulation; three waves per
SIMD, 12 waves of a workgroup sharing 8 LDS solve slices, rows claimed one
ticket at a time) returns the one-wave-per-row kernel's factors BIT FOR BIT.
Both kernels are reached through the explicit entry
(hrec_als_half_sweep_kernel: 0 = one wave per row, 1 = pooled), so the test
does not depend on which one the library's own dispatch picks for a shape."""
import numpy as np
import pytest
import torch

from oracle import build as obuild

pytestmark = pytest.mark.gpu

KP = 64
# the row lengths of test_gpu_core.test_half_sweep_window_boundaries: every
# boundary of the gather pipeline (steps of 4 ratings, windows of 64, prefetch)
BOUNDARY_DEG = np.array([0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 67, 95, 96, 97,
                         127, 128, 129, 130, 191, 192, 193, 255, 256, 257, 1000, 1023, 1024, 1025])


def _hrec():
    from src import _hrec

    return _hrec


def _problem(seed, deg, n_src, k, device, force_ends=False):
    rng = np.random.default_rng(seed)
    deg = np.asarray(deg, dtype=np.int64)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = rng.integers(0, n_src, indptr[-1]).astype(np.int32)
    if force_ends:  # the first and the last source row (the buffer range check must keep them)
        indices[::7] = n_src - 1
        indices[3::11] = 0
    values = rng.integers(0, 19, indptr[-1]).astype(np.float32)
    src = np.zeros((n_src, KP), np.float32)
    src[:, :k] = rng.normal(size=(n_src, k)).astype(np.float32)
    dev = (torch.as_tensor(indptr, device=device), torch.as_tensor(indices, device=device),
           torch.as_tensor(values, device=device), torch.as_tensor(src, device=device))
    return (indptr, indices, values, src), dev


def _run(dev, k, kernel, f64, fill=3.0, n_rows=None):
    h = _hrec()
    d_ip, d_ix, d_v, d_src = dev
    n = d_ip.numel() - 1 if n_rows is None else n_rows
    dst = torch.full((n, KP), fill, device=d_src.device)
    h.als_half_sweep(d_ip[: n + 1], d_ix, d_v, d_src, k, 0.1, dst, src64=h.f32_to_f64(d_src) if f64 else None,
                     kernel=kernel)
    return dst


def _both_equal(dev, k, f64, n_rows=None):
    a = _run(dev, k, 0, f64, 3.0, n_rows)
    b = _run(dev, k, 1, f64, 5.0, n_rows)
    assert torch.equal(a, b)
    return b


@pytest.fixture(scope="module")
def boundary(device):
    """The boundary problem at k = 64 and k = 50 with the oracle's factors of
    the first (computed once, read only)."""
    host64, dev64 = _problem(11, BOUNDARY_DEG, 301, 64, device, force_ends=True)
    _, dev50 = _problem(13, BOUNDARY_DEG, 301, 50, device, force_ends=True)
    exp = obuild.half_sweep(host64[0], host64[1], host64[2], host64[3], 64, 0.1)
    return {64: dev64, 50: dev50, "exp": exp}


@pytest.mark.parametrize("f64", [False, True], ids=["f32src", "f64src"])
@pytest.mark.parametrize("k", [64, 50])
def test_pooled_pipeline_boundaries(device, boundary, k, f64):
    got = _both_equal(boundary[k], k, f64)
    if k == 50:
        assert (got[:, k:] == 0).all(), "padding columns must stay zero"
    assert (got[0] == 0).all(), "a row without ratings has no factor"
    if k == 64 and not f64:  # the first case: also against the C oracle
        np.testing.assert_allclose(got.cpu().numpy(), boundary["exp"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("n_rows", [1, 11, 12, 13])
def test_pooled_fewer_rows_than_waves(device, n_rows):
    """Waves that claim no row leave without touching a slice."""
    rng = np.random.default_rng(n_rows)
    _, dev = _problem(20 + n_rows, rng.integers(1, 200, n_rows), 97, 64, device)
    _both_equal(dev, 64, False)
    _both_equal(dev, 64, True)


def test_pooled_every_wave_loops(device):
    """12 waves x CU count x 2 + 5 rows of ~40 ratings: every wave claims
    several rows and every slice is reused."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    n_rows = 12 * cus * 2 + 5
    rng = np.random.default_rng(5)
    _, dev = _problem(31, rng.integers(30, 51, n_rows), 500, 64, device)
    _both_equal(dev, 64, False)
    _both_equal(dev, 64, True)


@pytest.mark.parametrize("long_row", [False, True], ids=["short", "one-long-row"])
def test_pooled_slice_contention(device, long_row):
    """5,000 rows of 1-4 ratings: all 12 waves of a workgroup reach the solve
    together and queue for the 8 slices; then the same with one 20,000-rating
    row in the middle."""
    rng = np.random.default_rng(6)
    deg = rng.integers(1, 5, 5000)
    if long_row:
        deg[2500] = 20000
    _, dev = _problem(32, deg, 400, 64, device)
    _both_equal(dev, 64, True)
    _both_equal(dev, 64, False)


def test_pooled_empty_input(device):
    h = _hrec()
    _, dev = _problem(33, np.zeros(40, np.int64), 10, 64, device)
    # no rating at all: the CSR arrays are empty but must be non-null for the C entry
    dev = (dev[0], torch.zeros(1, dtype=torch.int32, device=device), torch.zeros(1, device=device), dev[3])
    for f64 in (False, True):
        assert (_run(dev, 64, 1, f64) == 0).all()
    # n_rows = 0: nothing to do, no launch
    dst = torch.full((4, KP), 2.0, device=device)
    h.als_half_sweep(dev[0][:1], dev[1], dev[2], dev[3], 64, 0.1, dst, kernel=1)
    assert (dst == 2.0).all()


def test_pooled_repeatable(device, boundary):
    a = _run(boundary[64], 64, 1, True)
    b = _run(boundary[64], 64, 1, True, fill=7.0)
    assert torch.equal(a, b)


def test_pooled_two_streams_have_private_tickets(device):
    """Two launches in flight on two streams, disjoint outputs: both complete
    and both are right (a shared row counter would make each skip rows)."""
    rng = np.random.default_rng(8)
    _, dev_a = _problem(41, rng.integers(100, 400, 3000), 800, 64, device)
    _, dev_b = _problem(42, rng.integers(100, 400, 3000), 800, 64, device)
    exp_a, exp_b = _run(dev_a, 64, 0, False), _run(dev_b, 64, 0, False)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(device=device), torch.cuda.Stream(device=device)
    with torch.cuda.stream(sa):
        got_a = _run(dev_a, 64, 1, False, fill=5.0)
    with torch.cuda.stream(sb):
        got_b = _run(dev_b, 64, 1, False, fill=6.0)
    torch.cuda.synchronize()
    assert torch.equal(got_a, exp_a)
    assert torch.equal(got_b, exp_b)


def test_engine_fit_same_bits_with_either_kernel(device):
    """DeviceALS.fit(3) on 600 x 300, k = 64, with the module-level override
    forcing each kernel on both sides: the factors are equal bit for bit."""
    from src import als_engine, synthetic

    n_users, n_items, k = 600, 300, 64
    csr = synthetic.generate(n_users, n_items, 0.05, False)
    csc = synthetic.generate(n_users, n_items, 0.05, True)
    out = {}
    old = als_engine.HALF_SWEEP_KERNEL
    try:
        for kernel in (0, 1):
            als_engine.HALF_SWEEP_KERNEL = kernel
            eng = als_engine.DeviceALS(n_users, n_items, k, 0.1, csr, csc)
            eng.init_user_factors(synthetic.SEED_INIT)
            eng.fit(3)
            out[kernel] = (eng.user_factors.clone(), eng.item_factors.clone())
    finally:
        als_engine.HALF_SWEEP_KERNEL = old
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
