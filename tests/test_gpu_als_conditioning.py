"""GPU: every ALS half-sweep solver against the extended-precision reference of
tests/als_exact.py on ill-conditioned normal equations (kappa_2 from 1 to
2e11), where the other ALS tests (Gaussian factors, reg 0.1 / 0.5, rtol 1e-5)
only ever see kappa < 100.

Assertion, per row and component, x* the reference, u = 2^-53, N = |x*|_inf:

  |x_gpu,i - x*_i| <= 2^-24 (1 + 2^-20) |x*_i| + rho_max kappa u N

The first term is the f32 rounding of an exactly solved row. For the second,
rho(solver) = max_i (|x_i - x*_i| - 2^-24 |x*_i|)_+ / (kappa u N), and
rho_max = 32 x the largest rho of the C oracle (oracle.build.half_sweep, taken
after its f32 cast: it returns f32) over the rows of the same family and k,
computed in the same run, and at least 1. The 32 = 2^5 is the allowance for
the kernels' 1 / pivot (v_rcp_f64 + one Newton step, about 2^-48, against
2^-53 of a division). The implicit kernel takes the C oracle's rho of the
family's explicit system at the same k: rho is normalised by kappa, so it is
a property of the solver, and the C oracle has no implicit branch.

Every row of every family is asserted; tests/test_als_exact.py shows on the
CPU that the reference and the oracle handle all of them. Each case prints
one "cond ..." line (profiles/als_conditioning.txt is those lines)."""
import numpy as np
import pytest
import torch

import als_exact as ax
from oracle import build as obuild

pytestmark = pytest.mark.gpu
LD = np.longdouble
FAMS = list(ax.FAMILIES)


def _hrec():
    from src import _hrec

    return _hrec


def _to_dev(prob, device):
    return tuple(torch.as_tensor(np.array(a), device=device) for a in prob)  # a copy: the shared problem is read-only


_rho_oracle = {}


def _oracle_rho(name, k, kp):
    """Largest rho of the C oracle over the rows of (family, k) — explicit system."""
    if (name, k, kp) not in _rho_oracle:
        ref = ax.family_reference(name, k, kp)
        got = obuild.half_sweep(*ref["problem"], k, ref["reg"])
        assert np.isfinite(got).all() and (ref["last_step"] < 1e-15).all()
        _rho_oracle[(name, k, kp)] = float(ax.rho(got, ref["x"], ref["kappa"]).max())
    return _rho_oracle[(name, k, kp)]


def _assert_rows(tag, got, x, kappa, k, rho_o, rho_max, unit=ax.U53, zero_rows=(0,)):
    """got f32 [n, kp] against x longdouble [n, k]."""
    assert np.isfinite(got).all(), f"{tag}: non-finite factors"
    assert (got[:, k:] == 0).all(), f"{tag}: padding columns must be exactly zero"
    for r in zero_rows:
        assert (x[r] == 0).all() and (got[r] == 0).all(), f"{tag}: row {r} must be exactly zero"
    rho_g = ax.rho(got[:, :k], x, kappa, unit)
    print(f"cond {tag} kappa_max={kappa.max():.2e} rho_gpu={rho_g.max():.4f} rho_oracle={rho_o:.4f} "
          f"rho_max={rho_max:.3f}")
    err = np.abs(got[:, :k].astype(LD) - x)
    lim = ax.bound(x, kappa, rho_max, unit)
    bad = np.argwhere(err > lim)
    assert bad.size == 0, (f"{tag}: {len(bad)} components outside the bound, first (row, col) {tuple(bad[0])}: "
                           f"err {float(err[tuple(bad[0])]):.3e} > {float(lim[tuple(bad[0])]):.3e}; "
                           f"rho_gpu per row {np.round(rho_g, 3).tolist()}")


def _explicit(tag, name, k, kp, device, runs):
    """runs: callables (dev problem, reg, dst) -> None; all results must be
    bit-identical, with one another and on a second call; the first is
    compared with the reference."""
    ref = ax.family_reference(name, k, kp)
    assert (ref["last_step"] < 1e-15).all()
    dev = _to_dev(ref["problem"], device)
    n = len(ref["kappa"])
    outs = []
    for fill, run in zip((3.0, 5.0, 7.0, 9.0), runs):
        a = torch.full((n, kp), fill, device=device)
        run(dev, ref["reg"], a)
        b = torch.full((n, kp), fill + 1.0, device=device)
        run(dev, ref["reg"], b)
        assert torch.equal(a, b), f"{tag}: two calls must give the same bits"
        outs.append(a)
    for o in outs[1:]:
        assert torch.equal(outs[0], o), f"{tag}: the kernels must agree bit for bit"
    rho_o = _oracle_rho(name, k, kp)
    _assert_rows(f"{tag} {name} k={k} kp={kp}", outs[0].cpu().numpy(), ref["x"], ref["kappa"], k, rho_o,
                 32.0 * max(rho_o, 1.0 / 32.0))


@pytest.mark.parametrize("k,kp", ax.KKP_SMALL)
@pytest.mark.parametrize("name", FAMS)
def test_one_wave_kernels(device, name, k, kp):
    """kp 16 / 32 / 64 through the library's own dispatch, f64 accumulation."""
    h = _hrec()
    _explicit("wave", name, k, kp, device,
              [lambda d, reg, dst: h.als_half_sweep(d[0], d[1], d[2], d[3], k, reg, dst)])


@pytest.mark.parametrize("k", [50, 64])
@pytest.mark.parametrize("name", FAMS)
def test_kp64_kernel_choice(device, name, k):
    """One wave per row, pooled, and both from f64 sources: the same bits on
    ill-conditioned rows too (test_gpu_als_pooled promises it on Gaussian data)."""
    h = _hrec()

    def run(kernel, f64):
        def go(d, reg, dst):
            h.als_half_sweep(d[0], d[1], d[2], d[3], k, reg, dst, src64=h.f32_to_f64(d[3]) if f64 else None,
                             kernel=kernel)
        return go

    _explicit("kp64x4", name, k, 64, device, [run(0, False), run(1, False), run(0, True), run(1, True)])


@pytest.mark.parametrize("k,kp", ax.KKP_WIDE)
@pytest.mark.parametrize("name", FAMS)
def test_wide_kernel(device, name, k, kp):
    """One workgroup per row (csrc/als_wide.hip): its own Gramian, panel and substitutions."""
    h = _hrec()
    _explicit("wide", name, k, kp, device,
              [lambda d, reg, dst: h.als_half_sweep(d[0], d[1], d[2], d[3], k, reg, dst)])


@pytest.mark.parametrize("alpha", ax.ALPHAS)
@pytest.mark.parametrize("k,kp", ax.KKP_IMPLICIT)
@pytest.mark.parametrize("name", FAMS)
def test_implicit_kernel(device, name, k, kp, alpha):
    """yty is the f64 rounding of the reference's longdouble YtY (one rounding
    per entry; als_gramian has its own test)."""
    h = _hrec()
    ref = ax.family_reference(name, k, kp, True, alpha)
    assert (ref["last_step"] < 1e-15).all()
    dev = _to_dev(ref["problem"], device)
    yty = np.zeros((kp, kp))
    yty[:k, :k] = ax.yty_longdouble(ref["problem"][3], k).astype(np.float64)
    d_yty = torch.as_tensor(yty, device=device)
    n = len(ref["kappa"])
    a, b = torch.full((n, kp), 3.0, device=device), torch.full((n, kp), 4.0, device=device)
    for dst in (a, b):
        h.als_half_sweep_implicit(dev[0], dev[1], dev[2], dev[3], k, ref["reg"], alpha, d_yty, dst)
    assert torch.equal(a, b), "two calls must give the same bits"
    rho_o = _oracle_rho(name, k, kp)
    _assert_rows(f"implicit{int(alpha)} {name} k={k} kp={kp}", a.cpu().numpy(), ref["x"], ref["kappa"], k, rho_o,
                 32.0 * max(rho_o, 1.0 / 32.0), zero_rows=(0, ax.NONPOS_ROW))


@pytest.mark.parametrize("k,kp", ax.KKP_SMALL)
@pytest.mark.parametrize("name", ax.MODE1_FAMILIES)
def test_f32_chunk_accumulation(device, name, k, kp):
    """accum_mode 1 sums the Gramian in f32 inside chunks of 16 ratings
    (HREC_ALS_CH1 = 4 pipeline steps of 4 ratings in csrc/als_row.h; each
    chunk is flushed into the f64 accumulators), b stays in f64. A chunk entry
    is a chain of at most 16 f32 fused multiply-adds, so to first order
    |dG_ij| <= 16 * 2^-24 * sum_t |v_ti v_tj| per chunk, and summed over the
    chunks the Gramian carries a relative perturbation |dA| / |A| of 16 * 2^-24.
    First-order perturbation of A x = b, dx = -A^-1 dA x, gives
      |dx|_inf <= kappa * 16 * 2^-24 * |x|_inf,
    which replaces kappa u N in the bound (rho_max = 1: it is the whole
    allowance, the f64 solve's own kappa u is 2^-25 of it).
    Run on the families up to corr2 for which that bound stays below 2^-10
    of |x|_inf, i.e. kappa <= 1024: gauss. corr2 (kappa 2e4 .. 5e4: a bound of
    2 .. 5 %) is beyond it, and so is everything after corr2 — that is the
    documented limit of accum_mode 1, not a failure (the family list is
    checked on the CPU, test_als_exact.test_mode1_families_...)."""
    h = _hrec()
    ref = ax.family_reference(name, k, kp)
    assert ref["kappa"].max() * ax.MODE1_UNIT <= 2.0 ** -10
    dev = _to_dev(ref["problem"], device)
    n = len(ref["kappa"])
    a, b = torch.full((n, kp), 3.0, device=device), torch.full((n, kp), 4.0, device=device)
    for dst in (a, b):
        h.als_half_sweep(dev[0], dev[1], dev[2], dev[3], k, ref["reg"], dst, accum_mode=1)
    assert torch.equal(a, b), "two calls must give the same bits"
    _assert_rows(f"mode1 {name} k={k} kp={kp}", a.cpu().numpy(), ref["x"], ref["kappa"], k, _oracle_rho(name, k, kp),
                 1.0, unit=ax.MODE1_UNIT)


# ---------------------------------------------- exactly singular rows (reg 0)
@pytest.mark.parametrize("k,kp,kernel", [(16, 16, None), (64, 64, 0), (64, 64, 1), (128, 128, None)],
                         ids=["16", "64-wave", "64-pooled", "128-wide"])
def test_singular_row_is_all_nan(device, k, kp, kernel):
    """reg = 0 and a Gramian v v^T (or 2 v v^T) with v in {0, 1, 2}^k: a pivot
    of the LDL^T is exactly 0, rcp gives inf, the Newton step NaN, and the
    NaN reaches every lane in the back substitution. The C oracle returns a
    NaN row there and Spark raises; the contract here is that all kp entries
    are NaN (ALSModel.train turns that into its error sentinel), and that the
    other rows of the launch are what they are without the singular ones."""
    h = _hrec()
    prob, sing = ax.singular_problem(k, kp, np.random.default_rng(k))
    dev = _to_dev(prob, device)
    n = len(prob[0]) - 1
    dst = torch.full((n, kp), 3.0, device=device)
    h.als_half_sweep(dev[0], dev[1], dev[2], dev[3], k, 0.0, dst, kernel=kernel)
    got = dst.cpu().numpy()
    assert np.isnan(got[sing]).all(), f"finite entries in a singular row: {got[sing]}"
    first = sing[0]
    x, kappa = ax.solve_rows(prob[0][:first + 1], prob[1], prob[2], prob[3], k, 0.0)
    orc = obuild.half_sweep(*prob, k, 0.0)
    assert np.isnan(orc[sing]).all()
    rho_o = float(ax.rho(orc[:first], x, kappa).max())
    _assert_rows(f"singular-neighbours k={k} kernel={kernel}", got[:first], x, kappa, k, rho_o,
                 32.0 * max(rho_o, 1.0 / 32.0), zero_rows=())
