"""GPU: the non-negative half-sweep (csrc/als_nonneg.hip, nnls_row) where its
iteration branches, against tests/nnls_oracle.py in the natural order. The
Gaussian problems of tests/test_gpu_als_nonneg.py stop within about 100
iterations on step < 1e-7 or ndir < 1e-12 nx; the cases here
(nnls_oracle.hard_cases(), pinned on the CPU by tests/test_nnls_oracle.py)
reach the rest:

  scaled_up   step < 1e-7 at x = 0: Spark's answer is the exact zero vector
  tiny        explicit: the 1e-20 guard of the step length gives exact zeros;
              implicit: it makes every step minute and the rows run to the cap
  ties        duplicated source columns: two entries reach the bound in one
              step, the evidence for the wave-minimum wall rule
  graded, short8, scaled_down, gauss   long runs, tiny entries, the control
  corr2, corr3   rows at the cap on an iterate that no two faithful
              implementations share

Every row: finite, >= 0, padding exactly 0, 0 <= iters <= max(400, 20 k), an
unsolved row exactly 0 with 0 iterations, two calls the same bits.

Stable rows: |got - exp| <= 1e-5 max|exp_row| with no absolute term (ten
times what six summation orders of the oracle differ by; tiny and scaled_down
have entries near 1e-12 and 1e-6, so an absolute term would make them
vacuous); an all-zero exp is met exactly with 0 iterations; rows that every
order runs to the cap do so on the device; iters > 0 where the oracle's are.

Unstable rows (nnls_oracle.unstable_rows: two pinned rows, and the rows of
corr2 / corr3 with more than one rating): the invariants, iters >= 2, the cap
where every order reaches it, and f(got) <= f(x_32) + 1e-9 |f(x_32)| with
f(x) = x^T A x / 2 - b^T x in longdouble and x_32 the oracle's iterate after
32 steps: every accepted step is an exact line search along a descent
direction cut at the bound, so f never increases.

Each case prints one "nnls ..." line (profiles/nnls_conditioning.txt is those
lines)."""
import numpy as np
import pytest
import torch

import nnls_oracle as no

pytestmark = pytest.mark.gpu


def _hrec():
    from src import _hrec

    return _hrec


def _id(case):
    return "%s-%d-%s" % (case[0], case[1], no.mode_key(case[3], case[4]))


def _run(h, device, prob, reg, k, kp, imp, alpha):
    """(factors [rows, kp], iterations) of one launch; a second launch must give the same bits."""
    indptr, indices, values, src = (torch.as_tensor(np.array(a), device=device) for a in prob)  # copies: prob is shared
    n = indptr.numel() - 1
    assert n <= 11 and int(np.diff(prob[0]).max()) <= 257
    yty = h.als_gramian(src, k) if imp else None
    outs = []
    for fill in (3.0, -5.0):
        dst = torch.full((n, kp), fill, device=device)
        iters = torch.full((n,), -1, dtype=torch.int32, device=device)
        h.als_half_sweep_nonneg(indptr, indices, values, src, k, reg, dst, implicit=imp, alpha=alpha, yty=yty,
                                iters=iters)
        outs.append((dst.cpu().numpy(), iters.cpu().numpy()))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)), "two calls must give the same bits"
    assert np.array_equal(outs[0][1], outs[1][1]), "two calls must give the same iteration counts"
    return outs[0]


@pytest.mark.parametrize("case", no.hard_cases(), ids=_id)
def test_nonneg_half_sweep_where_the_iteration_branches(device, case):
    name, k, kp, imp, alpha = case
    ref = no.hard_reference(*case)
    got, iters = _run(_hrec(), device, ref["problem"], ref["reg"], k, kp, imp, alpha)
    exp, exp_iters, eqs = ref["exp"], ref["iters"], ref["eqs"]
    cap = no.iter_max(k)
    solved = [r for r, eq in enumerate(eqs) if eq is not None]
    unsolved = [r for r, eq in enumerate(eqs) if eq is None]
    loose = no.unstable_rows(*case)
    stable = [r for r in solved if r not in loose]
    at_cap = no.cap_rows(name, k, imp, alpha)

    bound = 1e-5 * np.abs(exp.astype(np.float64)).max(axis=1, keepdims=True)
    err = np.abs(got[:, :k].astype(np.float64) - exp)
    with np.errstate(all="ignore"):
        rel = np.where(err == 0, 0.0, err / bound)  # inf where an all-zero row is not met exactly
    f_ratio = {}
    for r in loose:
        A, b = eqs[r]
        f_ratio[r] = (no.objective(A, b, got[r, :k]), no.objective(A, b, ref["x32"][r]))
    print("nnls %s k=%d %s err/bound=%.2e iters gpu %s oracle %s f(got)/f(x32) %s" % (
        name, k, no.mode_key(imp, alpha), float(rel[stable].max()) if stable else 0.0, iters.tolist(),
        exp_iters.tolist(), {r: round(float(f / f32), 9) for r, (f, f32) in f_ratio.items()}))

    assert np.isfinite(got).all() and (got >= 0).all(), "every factor is finite and >= 0, exactly"
    assert (got[:, k:] == 0).all(), "padding columns must be exactly zero"
    assert (iters >= 0).all() and (iters <= cap).all()
    assert 0 in unsolved and len(unsolved) == (2 if imp else 1)
    for r in unsolved:
        assert (got[r] == 0).all() and iters[r] == 0, "row %d has no system: exactly zero, no iteration" % r

    for r in stable:
        assert (err[r] <= bound[r]).all(), "row %d: err / bound %.3f" % (r, float(rel[r].max()))
        if (exp[r] == 0).all():
            assert (got[r] == 0).all() and iters[r] == 0, "row %d: Spark stops before the first step" % r
        if exp_iters[r] > 0:
            assert iters[r] > 0, "row %d: solved rows take iterations" % r
    for r in loose:
        f, f32 = f_ratio[r]
        assert f <= f32 + 1e-9 * abs(f32), "row %d: f(got) %.12g above f(x_32) %.12g" % (r, float(f), float(f32))
        assert iters[r] >= 2
    for r in at_cap:
        assert exp_iters[r] == cap and iters[r] == cap, "row %d runs to the cap in every summation order" % r
