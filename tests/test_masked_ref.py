"""The masked grid-GP algebra in NumPy (tests/masked_ref.py) against dense K_oo
algebra: the solve, CG / preconditioned CG agreement, and the Schur-identity
log-determinant.  CPU only; the device tests (test_gpu_masked.py) compare the
HIP implementation against the same restatement.

Shapes: RBF factors on linspace(0, 1, m), l_i = 0.1 (1 + 0.05 i), jitter 1e-12,
sigma^2 = 0.01; mask from default_rng(0).choice with the first and last grid
points forced missing.
"""
import numpy as np
import pytest

import masked_ref as mr

S2 = 0.01
CASES = [((7, 5, 3), 0.2), ((12, 10, 8), 0.1)]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _problem(ms, frac):
    F = mr.rbf_factors(ms)
    n = int(np.prod(ms))
    mask = mr.make_mask(n, frac)
    y = np.random.default_rng(1).standard_normal(n)
    return F, mask, y


@pytest.mark.parametrize("ms,frac", CASES)
def test_masked_cg_matches_dense_solve(ms, frac):
    F, mask, y = _problem(ms, frac)
    ex = mr.dense_solve(F, y, mask, S2)
    x, info, it = mr.masked_cg(F, y, mask, S2, rtol=1e-11)
    print("CG", ms, frac, "iters", it, "err", rel(x, ex))
    assert info == 0
    assert rel(x, ex) < 1e-10
    assert np.all(x[~mask] == 0)
    # Y at the missing points is never used
    ynan = np.where(mask, y, np.nan)
    x2, info2, it2 = mr.masked_cg(F, ynan, mask, S2, rtol=1e-11)
    assert info2 == 0 and it2 == it and np.array_equal(x2, x)


@pytest.mark.parametrize("ms,frac", CASES)
def test_pcg_and_cg_reach_the_same_x(ms, frac):
    F, mask, y = _problem(ms, frac)
    ex = mr.dense_solve(F, y, mask, S2)
    x, info, it = mr.masked_cg(F, y, mask, S2, rtol=1e-11)
    xp, infop, itp = mr.masked_cg(F, y, mask, S2, rtol=1e-11, precond='kron')
    print("PCG", ms, frac, "iters", itp, "CG iters", it, "err", rel(xp, ex))
    assert info == 0 and infop == 0
    assert rel(xp, ex) < 1e-10
    assert rel(xp, x) < 1e-10
    assert np.all(xp[~mask] == 0)


@pytest.mark.parametrize("ms,frac", CASES)
def test_schur_logdet_matches_slogdet(ms, frac):
    F, mask, _ = _problem(ms, frac)
    ref = mr.dense_logdet(F, mask, S2)
    ld = mr.schur_logdet(F, mask, S2)
    assert abs(ld - ref) <= 1e-12 * abs(ref)


def test_schur_logdet_without_missing_points_is_the_full_grid():
    F = mr.rbf_factors((7, 5, 3))
    mask = np.ones(105, dtype=bool)
    ref = float(np.linalg.slogdet(mr.dense_K(F) + S2 * np.eye(105))[1])
    assert abs(mr.schur_logdet(F, mask, S2) - ref) <= 1e-12 * abs(ref)


def test_scaled_eigs_is_exact_on_the_full_grid():
    """n = N: the scaling is 1 and the sum runs over every eigenvalue."""
    F = mr.rbf_factors((12, 10, 8))
    full = np.ones(960, dtype=bool)
    ref = float(np.linalg.slogdet(mr.dense_K(F) + S2 * np.eye(960))[1])
    assert abs(mr.scaled_eigs_logdet(F, full, S2) - ref) <= 1e-10 * abs(ref)
    # below the full grid it is an approximation: reported, not asserted
    mask = mr.make_mask(960, 0.1)
    print("scaled_eigs", mr.scaled_eigs_logdet(F, mask, S2), "exact",
          mr.dense_logdet(F, mask, S2))
