"""The per-point-noise restatement (noise_ref.py) against dense K_oo + D_oo
algebra, on the CPU: what the device tests in test_gpu_noise.py compare the
weighted CG, Lanczos and model with is itself checked here.

Shapes and masks as the masked CG tests (masked_ref.py); noise_var = 0.01 and
noise_scale two decades wide (noise_ref.noise_scale).
Bounds, from the algebra and not from the figures:
  CG at rtol: |x - x*| / |x*| <= cond(A) |r| / |b| < cond(A) rtol.
  Lanczos, first steps of two routes: rounding, 1e-12 of max|alpha| as
    test_masked_lanczos_ref.py.
  Lanczos run to n_obs steps: Gauss quadrature with k nodes is exact for
    polynomials of degree 2k - 1, so in exact arithmetic k = n_obs gives
    z^T log(A) z; in floating point the recurrence is an exact one for a
    matrix whose eigenvalues lie within ~eps |A| of A's (Greenbaum 1989), a
    relative change of eps cond(A) in the small ones and as much in their
    logs: bound 100 n_obs eps cond(A) of sum |log lam|.
  LML: |y.(alpha - alpha*)| <= |y| |alpha*| cond(A) rtol, plus 1e-12 |LML|.
Measured figures are printed.
"""
import os
import re

import numpy as np
import pytest

import masked_ref as mr
import noise_ref as nr
import oracle

from conftest import ROOT

RTOL = 1e-11
EPS = np.finfo(np.float64).eps


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


def cond(C):
    lam = np.linalg.eigvalsh(C["A"][0])
    return float(lam[-1] / lam[0])


@pytest.mark.parametrize("ms,frac", nr.CG_CASES)
def test_weighted_cg_vs_dense(ms, frac):
    C = nr.case(ms, frac)
    x, info, it = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL)
    _, _, ito = oracle.cg_solve(nr.weighted_op(C["F"], C["mask"], C["noise"]),
                                np.where(C["mask"], C["y"], 0.0), rtol=RTOL)
    k = cond(C)
    print("weighted CG", ms, frac, "iters", it, "oracle", ito, "err", rel(x, C["x"]), "cond", k)
    assert info == 0
    assert rel(x, C["x"]) < k * RTOL
    assert np.all(x[~C["mask"]] == 0)
    # the split p.K p + sum d p^2 against the plain recurrence on the operator
    assert abs(it - ito) <= 0.05 * ito, (it, ito)


@pytest.mark.parametrize("ms,frac", nr.CG_CASES)
def test_weighted_cg_ignores_the_missing_points(ms, frac):
    C = nr.case(ms, frac)
    x, _, it = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL)
    x2, _, it2 = nr.weighted_cg(C["F"], np.where(C["mask"], C["y"], np.nan), C["mask"],
                                np.where(C["mask"], C["noise"], np.nan), rtol=RTOL)
    assert it2 == it and np.array_equal(x2, x)


@pytest.mark.parametrize("ms,frac", nr.CG_CASES)
def test_preconditioned_cg_vs_dense(ms, frac):
    C = nr.case(ms, frac)
    x, info, it = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL, precond='kron')
    _, _, it0 = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL)
    print("weighted PCG", ms, frac, "iters", it, "unpreconditioned", it0, "err", rel(x, C["x"]))
    assert info == 0
    assert rel(x, C["x"]) < cond(C) * RTOL
    assert np.all(x[~C["mask"]] == 0)


def test_constant_noise_is_the_scalar_masked_cg():
    C = nr.case((12, 10, 8), 0.1)
    s = 0.01
    x, info, it = nr.weighted_cg(C["F"], C["y"], C["mask"], np.full(960, s), rtol=RTOL)
    xs, infos, its = mr.masked_cg(C["F"], C["y"], C["mask"], s, rtol=RTOL)
    ex = mr.dense_solve(C["F"], C["y"], C["mask"], s)
    assert info == 0 and infos == 0
    assert rel(x, ex) < 1e-8 and rel(xs, ex) < 1e-8
    assert abs(it - its) <= 0.05 * its


@pytest.mark.parametrize("ms,frac", [((7, 5, 3), 0.2), ((16, 12), 0.3), ((12, 10, 8), 0.3),
                                     ((8, 6, 5, 4), 0.3), ((9, 8, 7), 0.0)])
def test_tridiagonal_is_the_compressed_one(ms, frac):
    C = nr.case(ms, frac)
    a, b = nr.weighted_lanczos(C["F"], C["mask"], C["noise"], 7, 2, 8)
    Aoo, o = C["A"]
    z = oracle.cg.probe_signs(7, 2, C["mask"].size)[o]
    ad, bd = oracle.lanczos_tridiag(lambda v: Aoo.dot(v), z, 8)
    scale = np.max(np.abs(ad))
    ea, eb = np.max(np.abs(a - ad)) / scale, np.max(np.abs(b - bd)) / scale
    print("tridiagonal", ms, frac, "alpha", ea, "beta", eb)
    assert a.size == 8 and b.size == 7
    assert ea <= 1e-12 and eb <= 1e-12


@pytest.mark.parametrize("ms,frac", [((7, 5, 3), 0.2), ((12, 10, 8), 0.3)])
def test_full_lanczos_is_the_exact_quadrature(ms, frac):
    C = nr.case(ms, frac)
    Aoo, o = C["A"]
    lam, U = np.linalg.eigh(Aoo)
    bound = 100.0 * o.size * EPS * (lam[-1] / lam[0]) * float(np.sum(np.abs(np.log(lam))))
    for probe in (0, 1, 2):
        a, b = nr.weighted_lanczos(C["F"], C["mask"], C["noise"], 3, probe, o.size)
        k = a.size
        q = oracle.cg.quadrature_logdet(a, b[:k - 1], 1.0) * float(o.size)
        z = oracle.cg.probe_signs(3, probe, C["mask"].size)[o]
        exact = float(np.sum(U.T.dot(z) ** 2 * np.log(lam)))
        print("full Lanczos", ms, frac, "probe", probe, "steps", k, "quadrature", q, "exact",
              exact, "bound", bound)
        assert abs(q - exact) <= bound


@pytest.mark.parametrize("ms,frac", nr.CG_CASES)
def test_lml_is_the_gaussian_log_density(ms, frac):
    C = nr.case(ms, frac)
    Aoo, o = C["A"]
    yo = C["y"][o]
    # the density by a Cholesky factor: another route than solve + slogdet
    L = np.linalg.cholesky(Aoo)
    u = np.linalg.solve(L, yo)
    dens = -0.5 * float(u.dot(u)) - float(np.sum(np.log(np.diag(L)))) \
        - 0.5 * o.size * np.log(2 * np.pi)
    dl = nr.dense_lml(C["F"], C["y"], C["mask"], C["noise"], C["A"])
    alpha, info, _ = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL)
    cl = nr.lml(C["y"], alpha, nr.dense_logdet(C["F"], C["mask"], C["noise"], C["A"]), C["mask"])
    slack = 0.5 * np.linalg.norm(yo) * np.linalg.norm(C["x"]) * cond(C) * RTOL
    print("LML", ms, frac, "density", dens, "dense", dl, "cg", cl, "slack", slack)
    assert info == 0
    assert abs(dl - dens) <= 1e-12 * abs(dens)
    assert abs(cl - dens) <= slack + 1e-12 * abs(dens)


def test_slq_estimator_within_three_standard_errors():
    C = nr.case((12, 10, 8), 0.3)
    mean, ests = nr.weighted_slq(C["F"], C["mask"], C["noise"], probes=16, steps=40, seed=3)
    ld = nr.dense_logdet(C["F"], C["mask"], C["noise"], C["A"])
    se = float(np.std(ests)) / 4.0
    print("weighted slq mean", mean, "dense", ld, "se", se)
    assert abs(mean - ld) <= 3.0 * se


def test_abi_declares_and_exports_the_noise_entry_points():
    from gp_grief_amd import native
    src = open(os.path.join(ROOT, "include", "gp_grief_amd.h")).read()
    declared = re.findall(r"^int (gg_\w+)\(", src, re.M)
    lib = native.load()
    for name in ("gg_cgm_set_noise", "gg_lanczos_probe_masked_noise", "gg_sample_residual_noise"):
        assert name in declared
        assert name in native.SIGNATURES
        assert hasattr(lib, name)
    # the weighted probe takes the noise vector where the scalar one takes shift
    plain = native.SIGNATURES["gg_lanczos_probe_masked"]
    noisy = native.SIGNATURES["gg_lanczos_probe_masked_noise"]
    assert len(noisy) == len(plain) and noisy[2:] == plain[2:]
    plain = native.SIGNATURES["gg_sample_residual"]
    noisy = native.SIGNATURES["gg_sample_residual_noise"]
    assert len(noisy) == len(plain) and noisy[:2] == plain[:2] and noisy[4:] == plain[4:]
