"""The masked Lanczos / SLQ restatement (masked_lanczos_ref.py) against dense
K_oo algebra, on the CPU: what the device tests in test_gpu_masked_lanczos.py
compare gg_lanczos_probe_masked with is itself checked here.

Shapes, masks and sigma^2 = 0.01 as the masked CG tests (masked_ref.py).
Tolerances: the first Lanczos steps of the two routes differ by rounding
(measured 2e-15 of max|alpha|; bound 1e-12); long runs lose orthogonality and
the tridiagonals drift apart, the quadrature does not (measured at most 3.4e-7
|log det| at 20, 40 and 80 steps; bound 1e-5); the estimator's error is held
to three standard errors of its own 16 probes (measured within 1.6).
"""
import os
import re

import numpy as np
import pytest

import masked_lanczos_ref as mlr
import masked_ref as mr
import oracle

from conftest import ROOT

S2 = 0.01


@pytest.mark.parametrize("ms,frac", mlr.CASES)
def test_tridiagonal_is_the_compressed_one(ms, frac):
    C = mlr.case(ms, frac, S2)
    a, b = mlr.masked_lanczos(C["F"], C["mask"], S2, 7, 2, 8)
    ad, bd = mlr.dense_masked_lanczos(C["F"], C["mask"], S2, 7, 2, 8)
    scale = np.max(np.abs(ad))
    ea, eb = np.max(np.abs(a - ad)) / scale, np.max(np.abs(b - bd)) / scale
    print("tridiagonal", ms, frac, "alpha", ea, "beta", eb)
    assert a.size == 8 and b.size == 7
    assert ea <= 1e-12 and eb <= 1e-12


@pytest.mark.parametrize("ms,frac", mlr.CASES)
def test_quadrature_of_the_two_routes(ms, frac):
    C = mlr.case(ms, frac, S2)
    F, mask = C["F"], C["mask"]
    o = np.nonzero(mask)[0]
    Koo = mr.dense_K(F)[np.ix_(o, o)]
    worst = 0.0
    for steps in (20, 40, 80):
        for probe in (0, 1):
            a, b = mlr.masked_lanczos(F, mask, S2, 3, probe, steps)
            ad, bd = mlr.dense_masked_lanczos(F, mask, S2, 3, probe, steps, Koo=Koo)
            q = oracle.cg.quadrature_logdet(a, b, float(o.size))
            qd = oracle.cg.quadrature_logdet(ad, bd, float(o.size))
            worst = max(worst, abs(q - qd) / abs(C["ld"]))
    print("quadrature", ms, frac, "worst", worst)
    assert worst <= 1e-5


@pytest.mark.parametrize("ms,frac", mlr.CASES)
def test_estimator_within_three_standard_errors(ms, frac):
    C = mlr.case(ms, frac, S2)
    mean, ests = C["slq"]
    se = float(np.std(ests)) / 4.0
    print("slq", ms, frac, "mean", mean, "dense", C["ld"], "se", se,
          "err/se", abs(mean - C["ld"]) / se)
    assert ests.size == 16
    assert abs(mean - C["ld"]) <= 3.0 * se


def test_masked_probe_is_the_unmasked_one_zeroed():
    C = mlr.case((7, 5, 3), 0.2, S2)
    mask = C["mask"]
    # Lanczos normalises the start vector: n_obs nonzero entries of 1 / sqrt(n_obs)
    a, _ = mlr.masked_lanczos(C["F"], mask, S2, 7, 2, 1)
    z = np.where(mask, oracle.cg.probe_signs(7, 2, mask.size), 0.0)
    K = mr.dense_K(C["F"])
    assert abs(a[0] - (z.dot(K.dot(z)) / mask.sum() + S2)) <= 1e-12 * abs(a[0])


def test_abi_declares_and_exports_the_masked_probe():
    from gp_grief_amd import native
    src = open(os.path.join(ROOT, "include", "gp_grief_amd.h")).read()
    declared = re.findall(r"^int (gg_\w+)\(", src, re.M)
    lib = native.load()
    for name in ("gg_lanczos_probe_masked", "gg_lanczos_probe_masked_timed"):
        assert name in declared
        assert name in native.SIGNATURES
        assert hasattr(lib, name)
    # the timed twin takes the same arguments plus the per-step times
    plain = native.SIGNATURES["gg_lanczos_probe_masked"]
    timed = native.SIGNATURES["gg_lanczos_probe_masked_timed"]
    assert len(timed) == len(plain) + 1 and timed[:-2] == plain[:-1] and timed[-1] == plain[-1]
