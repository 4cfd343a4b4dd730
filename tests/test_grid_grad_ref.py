"""CPU checks of tests/grid_grad_ref.py, the dense reference the device tests
of the grid model's analytic gradient compare against: the kernel-parameter
derivatives against central differences of oracle.cov_1d, the dense gradient
against central differences of the dense LML (complete and masked grid), the
Kronecker-sum trace against the dense trace, the probe estimator against the
exact traces, and the float64 evaluation against the bounds the device tests
assert (the bounds are neither vacuous nor too tight for NumPy's own float64).
"""
import numpy as np
import pytest

import oracle

import grid_grad_ref as G
import grief_abi_ref as R
import masked_ref as MR


@pytest.mark.parametrize("kind", G.KINDS)
def test_param_derivatives_match_central_differences(kind):
    """Relative step 1e-6 (truncation O(h^2)); agreement to 1e-7 max|dk|."""
    g = np.linspace(0.0, 1.0, 9)
    var, ls = 1.3, 0.27
    dk = G.dk_1d(kind, g, var, ls)
    for name, at in (('variance', lambda h: (var + h, ls)), ('lengthscale', lambda h: (var, ls + h))):
        h = 1e-6 * (var if name == 'variance' else ls)
        fd = (oracle.cov_1d(kind, g, g, *at(h)) - oracle.cov_1d(kind, g, g, *at(-h))) / (2 * h)
        err = np.max(np.abs(fd - dk[name]))
        assert err <= 1e-7 * np.max(np.abs(dk[name])), (kind, name, err)


def test_delta_rbf_lengthscale_derivative_is_zero():
    g = np.linspace(0.0, 1.0, 5)
    assert np.array_equal(G.dk_1d("RBF", g, 1.3, 1e-7)['lengthscale'], np.zeros((5, 5)))
    assert np.array_equal(G.dk_1d("RBF", g, 1.3, 1e-7)['variance'], np.eye(5))


@pytest.mark.parametrize("kind", range(4))
@pytest.mark.parametrize("D", (1, 3))
def test_float64_derivatives_meet_the_device_bound(kind, D):
    rng = np.random.default_rng(5 + D)
    x, z = rng.random((33, D)), rng.random((17, D))
    for ls in (0.3, 2.0):
        for which in (0, 1):
            ref, t = G.grad_param_ref(kind, 1.3, ls, x, z, which)
            got = G.grad_param_ref(kind, 1.3, ls, x, z, which, np.float64)[0]
            bound = R.cov_bound(D, ref, t) if which == 0 else G.grad_param_bound(D, ref, t)
            assert np.all(np.abs(got.astype(G.LD) - ref) <= bound)
            assert np.max(np.abs(got.astype(G.LD) - ref) / bound) > 1e-3


@pytest.mark.parametrize("missing", (0, 25))
def test_dense_gradient_matches_central_differences(missing):
    """4 x 5 x 6, RBF / Matern32 / Matern52, s = 0.01, lengthscales 0.2 - 0.3,
    complete and with 25 missing points: 1e-6 relative on every free parameter."""
    p = G.mixed_problem((4, 5, 6), missing=missing)
    g, fd = G.dense_grad(p), G.central_diff_grad(p)
    rel = np.abs(g - fd)[p.free] / np.abs(g)[p.free]
    print("dense gradient vs central differences, relative:", rel)
    assert np.all(rel <= 1e-6), rel


def test_kronecker_sum_trace_equals_dense_trace():
    p = G.mixed_problem((4, 5, 6))
    _, tr = G.dense_parts(p)
    kt = G.kron_traces(p)
    cond = np.linalg.cond(G.dense_A(p))
    assert np.all(np.abs(kt - tr) <= 1e3 * G.U53 * cond * np.abs(tr)), (kt, tr)


def test_trace_ratio_reference():
    """The long-double grid sum equals the Kronecker-sum form, and numerator
    = lam at shift 0 sums to N."""
    p = G.mixed_problem((4, 5, 6))
    lam, rows = G.trace_rows(p)
    ms = [l.size for l in lam]
    num = np.stack([np.concatenate(r) for r in rows])
    vals, scales = G.trace_ratio_ref(ms, np.concatenate(lam), num, p.s)
    assert np.all(np.abs(vals - G.kron_traces(p)) <= 1e-12 * scales)
    lamv = np.random.default_rng(0).uniform(0.5, 2.0, sum(ms))
    v, sc = G.trace_ratio_ref(ms, lamv, lamv[None, :], 0.0)
    assert abs(v[0] - p.N) <= G.trace_ratio_bound(3, sc)[0]


def test_trace_ratio_chain_of_the_test_shapes():
    """The issue's shapes keep one thread's chain within 16 additions (the 64
    of the bound covers chain + 34); the long-run shape states its own."""
    for ms in [(7,), (5, 4), (6, 5, 4), (3, 4, 2, 5), (4, 1, 3), (2,) * 12, (33, 17, 9),
               (84, 84, 84), (1024, 1024, 2)]:
        assert G.trace_ratio_chain(ms) <= 16, ms
    assert G.trace_ratio_chain((84, 84, 84)) == 16
    assert G.trace_ratio_chain((1024, 1024, 2)) == 4          # two grid-stride passes
    assert G.trace_ratio_chain((640, 640, 72)) == 72          # whole runs of the last factor


def test_unit_vector_probes_sum_to_the_exact_traces():
    p = G.mixed_problem((6, 5, 4), missing=0)
    p.mask = MR.make_mask(p.N, 0.2)
    o = np.nonzero(p.mask)[0]
    Z = np.zeros((p.N, o.size))
    Z[o, np.arange(o.size)] = 1.0
    per, _ = G.probe_estimates(p, 0, Z=Z)
    _, tr = G.dense_parts(p)
    assert np.allclose(per.sum(axis=0), tr, rtol=1e-10, atol=0)
    # Rademacher probes: an unbiased estimator, here only its shape and the
    # noise column's sign
    per, _ = G.probe_estimates(p, 3, probes=4)
    assert per.shape == (4, 1 + 2 * p.d) and np.all(per[:, 0] > 0)


def test_forward_differences_agree_at_the_checkgrad_point():
    """BaseModel.checkgrad compares the analytic gradient with forward
    differences at step 1e-6 to 3 decimals of their ratio: at the device
    test's point (6 x 5 x 4) the dense forward differences are within 1e-3."""
    p = G.mixed_problem((6, 5, 4))
    g, fd = G.dense_grad(p), G.forward_diff_grad(p)
    rel = np.abs(fd - g)[p.free] / np.abs(g)[p.free]
    print("forward differences vs gradient, relative:", rel)
    assert np.all(rel <= 1e-3), rel
    assert np.all(np.abs(g[p.free]) > 1e-2)      # away from the optimum
