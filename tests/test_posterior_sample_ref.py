"""The NumPy restatement of the grid posterior sampler (posterior_sample_ref)
against its definition and the dense posterior: the generator's pinned hashes
and moments, and both sampling routes' draws against N(mu, Sigma) computed
densely.  Shapes as masked_ref: RBF factors (7, 5, 3), y from default_rng(1),
sigma^2 = 0.01, masks from make_mask.

The bounds on the sample statistics are multiples of the statistic's own
standard error under the exact Gaussian law (5 sigma; 6 for the maximum over
the 5460 off-diagonal entries of the whitened covariance), not fitted values;
the seed is fixed, so the tests are deterministic.
"""
import numpy as np
import pytest

import masked_ref as mr
import posterior_sample_ref as ps

S2 = 0.01
MS = (7, 5, 3)
DRAWS = 2000

# h(i), i = 0 .. 7, of (seed 7, stream 3), from a plain-integer evaluation of
# the definition (arbitrary-precision integers reduced mod 2^64)
PINS = [0x71ccaeaa17d67713, 0x5ab66b5153c67970, 0x45abc20942903358, 0x38cc9e034a8b86b3,
        0x8072210d2d0c0406, 0xd87a711d6dc42978, 0x0e3af5697af59585, 0x41d4c8b538fc8785]


def test_hash_pins():
    h = ps.normal_hashes(7, 3, np.arange(8))
    assert h.dtype == np.uint64
    assert [int(v) for v in h] == PINS


def test_hash_is_not_the_probe_hash():
    from oracle.cg import probe_signs
    # the probes' family uses another constant: same (seed, index), other bits
    signs = probe_signs(7, 3, 64)
    mine = np.where((ps.normal_hashes(7, 3, np.arange(64)) >> np.uint64(63)) == 0, 1.0, -1.0)
    assert not np.array_equal(signs, mine)


def test_streams_differ_and_prefix():
    a, b = ps.normal_stream(0, 0, 64), ps.normal_stream(0, 1, 64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert not np.any(a == b)
    assert not np.array_equal(ps.normal_stream(1, 0, 64), a)
    # an odd n takes the cosine half of its last pair
    assert np.array_equal(ps.normal_stream(7, 3, 5), ps.normal_stream(7, 3, 6)[:5])
    assert ps.normal_stream(7, 3, 0).size == 0
    assert ps.normal_stream(7, 3, 1).shape == (1,)


def test_stream_moments():
    from scipy import stats
    n = 1 << 18
    z = ps.normal_stream(0, 0, n)
    zm = abs(z.mean()) * np.sqrt(n)
    zv = abs(z.var() - 1.0) * np.sqrt(n / 2.0)
    p = stats.kstest(z, "norm").pvalue
    print("normal stream n=2^18: mean %.2f sigma, var %.2f sigma, KS p %.3f" % (zm, zv, p))
    assert zm <= 5 and zv <= 5 and p > 1e-4
    assert np.max(np.abs(z)) <= np.sqrt(2 * 53 * np.log(2.0))


def test_coefficient_formulas():
    t = np.array([2.0, 0.5, -1e-14, 0.0])
    z = np.array([1.0, -2.0, 3.0, 0.5])
    yt = np.array([0.3, 0.1, 4.0, -1.0])
    c = ps.posterior_coeffs(t, S2, yt, z)
    assert np.allclose(c[:2], [2 / 2.01 * 0.3 + np.sqrt(2 * S2 / 2.01),
                               0.5 / 0.51 * 0.1 - 2 * np.sqrt(0.5 * S2 / 0.51)], rtol=1e-15)
    # the clamp: a slightly negative eigenvalue adds no noise (and no NaN)
    assert c[2] == t[2] / (t[2] + S2) * yt[2] and c[3] == 0.0
    assert np.array_equal(ps.prior_coeffs(t, z), [np.sqrt(2.0), -2 * np.sqrt(0.5), 0.0, 0.0])
    y = np.array([1.0, np.nan, 2.0, np.nan])
    f = np.array([0.5, 0.5, 0.5, 0.5])
    mask = np.array([True, False, True, False])
    b = ps.residual(y, f, mask, 0.1, z)
    assert np.array_equal(b, [1.0 - 0.5 - 0.1, 0.0, 2.0 - 0.5 - 0.1 * 3.0, 0.0])
    X = np.random.default_rng(3).standard_normal((6, 5))
    mean, m2 = ps.welford(X)
    assert np.allclose(mean, X.mean(axis=1), rtol=1e-14, atol=1e-15)
    assert np.allclose(m2 / 4, X.var(axis=1, ddof=1), rtol=1e-14)


_dense = {}


def dense(frac):
    if frac not in _dense:
        F = mr.rbf_factors(MS)
        Q, lam = mr.factor_eigh(F)
        n = int(np.prod(MS))
        y = np.random.default_rng(1).standard_normal(n)
        mask = mr.make_mask(n, frac) if frac else None
        _dense[frac] = ps.DenseSampler(F, Q, lam, y, mask, S2)
    return _dense[frac]


def check_scores(D, X, what):
    zmean, zvar, off, diag = ps.sample_scores(D, X)
    print("%s: mean %.2f, var %.2f, whitened off-diagonal %.2f, diagonal %.2f (sigma)"
          % (what, zmean, zvar, off, diag))
    assert zmean <= 5
    assert zvar <= 5
    assert off <= 6
    assert diag <= 5


@pytest.mark.parametrize("frac", [0.2, 0])
def test_matheron_route_is_the_posterior(frac):
    D = dense(frac)
    X = D.draws("matheron", 0, DRAWS)
    assert X.shape == (105, DRAWS) and np.all(np.isfinite(X))
    check_scores(D, X, "Matheron, %g missing" % frac)


def test_matheron_ignores_y_at_missing_points():
    D = dense(0.2)
    E = ps.DenseSampler(D.F, D.Q, [np.diag(q.T.dot(f).dot(q)) for f, q in zip(D.F, D.Q)],
                        np.where(D.mask, D.y, np.nan), D.mask, S2)
    a, b = D.matheron_draw(0, 1), E.matheron_draw(0, 1)
    assert np.all(np.isfinite(b)) and np.allclose(a, b, rtol=1e-10, atol=1e-12)


def test_eigenbasis_route_is_the_posterior():
    D = dense(0)
    X = D.draws("eigen", 0, DRAWS)
    check_scores(D, X, "eigenbasis")
    # its mean part alone is the posterior mean
    yt = ps.oracle.kron_matvec(D.QT, D.y)
    mean = ps.oracle.kron_matvec(D.Q, ps.posterior_coeffs(D.t, S2, yt, np.zeros(D.n)))
    assert np.allclose(mean, D.mu, rtol=1e-9, atol=1e-11)


def test_routes_depend_on_eigenvector_signs_but_not_their_law():
    """Flipping eigenvector signs changes the draw (c is indexed by
    eigenvector), which is why device draws are compared with the restatement
    fed the device's eigenpairs; the law does not change."""
    D = dense(0)
    rng = np.random.default_rng(5)
    Q2 = [q * rng.choice([-1.0, 1.0], size=q.shape[1]) for q in D.Q]
    lam = [np.diag(q.T.dot(f).dot(q)) for f, q in zip(D.F, D.Q)]
    E = ps.DenseSampler(D.F, Q2, lam, D.y, None, S2)
    assert not np.allclose(D.eigen_draw(0, 0), E.eigen_draw(0, 0))
    check_scores(E, E.draws("eigen", 0, DRAWS), "eigenbasis, random signs")
