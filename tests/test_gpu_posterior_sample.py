"""Posterior sampling on the MI355X (gg_sample.hip, linalg.GridPosteriorSampler,
GPGridModel.sample_posterior / posterior_moments) against the NumPy restatement
in posterior_sample_ref.py and the dense posterior.

Shapes as masked_ref: RBF factors on linspace(0, 1, m), l_i = 0.1 (1 + 0.05 i),
jitter 1e-12, sigma^2 = 0.01, y from default_rng(1), masks from make_mask.
(7, 5, 3): N = 105 is odd (pair tails, a run of the last factor of odd length);
(48, 6, 5) and (12, 10, 8): more than one block of pairs.

Eigenvectors are defined up to sign and a draw depends on the signs, so every
model draw is compared with the restatement fed the model's own eigenpairs
(m._schur()).

Tolerances.  gg_normal_fill against NumPy: |z| <= sqrt(2 53 ln 2) = 8.6; FP64
log and sincos are good to a few ulp and the rounding of 2 pi u2 adds under
1e-15 to the cosine, so two correct implementations differ by under 5e-14;
the absolute tolerance is 20 x that, NORMAL_TOL = 1e-12.  The coefficient
kernels add a relative 1e-12 (a handful of roundings in the decode and the
formula) on top of the generator's absolute tolerance times the coefficient of
z.  The draws: 1e-10 norm-wise through the exact route (the Kronecker matvec's
accuracy class), 1e-8 through a converged solve (the project's converged-solve
tolerance).  The statistics are 6 sigma bounds of the exact Gaussian law.
"""
import ctypes

import numpy as np
import pytest

import masked_ref as mr
import posterior_sample_ref as ps

pytestmark = pytest.mark.gpu

S2 = 0.01
NORMAL_TOL = 1e-12
GG_OK, GG_ERR_VALUE = 0, -1


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ------------------------------------------------------------ gg_normal_fill
@pytest.mark.parametrize("n", [1, 2, 105, 4097, (1 << 20) + 3])
def test_normal_fill(nat, n):
    import torch
    buf = torch.full((n + 4,), 777.0, dtype=torch.float64, device="cuda")
    ref = ps.normal_stream(7, 3, n)
    for off in (0, 1):      # 16-byte lanes; a view one double in: 8-byte lanes
        buf.fill_(777.0)
        z = buf[off:off + n]
        assert z.data_ptr() % 16 == 8 * off
        assert nat.lib().gg_normal_fill(7, 3, nat.dptr(z), n, nat.stream_ptr()) == GG_OK
        got = host(buf)
        err = np.max(np.abs(got[off:off + n] - ref))
        print("gg_normal_fill n=%d offset %d: max abs err %.3e" % (n, off, err))
        assert err <= NORMAL_TOL
        # nothing before the vector or after z[n - 1] is written
        assert np.all(got[:off] == 777.0) and np.all(got[off + n:] == 777.0)


def test_normal_fill_streams_and_refusals(nat):
    import torch
    L, sp = nat.lib(), nat.stream_ptr
    n = 64
    z = torch.full((n,), 777.0, dtype=torch.float64, device="cuda")
    for args in ((7, -1, nat.dptr(z), n), (7, 65536, nat.dptr(z), n), (7, 3, None, n),
                 (7, 3, nat.dptr(z), -1)):
        assert L.gg_normal_fill(*args, sp()) == GG_ERR_VALUE
        assert torch.all(z == 777.0)
    assert L.gg_normal_fill(7, 3, nat.dptr(z), 0, sp()) == GG_OK     # no-op
    assert torch.all(z == 777.0)
    assert L.gg_normal_fill(7, 65535, nat.dptr(z), n, sp()) == GG_OK
    assert np.max(np.abs(host(z) - ps.normal_stream(7, 65535, n))) <= NORMAL_TOL
    assert L.gg_normal_fill((5 << 32) | 7, 0, nat.dptr(z), n, sp()) == GG_OK   # low 32 bits
    assert np.max(np.abs(host(z) - ps.normal_stream(7, 0, n))) <= NORMAL_TOL


# ------------------------------------------------- the coefficient kernels
def eig_tables(ms):
    """Per-factor eigenvalues of rbf_factors(ms), one of them set slightly
    negative (the clamp), and their Kronecker product."""
    lam = [l.copy() for l in mr.factor_eigh(mr.rbf_factors(ms))[1]]
    lam[1][0] = -1e-9
    return lam, mr.kron_eigs(lam)


@pytest.mark.parametrize("ms", [(7, 5, 3), (48, 6, 5)])
def test_coefficient_kernels(nat, ms):
    import torch
    L, sp = nat.lib(), nat.stream_ptr
    lam, t = eig_tables(ms)
    assert t.min() < 0
    n, d = t.size, len(ms)
    m = nat.i64_array(ms)
    lamd = dev(np.concatenate(lam))
    rng = np.random.default_rng(2)
    yt = rng.standard_normal(n)
    z = ps.normal_stream(11, 4, n)
    for off in (0, 1):
        ybuf = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
        cbuf = torch.full((n + 2,), 777.0, dtype=torch.float64, device="cuda")
        ytd, c = ybuf[off:off + n], cbuf[off:off + n]
        ytd.copy_(dev(yt))
        # posterior coefficients
        assert L.gg_kron_posterior_coeffs(d, m, nat.dptr(lamd), S2, nat.dptr(ytd), 11, 4,
                                          nat.dptr(c), sp()) == GG_OK
        ref = ps.posterior_coeffs(t, S2, yt, z)
        gain = np.sqrt(np.maximum(t, 0.0) * S2 / (t + S2))
        got = host(cbuf)
        err = np.abs(got[off:off + n] - ref)
        print("posterior_coeffs %r offset %d: max err %.3e" % (ms, off, err.max()))
        assert np.all(err <= 1e-12 * np.abs(ref) + NORMAL_TOL * gain + 1e-300)
        assert np.all(got[:off] == 777.0) and np.all(got[off + n:] == 777.0)
        # prior coefficients
        cbuf.fill_(777.0)
        assert L.gg_kron_prior_coeffs(d, m, nat.dptr(lamd), 11, 4, nat.dptr(c), sp()) == GG_OK
        ref = ps.prior_coeffs(t, z)
        got = host(cbuf)
        err = np.abs(got[off:off + n] - ref)
        print("prior_coeffs %r offset %d: max err %.3e" % (ms, off, err.max()))
        assert np.all(err <= 1e-12 * np.abs(ref) + NORMAL_TOL * np.sqrt(np.maximum(t, 0.0)))
        assert np.all(got[off:off + n][t < 0] == 0.0)
        assert np.all(got[:off] == 777.0) and np.all(got[off + n:] == 777.0)


@pytest.mark.parametrize("ms", [(7, 5, 3), (48, 6, 5)])
def test_sample_residual(nat, ms):
    import torch
    L, sp = nat.lib(), nat.stream_ptr
    n = int(np.prod(ms))
    mask = mr.make_mask(n, 0.2)
    rng = np.random.default_rng(3)
    y = np.where(mask, rng.standard_normal(n), np.nan)     # NaN at the missing points
    f = rng.standard_normal(n)
    z = ps.normal_stream(5, 9, n)
    sd = 0.1
    md = dev(mask.astype(np.uint8))
    for off in (0, 1):
        bufs = [torch.zeros(n + 2, dtype=torch.float64, device="cuda") for _ in range(2)]
        bbuf = torch.full((n + 2,), 777.0, dtype=torch.float64, device="cuda")
        yd, fd, b = bufs[0][off:off + n], bufs[1][off:off + n], bbuf[off:off + n]
        yd.copy_(dev(y))
        fd.copy_(dev(f))
        for mk, mref in ((md, mask), (None, None)):
            bbuf.fill_(777.0)
            mp = None if mk is None else ctypes.c_void_p(mk.data_ptr())
            assert L.gg_sample_residual(nat.dptr(yd), nat.dptr(fd), mp, sd, 5, 9, nat.dptr(b), n,
                                        sp()) == GG_OK
            got = host(bbuf)
            ref = ps.residual(y, f, mref, sd, z)
            if mref is None:     # no mask: the NaN of y passes, compare the finite part
                assert np.array_equal(np.isnan(got[off:off + n]), ~mask)
                sel = mask
            else:
                assert np.all(got[off:off + n][~mask] == 0.0)      # exact zeros, no NaN
                sel = np.ones(n, dtype=bool)
            err = np.abs(got[off:off + n][sel] - ref[sel])
            assert np.all(err <= 1e-12 * np.abs(ref[sel]) + NORMAL_TOL * sd)
            assert np.all(got[:off] == 777.0) and np.all(got[off + n:] == 777.0)


@pytest.mark.parametrize("n", [105, 1440])
def test_sample_accumulate(nat, n):
    import torch
    L, sp = nat.lib(), nat.stream_ptr
    rng = np.random.default_rng(4)
    F, W = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
    X = F + W
    for off in (0, 1):
        bufs = [torch.full((n + 2,), 777.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        out, mean, m2 = (v[off:off + n] for v in bufs)
        assert all(v.data_ptr() % 16 == 8 * off for v in (out, mean, m2))
        for k in range(5):
            fd, wd = dev(F[:, k]), dev(W[:, k])
            assert L.gg_sample_accumulate(nat.dptr(fd), nat.dptr(wd), nat.dptr(out),
                                          nat.dptr(mean), nat.dptr(m2), k + 1, n, sp()) == GG_OK
            assert np.array_equal(host(out), X[:, k])
        got = np.stack([host(v) for v in bufs])
        assert np.allclose(got[1, off:off + n], X.mean(axis=1), rtol=1e-13, atol=1e-13)
        assert np.allclose(got[2, off:off + n] / 4, X.var(axis=1, ddof=1), rtol=1e-13, atol=0)
        assert np.all(got[:, :off] == 777.0) and np.all(got[:, off + n:] == 777.0)
    # the moments alone, the draw alone, and the draw written over f
    fd, wd = dev(F[:, 0]), dev(W[:, 0])
    mean, m2 = dev(np.zeros(n)), dev(np.full(n, 5.0))
    assert L.gg_sample_accumulate(nat.dptr(fd), nat.dptr(wd), None, nat.dptr(mean),
                                  nat.dptr(m2), 1, n, sp()) == GG_OK
    assert np.array_equal(host(mean), X[:, 0]) and np.all(host(m2) == 0.0)
    assert L.gg_sample_accumulate(nat.dptr(fd), nat.dptr(wd), nat.dptr(fd), None, None, 0, n,
                                  sp()) == GG_OK
    assert np.array_equal(host(fd), X[:, 0])


def test_sampling_refusals(nat):
    import torch
    L, sp = nat.lib(), nat.stream_ptr
    ms = (7, 5, 3)
    lam, t = eig_tables(ms)
    n = t.size
    lamd = dev(np.concatenate(lam))
    v = dev(np.ones(n))
    out = torch.full((n,), 777.0, dtype=torch.float64, device="cuda")
    out2 = torch.full((n,), 777.0, dtype=torch.float64, device="cuda")
    m3, lp, vp, op = nat.i64_array(ms), nat.dptr(lamd), nat.dptr(v), nat.dptr(out)
    m17 = nat.i64_array([2] * 17)
    zero = nat.i64_array((7, 0, 3))
    bad_post = [(0, m3, lp, S2, vp, 1, 0, op), (17, m17, lp, S2, vp, 1, 0, op),
                (3, None, lp, S2, vp, 1, 0, op), (3, zero, lp, S2, vp, 1, 0, op),
                (3, m3, None, S2, vp, 1, 0, op), (3, m3, lp, S2, None, 1, 0, op),
                (3, m3, lp, S2, vp, 1, 0, None), (3, m3, lp, S2, vp, 1, 65536, op),
                (3, m3, lp, S2, vp, 1, -1, op), (3, m3, lp, 0.0, vp, 1, 0, op)]
    for a in bad_post:
        assert L.gg_kron_posterior_coeffs(*a, sp()) == GG_ERR_VALUE, a
    bad_prior = [(0, m3, lp, 1, 0, op), (17, m17, lp, 1, 0, op), (3, None, lp, 1, 0, op),
                 (3, zero, lp, 1, 0, op), (3, m3, None, 1, 0, op), (3, m3, lp, 1, 0, None),
                 (3, m3, lp, 1, 65536, op)]
    for a in bad_prior:
        assert L.gg_kron_prior_coeffs(*a, sp()) == GG_ERR_VALUE, a
    bad_res = [(None, vp, None, 0.1, 1, 0, op, n), (vp, None, None, 0.1, 1, 0, op, n),
               (vp, vp, None, 0.1, 1, 0, None, n), (vp, vp, None, 0.1, 1, 0, op, -1),
               (vp, vp, None, 0.1, 1, 65536, op, n)]
    for a in bad_res:
        assert L.gg_sample_residual(*a, sp()) == GG_ERR_VALUE, a
    o2 = nat.dptr(out2)
    bad_acc = [(None, vp, op, None, None, 1, n), (vp, None, op, None, None, 1, n),
               (vp, vp, op, o2, None, 1, n), (vp, vp, op, None, o2, 1, n),
               (vp, vp, op, o2, o2, 0, n), (vp, vp, op, None, None, 1, -1)]
    for a in bad_acc:
        assert L.gg_sample_accumulate(*a, sp()) == GG_ERR_VALUE, a
    assert L.gg_sample_residual(vp, vp, None, 0.1, 1, 0, op, 0, sp()) == GG_OK      # no-ops
    assert L.gg_sample_accumulate(vp, vp, op, None, None, 1, 0, sp()) == GG_OK
    torch.cuda.synchronize()
    assert torch.all(out == 777.0) and torch.all(out2 == 777.0)


# ------------------------------------------------------------ model draws
def grid_model(gg, ms, y, mask=None, **kw):
    """GPGridModel whose operator has masked_ref.rbf_factors(ms) (cov_grid
    reverses the input dimensions: input j is factor d - 1 - j)."""
    d = len(ms)
    ls = [0.1 * (1 + 0.05 * i) for i in range(d)]
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=ls[d - 1 - j]) for j in range(d)]
    xg = [np.linspace(0, 1, ms[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    kw.setdefault("cg_rtol", 1e-11)
    return gg.models.GPGridModel(xg, y, gg.kern.GridKernel(kerns), noise_var=S2, mask=mask, **kw)


def restatement(m, y, mask):
    """posterior_sample_ref.DenseSampler on the model's factors and eigenpairs."""
    m.parameters        # settle the parameter cache: the sampler sees these eigenpairs
    Q, T = m._schur()
    F = [np.asarray(f, dtype=np.float64) for f in m._operator().K]
    lam = [np.asarray(e, dtype=np.float64).reshape(-1) for e in T.diag().K]
    return ps.DenseSampler(F, [np.asarray(q) for q in Q.K], lam, y, mask, S2)


def problem(ms, frac):
    n = int(np.prod(ms))
    y = np.random.default_rng(1).standard_normal(n)
    return y, (mr.make_mask(n, frac) if frac else None)


def test_model_draws_exact(gg):
    ms = (7, 5, 3)
    y, _ = problem(ms, 0)
    m = grid_model(gg, ms, y.reshape(-1, 1), solver='exact')
    D = restatement(m, y, None)
    assert np.allclose(D.K, mr.dense_K(mr.rbf_factors(ms)), rtol=1e-12, atol=1e-14)
    X = m.sample_posterior(4, seed=3)
    assert isinstance(X, np.ndarray) and X.shape == (105, 4)
    for k in range(4):
        err = rel(X[:, k], D.eigen_draw(3, k))
        print("exact route draw %d: rel err %.3e" % (k, err))
        assert err <= 1e-10
    # deterministic in the seed, changes with it, column k is draw k
    assert np.array_equal(m.sample_posterior(4, seed=3), X)
    assert np.array_equal(m.sample_posterior(2, seed=3), X[:, :2])
    assert rel(m.sample_posterior(1, seed=4)[:, 0], X[:, 0]) > 0.01
    smp = m._sampler(3)
    assert smp.route == 'eigen'
    for k in range(4):
        assert np.array_equal(host(smp.draw(k)), X[:, k])
    # seed=None is the model's seed (0)
    assert np.array_equal(m.sample_posterior(1), m.sample_posterior(1, seed=0))
    with pytest.raises(ValueError):
        smp.draw(32768)
    with pytest.raises(ValueError):
        smp.draw(-1)
    with pytest.raises(ValueError):
        m.sample_posterior(0)


def test_model_draws_cg(gg):
    ms = (7, 5, 3)
    y, _ = problem(ms, 0)
    m = grid_model(gg, ms, y.reshape(-1, 1), solver='cg')
    D = restatement(m, y, None)
    X = m.sample_posterior(2, seed=3)
    assert m._sampler(3).route == 'matheron' and m._sampler(3).mask is None
    for k in range(2):
        err = rel(X[:, k], D.matheron_draw(3, k))
        print("cg route draw %d: rel err %.3e" % (k, err))
        assert err <= 1e-8


@pytest.mark.parametrize("ms,frac,precond,on_device",
                         [((7, 5, 3), 0.2, None, False), ((12, 10, 8), 0.3, 'kron', False),
                          ((48, 6, 5), 0.1, None, True)])
def test_model_draws_masked(gg, ms, frac, precond, on_device):
    import torch
    y, mask = problem(ms, frac)
    ynan = np.where(mask, y, np.nan).reshape(-1, 1)      # never read where missing
    Y = dev(ynan) if on_device else ynan
    m = grid_model(gg, ms, Y, mask=mask, precond=precond)
    D = restatement(m, np.where(mask, y, 0.0), mask)
    X = m.sample_posterior(4, seed=1)
    if on_device:
        assert isinstance(X, torch.Tensor) and X.is_cuda and tuple(X.shape) == (y.size, 4)
        X = host(X)
    else:
        assert isinstance(X, np.ndarray) and X.shape == (y.size, 4)
    assert np.all(np.isfinite(X))
    for k in range(4):
        err = rel(X[:, k], D.matheron_draw(1, k))
        print("masked route %r %g draw %d: rel err %.3e" % (ms, frac, k, err))
        assert err <= 1e-8
    smp = m._sampler(1)
    assert smp._cg is m._masked_cg()          # the model's resident solver
    for k in range(4):
        assert np.array_equal(host(smp.draw(k)), X[:, k])
    assert np.array_equal(host(m.sample_posterior(4, seed=1)) if on_device
                          else m.sample_posterior(4, seed=1), X)
    assert rel(host(m._sampler(2).draw(0)), X[:, 0]) > 0.01
    # sampling invalidates nothing: the fit and the imputed mean are unchanged
    mean = m.predict_grid(compute_var=False)[0]
    mean = host(mean) if on_device else mean
    assert rel(mean, D.mu) <= 1e-8
    with pytest.raises(ValueError, match="compute_var=False"):
        m.predict_grid(compute_var=True)


def test_sampler_follows_the_parameters(gg):
    ms = (7, 5, 3)
    y, mask = problem(ms, 0.2)
    m = grid_model(gg, ms, y.reshape(-1, 1), mask=mask)
    a = m.sample_posterior(1, seed=0)
    p = m.parameters
    p2 = p.copy()
    p2[0] = 0.04
    m.parameters = p2
    b = m.sample_posterior(1, seed=0)
    assert rel(b, a) > 1e-3
    m.parameters = p
    assert np.array_equal(m.sample_posterior(1, seed=0), a)


def test_posterior_moments_equal_the_draws(gg):
    ms = (7, 5, 3)
    y, mask = problem(ms, 0.2)
    m = grid_model(gg, ms, y.reshape(-1, 1), mask=mask)
    X = m.sample_posterior(64, seed=2)
    mean, var = m.posterior_moments(64, seed=2)
    assert mean.shape == (105, 1) and var.shape == (105, 1)
    em = np.max(np.abs(mean[:, 0] - X.mean(axis=1)) / np.abs(X).max(axis=1))
    ev = np.max(np.abs(var[:, 0] / X.var(axis=1, ddof=1) - 1.0))
    print("posterior_moments(64) against the draws: mean %.3e, var %.3e" % (em, ev))
    assert em <= 1e-12 and ev <= 1e-12
    with pytest.raises(ValueError):
        m.posterior_moments(1)
    # the eigenbasis route's moments too
    y0, _ = problem(ms, 0)
    m0 = grid_model(gg, ms, y0.reshape(-1, 1), solver='exact')
    X = m0.sample_posterior(8, seed=2)
    mean, var = m0.posterior_moments(8, seed=2)
    assert np.max(np.abs(mean[:, 0] - X.mean(axis=1)) / np.abs(X).max(axis=1)) <= 1e-12
    assert np.max(np.abs(var[:, 0] / X.var(axis=1, ddof=1) - 1.0)) <= 1e-12


# ------------------------------------------------------------ statistics
def test_statistics_masked(gg):
    """256 device draws against the dense posterior: 6 sigma bounds of the
    exact Gaussian law (the eigenvector signs are the device's own, so the
    values are not pinned)."""
    ms, S = (7, 5, 3), 256
    y, mask = problem(ms, 0.2)
    m = grid_model(gg, ms, y.reshape(-1, 1), mask=mask)
    D = restatement(m, np.where(mask, y, 0.0), mask)
    X = m.sample_posterior(S, seed=0)
    sd = np.sqrt(np.diag(D.Sigma))
    zmean = np.max(np.abs(X.mean(axis=1) - D.mu) / (sd / np.sqrt(S)))
    vr = X.var(axis=1, ddof=1) / sd ** 2
    print("masked statistics: mean z %.2f, var ratio in [%.3f, %.3f] (bound +-%.3f)"
          % (zmean, vr.min(), vr.max(), 6 * np.sqrt(2.0 / (S - 1))))
    assert zmean <= 6
    assert np.max(np.abs(vr - 1.0)) <= 6 * np.sqrt(2.0 / (S - 1))


def test_statistics_complete_against_predict_grid(gg):
    ms, S = (7, 5, 3), 256
    y, _ = problem(ms, 0)
    m = grid_model(gg, ms, y.reshape(-1, 1), solver='exact')
    mu, pv = m.predict_grid()
    lat = pv[:, 0] - S2
    mean, var = m.posterior_moments(S, seed=0)
    zmean = np.max(np.abs(mean[:, 0] - mu[:, 0]) / np.sqrt(lat / S))
    vr = var[:, 0] / lat
    print("complete statistics: mean z %.2f, var ratio in [%.3f, %.3f]"
          % (zmean, vr.min(), vr.max()))
    assert zmean <= 6
    assert np.max(np.abs(vr - 1.0)) <= 6 * np.sqrt(2.0 / (S - 1))
