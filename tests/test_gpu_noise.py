"""Per-point noise on the MI355X: the weighted masked CG (gg_cgm_set_noise,
linalg.cg(noise=), MaskedKronCG(noise=)), the weighted masked Lanczos / SLQ
(gg_lanczos_probe_masked_noise), the weighted sampling residual
(gg_sample_residual_noise) and GPGridModel(noise_scale=) against dense
K_oo + D_oo algebra and the NumPy restatement in noise_ref.py (itself checked
against dense algebra on the CPU, test_noise_ref.py).

Shapes and masks as the masked CG tests; noise_var = 0.01 and noise_scale two
decades wide (noise_ref.noise_scale).  (7, 5, 3): N = 105 is odd (the scalar
lanes and the odd tails); frac 0 is the complete grid, solved without mask=.
Tolerances are those of the scalar masked path (test_gpu_masked.py,
test_gpu_masked_lanczos.py): converged solve 1e-8, unconverged Krylov steps
1e-3, iteration counts 5 %, chunking 1e-12, the first 12 alphas at 1e-8 and
betas at 1e-7, per-probe SLQ estimates 1e-5 |log det|; probe traces 10 rtol
cond(A) sum|terms| (test_gpu_grid_grad.py); the sampled mean within 6 sigma of
the dense posterior's law (test_gpu_posterior_sample.py).
"""
import ctypes

import numpy as np
import pytest

import masked_ref as mr
import noise_ref as nr

pytestmark = pytest.mark.gpu

S2 = nr.NOISE_VAR
RTOL = 1e-11


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def mask_arg(C, frac):
    return C["mask"] if frac > 0 else None


_ref = {}


def ref_cg(ms, frac, precond=None):
    """noise_ref.weighted_cg to RTOL: (x, info, iters), once per case."""
    key = (tuple(ms), frac, precond)
    if key not in _ref:
        C = nr.case(ms, frac)
        _ref[key] = nr.weighted_cg(C["F"], C["y"], C["mask"], C["noise"], rtol=RTOL,
                                   precond=precond)
    return _ref[key]


# ------------------------------------------------------------ converged solve
@pytest.mark.parametrize("ms,frac", nr.CG_CASES)
def test_weighted_cg_converged(gg, ms, frac):
    C = nr.case(ms, frac)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    y, mask = C["y"], C["mask"]
    x, info = gg.linalg.cg(K, y.reshape(-1, 1), rtol=RTOL, mask=mask_arg(C, frac),
                           noise=C["noise"])
    it = gg.linalg.cg.last.iters
    _, _, itref = ref_cg(ms, frac)
    print("weighted CG", ms, frac, "iters", it, "noise_ref", itref, "err", rel(x, C["x"]))
    assert info == 0
    assert x.shape == (y.size, 1)
    assert rel(x, C["x"]) < 1e-8
    assert np.all(x[~mask, 0] == 0)
    assert abs(it - itref) <= 0.05 * itref, (it, itref)
    if frac > 0:
        # b and the noise at the missing points are never used: NaN changes nothing
        x2, info2 = gg.linalg.cg(K, np.where(mask, y, np.nan).reshape(-1, 1), rtol=RTOL,
                                 mask=mask, noise=np.where(mask, C["noise"], np.nan))
        assert info2 == 0 and gg.linalg.cg.last.iters == it
        assert np.array_equal(x2, x)


def test_weighted_cg_device_inputs(gg):
    """b, the mask and the noise as device tensors; the noise, then b, one
    double into an allocation (N = 105 is odd): the scalar kernels."""
    import torch
    C = nr.case((7, 5, 3), 0.2)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    yd = torch.from_numpy(C["y"].copy()).cuda()
    md = torch.from_numpy(C["mask"].copy()).cuda()
    nd = torch.from_numpy(C["noise"].copy()).cuda()
    x, info = gg.linalg.cg(K, yd, rtol=RTOL, mask=md, noise=nd)
    assert info == 0 and x.is_cuda and x.shape == (105,)
    assert rel(host(x), C["x"]) < 1e-8
    nbuf = torch.zeros(106, dtype=torch.float64, device="cuda")
    nbuf[1:] = nd
    assert nbuf[1:].data_ptr() % 16 == 8
    x2, info = gg.linalg.cg(K, yd, rtol=RTOL, mask=md, noise=nbuf[1:])
    assert info == 0 and rel(host(x2), C["x"]) < 1e-8
    buf = torch.zeros(106, dtype=torch.float64, device="cuda")
    buf[1:] = yd
    x3, info = gg.linalg.cg(K, buf[1:], rtol=RTOL, mask=md.to(torch.uint8), noise=nbuf[1:])
    assert info == 0 and rel(host(x3), C["x"]) < 1e-8


def test_unaligned_noise_on_an_even_grid(gg):
    """An even N with the noise one double into an allocation: the scalar
    variant against the 16-byte one."""
    import torch
    C = nr.case((12, 10, 8), 0.3)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    x, info = gg.linalg.cg(K, C["y"], rtol=RTOL, mask=C["mask"], noise=C["noise"])
    nbuf = torch.zeros(961, dtype=torch.float64, device="cuda")
    nbuf[1:] = torch.from_numpy(C["noise"].copy()).cuda()
    x2, info2 = gg.linalg.cg(K, C["y"], rtol=RTOL, mask=C["mask"], noise=nbuf[1:])
    assert info == 0 and info2 == 0
    assert rel(x, C["x"]) < 1e-8 and rel(x2, C["x"]) < 1e-8


# ------------------------------------------------------------ fixed iterations
def test_weighted_cg_fixed_iterations_match_noise_ref(gg):
    C = nr.case((12, 10, 8), 0.1)
    F, mask, y, noise = C["F"], C["mask"], C["y"], C["noise"]
    K = gg.tensors.KronMatrix(F, sym=True)
    x, info = gg.linalg.cg(K, y, rtol=1e-30, maxiter=30, mask=mask, noise=noise)
    assert info == 30 and gg.linalg.cg.last.iters == 30
    xo, _, _ = nr.weighted_cg(F, y, mask, noise, rtol=1e-30, maxiter=30)
    rn = np.linalg.norm(np.where(mask, y, 0.0) - nr.weighted_op(F, mask, noise)(xo))
    print("fixed 30: x err", rel(x, xo), "resid", gg.linalg.cg.last.resid, "noise_ref", rn)
    assert rel(x, xo) < 1e-3
    assert abs(gg.linalg.cg.last.resid - rn) <= 1e-3 * rn
    assert np.all(x[~mask] == 0)


@pytest.mark.parametrize("precond", [None, 'kron'])
def test_weighted_cg_chunking(gg, precond):
    import torch
    C = nr.case((12, 10, 8), 0.1)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    yd = torch.from_numpy(C["y"].copy()).cuda()
    a = gg.linalg.MaskedKronCG(K, 0.0, C["mask"], precond=precond, noise=C["noise"])
    a.start(yd, rtol=1e-30)
    for _ in range(3):
        a.iterate(10)
    b = gg.linalg.MaskedKronCG(K, None, C["mask"], precond=precond, noise=C["noise"])
    b.start(yd, rtol=1e-30)
    b.iterate(30, check_every=7)
    sa, sb = a.status(), b.status()
    assert sa[0] == 30 and sb[0] == 30 and not sa[1]
    assert rel(host(a.x), host(b.x)) < 1e-12
    assert abs(sa[2] - sb[2]) <= 1e-12 * sb[2]
    assert a.n_observed == int(C["mask"].sum())
    # the preconditioner's stand-in defaults to the geometric mean
    g = nr.geometric_mean(C["mask"], C["noise"])
    assert abs(a.shift - g) <= 1e-12 * g and abs(b.shift - g) <= 1e-12 * g


# ------------------------------------------------------------ scalar equivalence
def test_constant_noise_against_the_scalar_masked_solve(gg):
    """noise = s everywhere is the scalar system; the arithmetic differs (p.K p
    + s sum p^2 against the shifted epilogue), so no bitwise equality."""
    C = nr.case((12, 10, 8), 0.1)
    F, mask, y = C["F"], C["mask"], C["y"]
    K = gg.tensors.KronMatrix(F, sym=True)
    ex = mr.dense_solve(F, y, mask, S2)
    xs, infos = gg.linalg.cg(K, y, shift=S2, rtol=RTOL, mask=mask)
    its = gg.linalg.cg.last.iters
    xn, infon = gg.linalg.cg(K, y, rtol=RTOL, mask=mask, noise=np.full(960, S2))
    itn = gg.linalg.cg.last.iters
    print("constant noise: iters", itn, "scalar", its, "err", rel(xn, ex), rel(xs, ex))
    assert infos == 0 and infon == 0
    assert rel(xs, ex) < 1e-8 and rel(xn, ex) < 1e-8
    assert abs(itn - its) <= 0.05 * its, (itn, its)


# ------------------------------------------------------------ preconditioner
@pytest.mark.parametrize("frac", [0.1, 0.3])
def test_kron_preconditioner(gg, frac):
    ms = (12, 10, 8)
    C = nr.case(ms, frac)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    x, info = gg.linalg.cg(K, C["y"], rtol=RTOL, mask=C["mask"], noise=C["noise"])
    it = gg.linalg.cg.last.iters
    xp, infop = gg.linalg.cg(K, C["y"], rtol=RTOL, mask=C["mask"], noise=C["noise"],
                             precond='kron')
    itp = gg.linalg.cg.last.iters
    _, inforef, itref = ref_cg(ms, frac, 'kron')
    print("weighted PCG", frac, "iters", itp, "noise_ref", itref, "unpreconditioned", it,
          "err", rel(xp, C["x"]))
    assert info == 0 and infop == 0 and inforef == 0
    assert rel(xp, C["x"]) < 1e-8 and rel(xp, x) < 1e-8
    assert np.all(xp[~C["mask"]] == 0)
    assert abs(itp - itref) <= 0.05 * itref, (itp, itref)


# ------------------------------------------------------------ tridiagonal, SLQ
def check_tridiag(a, b, ao, bo):
    k = min(a.size, ao.size, 12)
    assert k >= 2
    np.testing.assert_allclose(a[:k], ao[:k], rtol=1e-8)
    np.testing.assert_allclose(b[:k - 1], bo[:k - 1], rtol=1e-7)


LZ_CASES = [((7, 5, 3), 0.2), ((16, 12), 0.3), ((12, 10, 8), 0.3), ((12, 10, 8), 0.1),
            ((16, 16, 8), 0.6), ((8, 6, 5, 4), 0.3), ((9, 8, 7), 0.0)]


@pytest.mark.parametrize("ms,frac", LZ_CASES)
def test_weighted_tridiag_vs_numpy(gg, ms, frac):
    import torch
    n = int(np.prod(ms))
    F = mr.rbf_factors(ms)
    mask = nr.make_mask(n, frac)
    noise = S2 * nr.noise_scale(n)
    K = gg.tensors.KronMatrix(F, sym=True)
    a, b = gg.linalg.lanczos_tridiag(K, 0.0, 20, seed=7, probe=2, noise=noise,
                                     mask=mask if frac > 0 else None)
    ao, bo = nr.weighted_lanczos(F, mask, noise, 7, 2, 20)
    k = min(a.size, ao.size, 12)
    print("weighted Lanczos", ms, frac, "alpha", np.max(np.abs(a[:k] / ao[:k] - 1)),
          "beta", np.max(np.abs(b[:k - 1] / bo[:k - 1] - 1)))
    assert a.size == 20 and b.size == 19
    check_tridiag(a, b, ao, bo)
    assert gg.linalg.lanczos_tridiag.n_observed == int(mask.sum())
    # NaN at the missing points, and the noise one double into an allocation
    # (the scalar lanes), on the device
    nbuf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    nbuf[1:] = torch.from_numpy(np.where(mask, noise, np.nan)).cuda()
    a2, b2 = gg.linalg.lanczos_tridiag(K, 0.0, 20, seed=7, probe=2, noise=nbuf[1:],
                                       mask=torch.from_numpy(mask.copy()).cuda())
    check_tridiag(a2, b2, ao, bo)


@pytest.mark.parametrize("frac", [0.1, 0.3])
def test_weighted_slq_vs_numpy_and_dense(gg, frac):
    C = nr.case((12, 10, 8), frac)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    mean, ests = gg.linalg.slq_logdet(K, 0.0, probes=8, steps=40, seed=3, mask=C["mask"],
                                      noise=C["noise"])
    mo, eo = nr.weighted_slq(C["F"], C["mask"], C["noise"], probes=8, steps=40, seed=3)
    ld = nr.dense_logdet(C["F"], C["mask"], C["noise"], C["A"])
    print("weighted SLQ", frac, "mean", mean, "numpy", mo, "dense", ld, "per-probe",
          np.max(np.abs(ests - eo)) / abs(ld))
    assert ests.shape == (8,)
    assert np.max(np.abs(ests - eo)) <= 1e-5 * abs(ld)


# ------------------------------------------------------------ model
MS = (12, 10, 8)


def grid_model(gg, ms, y, scale, mask=None, **kw):
    """GPGridModel whose operator has masked_ref.rbf_factors(ms) (cov_grid
    reverses the input dimensions: input j is factor d - 1 - j)."""
    d = len(ms)
    ls = [0.1 * (1 + 0.05 * i) for i in range(d)]
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=ls[d - 1 - j]) for j in range(d)]
    xg = [np.linspace(0, 1, ms[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    kw.setdefault("cg_rtol", RTOL)
    kw.setdefault("logdet", "lanczos")
    return gg.models.GPGridModel(xg, np.asarray(y).reshape(-1, 1), gg.kern.GridKernel(kerns),
                                 noise_var=S2, mask=mask, noise_scale=scale, **kw)


@pytest.fixture(scope="module")
def dense_model():
    """Dense posterior algebra at (12, 10, 8), 10 % missing, 5 off-grid rows."""
    import oracle
    C = nr.case(MS, 0.1)
    F, mask, y, ex = C["F"], C["mask"], C["y"], C["x"]
    d = len(MS)
    K = mr.dense_K(F)
    Aoo, o = C["A"]
    Xnew = np.random.default_rng(2).uniform(0.0, 1.0, (5, d))
    ks = np.empty((5, K.shape[0]))
    for r in range(5):
        row = np.ones(1)
        for i in range(d):   # factor i is input dimension d - 1 - i
            g = np.linspace(0, 1, MS[i])
            row = np.kron(row, oracle.cov_1d("RBF", Xnew[r:r + 1, d - 1 - i], g, 1.0,
                                             0.1 * (1 + 0.05 * i)).reshape(-1))
        ks[r] = row
    mean = ks.dot(ex)
    var = 1.0 - np.einsum("ro,ro->r", ks[:, o], np.linalg.solve(Aoo, ks[:, o].T).T) + S2
    lam = np.linalg.eigvalsh(Aoo)
    return dict(C=C, grid_mean=K.dot(ex), Xnew=Xnew, mean=mean, var=var,
                cond=float(lam[-1] / lam[0]))


@pytest.mark.parametrize("precond", [None, 'kron'])
def test_model_posterior(gg, dense_model, precond):
    D, C = dense_model, dense_model["C"]
    mask = C["mask"]
    # Y and noise_scale at the missing points are ignored
    m = grid_model(gg, MS, np.where(mask, C["y"], np.nan), np.where(mask, C["scale"], np.nan),
                   mask=mask, precond=precond)
    assert m.solver == 'cg'
    m.fit()
    alpha = host(m._alpha)
    assert rel(alpha, C["x"]) < 1e-8
    assert np.all(alpha[~mask] == 0)
    mean, var = m.predict_grid(compute_var=False)
    assert var is None and mean.shape == (960, 1)
    assert rel(mean, D["grid_mean"]) < 1e-8
    pm, pv = m.predict(D["Xnew"])
    assert pm.shape == (5, 1) and pv.shape == (5, 1)
    print("predict mean", rel(pm, D["mean"]), "var", rel(pv, D["var"]))
    assert rel(pm, D["mean"]) < 1e-8
    assert rel(pv, D["var"]) < 1e-8


def test_model_without_a_mask(gg):
    C = nr.case((7, 5, 3), 0.0)
    m = grid_model(gg, (7, 5, 3), C["y"], C["scale"])
    m.fit()
    assert m.num_observed == 105
    assert rel(host(m._alpha), C["x"]) < 1e-8


def test_model_lml_and_gradient_estimates(gg, dense_model):
    D, C = dense_model, dense_model["C"]
    F, mask, noise = C["F"], C["mask"], C["noise"]
    m = grid_model(gg, MS, C["y"], C["scale"], mask=mask, slq_probes=8, slq_steps=40, seed=3,
                   grad_method='adjoint', grad_probes=6)
    ll, g = m._adjoint_gradient(m.parameters)
    lml = float(np.squeeze(ll))
    mean, ests = nr.weighted_slq(F, mask, noise, probes=8, steps=40, seed=3)
    ref = nr.lml(C["y"], C["x"], mean, mask)
    ld = nr.dense_logdet(F, mask, noise, C["A"])
    print("LML", lml, "noise_ref (same probes)", ref, "dense", nr.lml(C["y"], C["x"], ld, mask))
    assert m.slq_estimates.shape == (8,)
    assert np.max(np.abs(m.slq_estimates - ests)) <= 1e-5 * abs(ld)
    # the data-fit term to the solve's 1e-8, the log det to the per-probe 1e-5
    fit = abs(float(C["y"][mask].dot(C["x"][mask])))
    assert abs(lml - ref) <= 0.5 * (1e-8 * fit + 1e-5 * abs(ld))
    tr, absref = nr.noise_trace_estimates(F, mask, noise, C["scale"], 6, 3, C["A"])
    tol = 10 * RTOL * D["cond"] * absref
    err = np.abs(m.grad_estimates[:, 0] - tr)
    print("noise trace per probe: err / tol", err / tol)
    assert m.grad_estimates.shape == (6, 1 + 6)
    assert np.all(err <= tol)
    # the noise entry: 1/2 alpha^T (scale o alpha) - 1/2 mean of the probe traces
    want = 0.5 * float(np.sum(C["scale"][mask] * C["x"][mask] ** 2)) - 0.5 * tr.mean()
    fit0 = 0.5 * float(np.sum(C["scale"][mask] * C["x"][mask] ** 2))
    assert np.all(np.isfinite(g))
    assert abs(g[0] - want) <= 10 * RTOL * D["cond"] * (fit0 + 0.5 * absref.mean())


def test_trace_grad_unit_vectors_give_the_dense_traces(gg):
    """Z = the unit vectors of the observed points: column 0 sums to
    tr(A^-1 diag(scale)), the column of dK = K to tr(A^-1 K_oo); 10 rtol
    cond(A) sum|terms|."""
    rtol = 1e-12
    C = nr.case((7, 5, 3), 0.2)
    Aoo, o = C["A"]
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    Z = np.zeros((105, o.size))
    Z[o, np.arange(o.size)] = 1.0
    means, per = gg.linalg.trace_grad(K, [K], 0.0, mask=C["mask"], rtol=rtol, Z=Z,
                                      noise=C["noise"], noise_scale=C["scale"])
    Ai = np.linalg.inv(Aoo)
    Koo = mr.dense_K(C["F"])[np.ix_(o, o)]
    want = np.array([np.sum(np.diag(Ai) * C["scale"][o]), np.sum(Ai * Koo)])
    absref = np.array([np.sum(np.abs(np.diag(Ai)) * C["scale"][o]), np.sum(np.abs(Ai * Koo))])
    lam = np.linalg.eigvalsh(Aoo)
    tol = 10 * rtol * (lam[-1] / lam[0]) * absref
    err = np.abs(per.sum(axis=0) - want)
    print("unit vectors: err / tol", err / tol)
    assert per.shape == (o.size, 2)
    assert np.all(err <= tol)


def test_model_optimize(gg, dense_model):
    C = dense_model["C"]
    m = grid_model(gg, MS, C["y"], C["scale"], mask=C["mask"], slq_probes=8, slq_steps=30,
                   seed=3, cg_rtol=1e-10)
    before = float(np.squeeze(m.log_likelihood()))
    m.optimize(max_iters=3)
    after = float(np.squeeze(m.log_likelihood()))
    print("optimize: LML", before, "->", after)
    assert np.isfinite(after) and after >= before


# ------------------------------------------------------------ sampling
def test_sample_residual_noise_kernel(gg):
    """b = select(mask, y - f - sqrt(noise) z, 0) with z of gg_normal_fill's
    stream, at an odd n, aligned and one double in; NaN off the mask."""
    import torch
    from gp_grief_amd import native
    L = native.lib()
    n = 105
    C = nr.case((7, 5, 3), 0.2)
    mask, noise = C["mask"], C["noise"]
    rng = np.random.default_rng(5)
    y, f = rng.standard_normal(n), rng.standard_normal(n)
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    native.check(L.gg_normal_fill(9, 5, native.dptr(z), n, native.stream_ptr()))
    want = np.where(mask, y - f - np.sqrt(noise) * host(z), 0.0)
    md = torch.from_numpy(mask.copy()).cuda().to(torch.uint8)
    for off in (0, 1):
        bufs = []
        for v in (np.where(mask, y, np.nan), f, np.where(mask, noise, np.nan)):
            t = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
            t[off:off + n] = torch.from_numpy(v).cuda()
            bufs.append(t[off:off + n])
        out = torch.full((n + 1,), 777.0, dtype=torch.float64, device="cuda")
        b = out[off:off + n]
        native.check(L.gg_sample_residual_noise(
            native.dptr(bufs[0]), native.dptr(bufs[1]), native.dptr(bufs[2]),
            ctypes.c_void_p(md.data_ptr()), 9, 5, native.dptr(b), n, native.stream_ptr()))
        got = host(b)
        # one product and two differences of O(1) numbers: a few ulps of |y| + |f| + |sd z|
        bound = 4 * np.finfo(np.float64).eps * (np.abs(y) + np.abs(f)
                                                + np.sqrt(noise) * np.abs(host(z)))
        assert np.all(got[~mask] == 0)
        assert np.all(np.abs(got - want)[mask] <= bound[mask])
        assert float(out[n if off == 0 else 0]) == 777.0
    # no mask: every point
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    yd, fd, nd = (torch.from_numpy(v.copy()).cuda() for v in (y, f, noise))
    native.check(L.gg_sample_residual_noise(native.dptr(yd), native.dptr(fd), native.dptr(nd),
                                            None, 9, 5, native.dptr(out), n,
                                            native.stream_ptr()))
    full = y - f - np.sqrt(noise) * host(z)
    assert np.all(np.abs(host(out) - full) <= 4 * np.finfo(np.float64).eps
                  * (np.abs(y) + np.abs(f) + np.sqrt(noise) * np.abs(host(z))))


def test_draws_and_their_mean(gg):
    """Draw k is the same whatever n_samples; the mean of 64 draws against the
    dense posterior N(mu, Sigma), mu = K_:o A^-1 y_o, Sigma = K - K_:o A^-1 K_o:
    -- each grid point's sample mean is Gaussian with sd sqrt(Sigma_ii / 64),
    held to 6 of them as test_statistics_masked."""
    ms, S = (7, 5, 3), 64
    C = nr.case(ms, 0.2)
    mask = C["mask"]
    m = grid_model(gg, ms, np.where(mask, C["y"], np.nan), C["scale"], mask=mask)
    X = m.sample_posterior(S, seed=2)
    assert X.shape == (105, S) and np.all(np.isfinite(X))
    assert np.array_equal(m.sample_posterior(3, seed=2), X[:, :3])
    assert np.array_equal(m.sample_posterior(1, seed=2), X[:, :1])
    assert rel(m.sample_posterior(1, seed=4)[:, 0], X[:, 0]) > 0.01
    smp = m._sampler(2)
    assert smp.route == 'matheron' and smp._cg is m._masked_cg() and smp.noise is not None
    K = mr.dense_K(C["F"])
    Aoo, o = C["A"]
    Ko = K[:, o]
    mu = Ko.dot(C["x"][o])
    Sigma = K - Ko.dot(np.linalg.solve(Aoo, Ko.T))
    sd = np.sqrt(np.diag(Sigma))
    zmean = np.max(np.abs(X.mean(axis=1) - mu) / (sd / np.sqrt(S)))
    print("mean of %d draws: worst z %.2f" % (S, zmean))
    assert zmean <= 6
    mean, var = m.posterior_moments(S, seed=2)
    assert np.max(np.abs(mean[:, 0] - X.mean(axis=1)) / np.abs(X).max(axis=1)) <= 1e-12
    assert np.max(np.abs(var[:, 0] / X.var(axis=1, ddof=1) - 1.0)) <= 1e-12
    # the variances see the noise draw's scale, which the mean does not: 256
    # streamed draws, (S - 1) s^2 / Sigma_ii is chi-square with S - 1 degrees, sd
    # of the ratio sqrt(2 / (S - 1)), held to 6 of them as test_statistics_masked
    S2_ = 256
    mean, var = m.posterior_moments(S2_, seed=0)
    zmean = np.max(np.abs(mean[:, 0] - mu) / (sd / np.sqrt(S2_)))
    vr = var[:, 0] / sd ** 2
    print("256 draws: mean z %.2f, var ratio in [%.3f, %.3f] (bound +-%.3f)"
          % (zmean, vr.min(), vr.max(), 6 * np.sqrt(2.0 / (S2_ - 1))))
    assert zmean <= 6
    assert np.max(np.abs(vr - 1.0)) <= 6 * np.sqrt(2.0 / (S2_ - 1))


# ------------------------------------------------------------ errors
def test_noise_value_errors(gg):
    C = nr.case((7, 5, 3), 0.2)
    mask, noise, y = C["mask"], C["noise"], C["y"]
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    cg = gg.linalg.cg
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask, noise=noise)               # two diagonals
    with pytest.raises(ValueError):
        gg.linalg.MaskedKronCG(K, S2, mask, noise=noise)         # the same, resident
    with pytest.raises(ValueError):
        gg.linalg.MaskedKronCG(K, S2, mask, precond_shift=S2)    # a stand-in without noise
    with pytest.raises(ValueError):
        gg.linalg.MaskedKronCG(K, None, mask, noise=noise, precond_shift=0.0)
    with pytest.raises(ValueError):
        gg.linalg.trace_grad(K, [], S2, mask=mask, noise=noise, noise_scale=C["scale"])
    x, info = cg(K, y, shift=None, mask=mask, noise=noise, rtol=RTOL)   # None is "omitted"
    assert info == 0 and rel(x, C["x"]) < 1e-8
    with pytest.raises(ValueError):
        cg(K, y, noise=noise, comm=True)
    with pytest.raises(ValueError):
        cg(K, y, noise=noise, basis='block')
    with pytest.raises(ValueError):
        cg(K, y, noise=noise, recurrence='fused')
    with pytest.raises(ValueError):
        cg(K, y, noise=noise, fusion=0)
    with pytest.raises(ValueError):
        cg(K, y, mask=mask, noise=noise, precond='jacobi')
    with pytest.raises(ValueError):
        cg(K, y, mask=mask, noise=noise[:-1])                    # wrong length
    bad = noise.copy()
    bad[np.nonzero(mask)[0][3]] = 0.0
    with pytest.raises(ValueError, match="positive"):
        cg(K, y, mask=mask, noise=bad)                           # not positive where observed
    bad[np.nonzero(mask)[0][3]] = np.nan
    with pytest.raises(ValueError, match="positive"):
        cg(K, y, mask=mask, noise=bad)
    with pytest.raises(ValueError):
        gg.linalg.lanczos_tridiag(K, S2, 5, mask=mask, noise=noise)
    with pytest.raises(ValueError):
        gg.linalg.slq_logdet(K, 0.0, mask=mask, noise=noise[:-1])
    with pytest.raises(ValueError):
        gg.linalg.trace_grad(K, [], 0.0, mask=mask, noise=noise)  # noise_scale missing
    yd = gg.device.to_device(y)
    with pytest.raises(ValueError, match="cg"):
        gg.linalg.GridPosteriorSampler(K, 0.0, yd, mask=mask, noise=noise, solver='exact')
    with pytest.raises(ValueError, match="cg"):
        grid_model(gg, (7, 5, 3), y, C["scale"], mask=mask, solver='exact')
    for logdet in ('exact', 'scaled_eigs', 'slq'):
        with pytest.raises(ValueError, match="lanczos"):
            grid_model(gg, (7, 5, 3), y, C["scale"], mask=mask, logdet=logdet)
        with pytest.raises(ValueError, match="lanczos"):
            grid_model(gg, (7, 5, 3), y, C["scale"], logdet=logdet)
    with pytest.raises(ValueError):
        grid_model(gg, (7, 5, 3), y, C["scale"][:-1], mask=mask)
    m = grid_model(gg, (7, 5, 3), y, C["scale"], mask=mask)
    with pytest.raises(ValueError, match="posterior_moments"):
        m.predict_grid(compute_var=True)


def test_noise_abi_errors(gg):
    import torch
    from gp_grief_amd import native
    L = native.lib()
    sp = native.stream_ptr
    C = nr.case((7, 5, 3), 0.2)
    K = gg.tensors.KronMatrix(C["F"], sym=True)._device()
    md = torch.from_numpy(C["mask"].copy()).cuda().to(torch.uint8)
    mp = ctypes.c_void_p(md.data_ptr())
    nd = torch.from_numpy(C["noise"].copy()).cuda()
    yd = torch.from_numpy(C["y"].copy()).cuda()
    # ---- gg_cgm_set_noise
    assert L.gg_cgm_set_noise(None, native.dptr(nd)) == native.GG_ERR_VALUE
    we = ctypes.c_int64()
    native.check(L.gg_cgm_work_elems(K.h, ctypes.byref(we)))
    work = gg.device.empty(we.value)
    h = ctypes.c_void_p()
    native.check(L.gg_cgm_create(K.h, S2, mp, native.dptr(work), ctypes.byref(h)))
    try:
        assert L.gg_cgm_set_noise(h, ctypes.c_void_p(nd.data_ptr() + 4)) == native.GG_ERR_VALUE
        assert L.gg_cgm_set_noise(h, native.dptr(nd)) == native.GG_OK
        assert L.gg_cgm_set_noise(h, None) == native.GG_OK          # off again
        assert L.gg_cgm_set_noise(h, native.dptr(nd)) == native.GG_OK
        x = torch.full((105,), 777.0, dtype=torch.float64, device="cuda")
        native.check(L.gg_cgm_start(h, native.dptr(yd), native.dptr(x), RTOL, 0.0, sp()))
        # refused after start: the solve that follows is still the weighted one
        assert L.gg_cgm_set_noise(h, None) == native.GG_ERR_VALUE
        native.check(L.gg_cgm_iterate(h, 1000, 50, sp()))
        assert rel(host(x), C["x"]) < 1e-8
    finally:
        L.gg_cgm_destroy(h)
    # set and switched off again before start: the scalar system of the create-time shift
    h = ctypes.c_void_p()
    native.check(L.gg_cgm_create(K.h, S2, mp, native.dptr(work), ctypes.byref(h)))
    try:
        assert L.gg_cgm_set_noise(h, native.dptr(nd)) == native.GG_OK
        assert L.gg_cgm_set_noise(h, None) == native.GG_OK
        x = torch.full((105,), 777.0, dtype=torch.float64, device="cuda")
        native.check(L.gg_cgm_start(h, native.dptr(yd), native.dptr(x), RTOL, 0.0, sp()))
        native.check(L.gg_cgm_iterate(h, 1000, 50, sp()))
        assert rel(host(x), mr.dense_solve(C["F"], C["y"], C["mask"], S2)) < 1e-8
    finally:
        L.gg_cgm_destroy(h)
    # ---- gg_lanczos_probe_masked_noise
    lwork = gg.device.empty(4 * 105)
    a, b = (ctypes.c_double * 4)(*[777.0] * 4), (ctypes.c_double * 4)(*[777.0] * 4)
    done, nobs = ctypes.c_int(-5), ctypes.c_int64(-5)

    def call(kh, npx, mpx, steps, wp=native.dptr(lwork), ap=a, bp=b):
        return L.gg_lanczos_probe_masked_noise(kh, npx, mpx, 7, 2, steps, wp, ap, bp,
                                               ctypes.byref(done), ctypes.byref(nobs), sp())
    rng = np.random.default_rng(0)
    R = gg.tensors.KronMatrix([rng.standard_normal((3, 4)), rng.standard_normal((5, 2))])._device()
    zeros = torch.zeros(105, dtype=torch.uint8, device="cuda")
    for args in [(None, native.dptr(nd), mp, 4), (K.h, None, mp, 4), (K.h, native.dptr(nd), None, 4),
                 (K.h, native.dptr(nd), mp, 0), (R.h, native.dptr(nd), mp, 4),
                 (K.h, ctypes.c_void_p(nd.data_ptr() + 4), mp, 4),
                 (K.h, native.dptr(nd), mp, 4, None), (K.h, native.dptr(nd), mp, 4,
                                                        native.dptr(lwork), None),
                 (K.h, native.dptr(nd), mp, 4, native.dptr(lwork), a, None)]:
        assert call(*args) == native.GG_ERR_VALUE, args
    assert list(a) == [777.0] * 4 and list(b) == [777.0] * 4
    assert done.value == -5 and nobs.value == -5
    # an empty mask is found after the run: the count is reported, the arrays untouched
    assert call(K.h, native.dptr(nd), ctypes.c_void_p(zeros.data_ptr()), 4) == native.GG_ERR_VALUE
    assert list(a) == [777.0] * 4 and list(b) == [777.0] * 4
    assert done.value == -5 and nobs.value == 0
    assert call(K.h, native.dptr(nd), mp, 4) == native.GG_OK
    assert nobs.value == int(C["mask"].sum()) and done.value == 4
    ao, _ = nr.weighted_lanczos(C["F"], C["mask"], C["noise"], 7, 2, 4)
    np.testing.assert_allclose(np.array(a[:4]), ao, rtol=1e-8)
    # ---- gg_sample_residual_noise
    n = 105
    out = torch.full((n,), 777.0, dtype=torch.float64, device="cuda")
    vp, npt, op = native.dptr(yd), native.dptr(nd), native.dptr(out)
    for args in [(None, vp, npt, None, 1, 0, op, n), (vp, None, npt, None, 1, 0, op, n),
                 (vp, vp, None, None, 1, 0, op, n), (vp, vp, npt, None, 1, 0, None, n),
                 (vp, vp, npt, None, 1, 0, op, -1), (vp, vp, npt, None, 1, 65536, op, n),
                 (vp, vp, npt, None, 1, -1, op, n)]:
        assert L.gg_sample_residual_noise(*args, sp()) == native.GG_ERR_VALUE, args
    assert L.gg_sample_residual_noise(vp, vp, npt, None, 1, 0, op, 0, sp()) == native.GG_OK
    torch.cuda.synchronize()
    assert torch.all(out == 777.0)
