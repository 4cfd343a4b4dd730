"""The grid GP with missing observations on the MI355X: the masked device CG
(gg_cgm_*, linalg.cg(mask=...), linalg.MaskedKronCG) and GPGridModel(mask=...)
against dense K_oo algebra, oracle.cg_solve on the masked operator and the
NumPy restatement in masked_ref.py.

Shapes: RBF factors on linspace(0, 1, m), l_i = 0.1 (1 + 0.05 i), jitter 1e-12,
sigma^2 = 0.01; mask from default_rng(0).choice with the first and last grid
points forced missing.  (7, 5, 3): N = 105 is odd (unaligned tails);
(48, 6, 5): the folded-factor path; (50, 48, 40): many workgroups.
Tolerances are those of test_gpu_kron.py for the same kinds of comparison
(converged solve 1e-8, unconverged Krylov steps 1e-3, iteration counts 5 %,
log det 1e-9).
"""
import ctypes

import numpy as np
import pytest

import masked_ref as mr
import oracle

pytestmark = pytest.mark.gpu

S2 = 0.01


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


_cache = {}


def problem(ms, frac):
    """(factors, mask, y, dense exact solve): computed once per shape."""
    key = (tuple(ms), frac)
    if key not in _cache:
        F = mr.rbf_factors(ms)
        n = int(np.prod(ms))
        mask = mr.make_mask(n, frac)
        y = np.random.default_rng(1).standard_normal(n)
        ex = mr.dense_solve(F, y, mask, S2) if n <= 2000 else None
        # shared between the tests and left unchanged (y stays writable: torch
        # wraps it without a copy on its way to the device)
        for a in F + [mask] + ([ex] if ex is not None else []):
            a.setflags(write=False)
        _cache[key] = (F, mask, y, ex)
    return _cache[key]


def masked_op(F, mask):
    return lambda v: np.where(mask, oracle.kron_matvec(F, np.where(mask, v, 0.0)), 0.0) + S2 * v


# ------------------------------------------------------------ converged solve
@pytest.mark.parametrize("ms,frac", [((7, 5, 3), 0.2), ((12, 10, 8), 0.1), ((12, 10, 8), 0.3),
                                     ((48, 6, 5), 0.1)])
def test_masked_cg_converged(gg, ms, frac):
    F, mask, y, ex = problem(ms, frac)
    K = gg.tensors.KronMatrix(F, sym=True)
    x, info = gg.linalg.cg(K, y.reshape(-1, 1), shift=S2, rtol=1e-11, mask=mask)
    it = gg.linalg.cg.last.iters
    _, _, ito = oracle.cg_solve(masked_op(F, mask), np.where(mask, y, 0.0), rtol=1e-11)
    print("masked CG", ms, frac, "iters", it, "oracle", ito, "err", rel(x, ex))
    assert info == 0
    assert x.shape == (y.size, 1)
    assert rel(x, ex) < 1e-8
    assert np.all(x[~mask, 0] == 0)
    assert abs(it - ito) <= 0.05 * ito, (it, ito)
    # Y at the missing points is never read: NaN there changes nothing
    ynan = np.where(mask, y, np.nan)
    x2, info2 = gg.linalg.cg(K, ynan.reshape(-1, 1), shift=S2, rtol=1e-11, mask=mask)
    assert info2 == 0 and gg.linalg.cg.last.iters == it
    assert np.array_equal(x2, x)


def test_masked_cg_device_inputs(gg):
    """b and the mask as device tensors; x comes back on the device."""
    import torch
    F, mask, y, ex = problem((7, 5, 3), 0.2)
    K = gg.tensors.KronMatrix(F, sym=True)
    yd = torch.from_numpy(y.copy()).cuda()
    md = torch.from_numpy(mask.copy()).cuda()
    x, info = gg.linalg.cg(K, yd, shift=S2, rtol=1e-11, mask=md)
    assert info == 0 and x.is_cuda and x.shape == (105,)
    assert rel(x.cpu().numpy(), ex) < 1e-8
    # an unaligned b (a view one double into an allocation): the scalar kernels
    buf = torch.zeros(106, dtype=torch.float64, device="cuda")
    buf[1:] = yd
    x2, info = gg.linalg.cg(K, buf[1:], shift=S2, rtol=1e-11, mask=md.to(torch.uint8))
    assert info == 0 and rel(x2.cpu().numpy(), ex) < 1e-8


# ------------------------------------------------------------ fixed iterations
def test_masked_cg_fixed_iterations_match_oracle(gg):
    """30 unconverged steps on N = 96 000 (many workgroups) track the oracle to
    rounding growth, as test_cg_fixed_iterations_match_oracle."""
    F, mask, y, _ = problem((50, 48, 40), 0.25)
    K = gg.tensors.KronMatrix(F, sym=True)
    x, info = gg.linalg.cg(K, y, shift=S2, rtol=1e-30, maxiter=30, mask=mask)
    assert info == 30 and gg.linalg.cg.last.iters == 30
    A = masked_op(F, mask)
    b = np.where(mask, y, 0.0)
    xo, _, _ = oracle.cg_solve(A, b, rtol=1e-30, maxiter=30)
    rn = np.linalg.norm(b - A(xo))
    print("fixed 30: x err", rel(x, xo), "resid", gg.linalg.cg.last.resid, "oracle", rn)
    assert rel(x, xo) < 1e-3
    assert abs(gg.linalg.cg.last.resid - rn) <= 1e-3 * rn
    assert np.all(x[~mask] == 0)


# ------------------------------------------------------------ unmasked equivalence
def test_all_ones_mask_is_the_textbook_cg(gg):
    F, _, y, _ = problem((12, 10, 8), 0.1)
    K = gg.tensors.KronMatrix(F, sym=True)
    xm, info = gg.linalg.cg(K, y, shift=S2, rtol=1e-30, maxiter=20, mask=np.ones(960, bool))
    assert info == 20
    rm = gg.linalg.cg.last.resid
    xt, info = gg.linalg.cg(K, y, shift=S2, rtol=1e-30, maxiter=20, recurrence="textbook",
                            basis="grid")
    assert info == 20
    print("all-ones vs textbook", rel(xm, xt))
    assert rel(xm, xt) < 1e-12
    assert abs(rm - gg.linalg.cg.last.resid) <= 1e-12 * rm


# ------------------------------------------------------------ preconditioner
def test_kron_preconditioner(gg):
    F, mask, y, ex = problem((12, 10, 8), 0.1)
    K = gg.tensors.KronMatrix(F, sym=True)
    x, info = gg.linalg.cg(K, y, shift=S2, rtol=1e-11, mask=mask)
    it = gg.linalg.cg.last.iters
    xp, infop = gg.linalg.cg(K, y, shift=S2, rtol=1e-11, mask=mask, precond='kron')
    itp = gg.linalg.cg.last.iters
    _, inforef, itref = mr.masked_cg(F, y, mask, S2, rtol=1e-11, precond='kron')
    print("PCG iters", itp, "ref", itref, "CG iters", it, "err", rel(xp, ex))
    assert info == 0 and infop == 0 and inforef == 0
    assert rel(xp, ex) < 1e-8 and rel(xp, x) < 1e-8
    assert np.all(xp[~mask] == 0)
    assert abs(itp - itref) <= 0.05 * itref, (itp, itref)
    assert itp < it


# ------------------------------------------------------------ resident solver
@pytest.mark.parametrize("precond", [None, 'kron'])
def test_masked_kron_cg_chunking(gg, precond):
    import torch
    F, mask, y, _ = problem((12, 10, 8), 0.1)
    K = gg.tensors.KronMatrix(F, sym=True)
    yd = torch.from_numpy(y.copy()).cuda()
    a = gg.linalg.MaskedKronCG(K, S2, mask, precond=precond)
    a.start(yd, rtol=1e-30)
    for _ in range(3):
        a.iterate(10)
    b = gg.linalg.MaskedKronCG(K, S2, mask, precond=precond)
    b.start(yd, rtol=1e-30)
    b.iterate(30, check_every=7)
    sa, sb = a.status(), b.status()
    assert sa[0] == 30 and sb[0] == 30 and not sa[1]
    # the same launch sequence whatever the chunking: the same bits
    # (test_gpu_masked_abi.py pins it for the C ABI)
    assert np.array_equal(a.x.cpu().numpy(), b.x.cpu().numpy())
    assert sa[2] == sb[2]
    assert a.n_observed == int(mask.sum())


# ------------------------------------------------------------ model
MS = (12, 10, 8)


def _grid_model(gg, y, mask, **kw):
    """GPGridModel whose operator has masked_ref.rbf_factors(MS) (cov_grid
    reverses the input dimensions: input j is factor d - 1 - j)."""
    d = len(MS)
    ls = [0.1 * (1 + 0.05 * i) for i in range(d)]
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=ls[d - 1 - j]) for j in range(d)]
    xg = [np.linspace(0, 1, MS[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    gk = gg.kern.GridKernel(kerns)
    kw.setdefault("cg_rtol", 1e-11)
    return gg.models.GPGridModel(xg, y.reshape(-1, 1), gk, noise_var=S2, solver='cg', mask=mask,
                                 **kw)


@pytest.fixture(scope="module")
def dense_model():
    """Dense posterior algebra at (12, 10, 8), 10 % missing, 5 off-grid rows."""
    F, mask, y, ex = problem(MS, 0.1)
    d = len(MS)
    K = mr.dense_K(F)
    o = np.nonzero(mask)[0]
    Koo = K[np.ix_(o, o)] + S2 * np.eye(o.size)
    ld = float(np.linalg.slogdet(Koo)[1])
    lml = -0.5 * (float(y[o].dot(ex[o])) + ld + o.size * np.log(2 * np.pi))
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
    var = 1.0 - np.einsum("ro,ro->r", ks[:, o], np.linalg.solve(Koo, ks[:, o].T).T) + S2
    return dict(F=F, mask=mask, y=y, alpha=ex, grid_mean=K.dot(ex), ld=ld, lml=lml, Xnew=Xnew,
                mean=mean, var=var)


def test_model_posterior(gg, dense_model):
    D = dense_model
    ynan = np.where(D["mask"], D["y"], np.nan)   # Y at the missing points is ignored
    m = _grid_model(gg, ynan, D["mask"])
    m.fit()
    alpha = m._alpha.cpu().numpy()
    assert rel(alpha, D["alpha"]) < 1e-8
    assert np.all(alpha[~D["mask"]] == 0)
    mean, var = m.predict_grid(compute_var=False)
    assert var is None and mean.shape == (960, 1)
    assert rel(mean, D["grid_mean"]) < 1e-8
    pm, pv = m.predict(D["Xnew"])
    assert pm.shape == (5, 1) and pv.shape == (5, 1)
    print("predict mean", rel(pm, D["mean"]), "var", rel(pv, D["var"]))
    assert rel(pm, D["mean"]) < 1e-8
    assert rel(pv, D["var"]) < 1e-8


@pytest.mark.parametrize("precond", [None, 'kron'])
def test_model_exact_logdet_and_lml(gg, dense_model, precond):
    D = dense_model
    m = _grid_model(gg, D["y"], D["mask"], logdet='exact', precond=precond)
    lml = float(np.squeeze(m.log_likelihood()))
    print("logdet", m._cov_log_det(), D["ld"], "lml", lml, D["lml"])
    assert abs(m._cov_log_det() - D["ld"]) <= 1e-9 * abs(D["ld"])
    assert abs(lml - D["lml"]) <= 1e-9 * abs(D["lml"])
    assert m.num_observed == int(D["mask"].sum())


def test_model_scaled_eigs_logdet(gg, dense_model):
    D = dense_model
    m = _grid_model(gg, D["y"], D["mask"], logdet='scaled_eigs')
    m.fit()
    ref = mr.scaled_eigs_logdet(D["F"], D["mask"], S2)
    assert abs(m._cov_log_det() - ref) <= 1e-10 * abs(ref)


def test_model_exact_missing_max(gg, dense_model):
    D = dense_model
    m = _grid_model(gg, D["y"], D["mask"], logdet='exact', exact_missing_max=10)
    with pytest.raises(ValueError, match="exact_missing_max"):
        m.log_likelihood()


def test_model_optimize(gg, dense_model):
    D = dense_model
    m = _grid_model(gg, D["y"], D["mask"], logdet='scaled_eigs', cg_rtol=1e-10)
    before = float(np.squeeze(m.log_likelihood()))
    m.optimize(max_iters=2)
    after = float(np.squeeze(m.log_likelihood()))
    print("optimize: LML", before, "->", after)
    assert np.isfinite(after) and after >= before


# ------------------------------------------------------------ errors
def test_cg_mask_errors(gg):
    F, mask, y, _ = problem((7, 5, 3), 0.2)
    K = gg.tensors.KronMatrix(F, sym=True)
    cg = gg.linalg.cg
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask[:-1])                       # wrong length
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=np.zeros(105, bool))             # no observed point
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask, comm=True)
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask, basis='block')
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask, recurrence='fused')
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, precond='kron')                       # precond without mask
    with pytest.raises(ValueError):
        cg(K, y, shift=S2, mask=mask, precond='jacobi')
    with pytest.raises(ValueError):
        cg(K, y, shift=0.0, mask=mask)                           # W K W alone is singular
    with pytest.raises(ValueError):
        gg.linalg.MaskedKronCG(K, S2, mask).start(gg.device.zeros(104))


def test_cgm_abi_errors(gg):
    import torch
    from gp_grief_amd import native
    L = native.lib()
    F, mask, _, _ = problem((7, 5, 3), 0.2)
    K = gg.tensors.KronMatrix(F, sym=True)._device()
    work = gg.device.empty(4096)
    md = torch.from_numpy(mask.copy()).cuda().to(torch.uint8)
    h = ctypes.c_void_p()
    with pytest.raises(ValueError):    # NULL mask
        native.check(L.gg_cgm_create(K.h, S2, None, native.dptr(work), ctypes.byref(h)))
    with pytest.raises(ValueError):    # shift <= 0
        native.check(L.gg_cgm_create(K.h, -1.0, ctypes.c_void_p(md.data_ptr()),
                                     native.dptr(work), ctypes.byref(h)))
    rng = np.random.default_rng(0)
    R = gg.tensors.KronMatrix([rng.standard_normal((3, 4)), rng.standard_normal((5, 2))])._device()
    with pytest.raises(ValueError):    # non-square operator
        native.check(L.gg_cgm_create(R.h, S2, ctypes.c_void_p(md.data_ptr()),
                                     native.dptr(work), ctypes.byref(h)))
    ok = ctypes.c_void_p()
    native.check(L.gg_cgm_create(K.h, S2, ctypes.c_void_p(md.data_ptr()), native.dptr(work),
                                 ctypes.byref(ok)))
    try:
        with pytest.raises(ValueError):    # iterate before start
            native.check(L.gg_cgm_iterate(ok, 1, 0, native.stream_ptr()))
    finally:
        L.gg_cgm_destroy(ok)


def test_model_mask_errors(gg, dense_model):
    D = dense_model
    with pytest.raises(ValueError, match="cg"):
        gg.models.GPGridModel(*_model_args(gg), noise_var=S2, solver='exact', mask=D["mask"])
    with pytest.raises(ValueError, match="scaled_eigs"):
        _grid_model(gg, D["y"], D["mask"], logdet='slq')
    with pytest.raises(ValueError):
        _grid_model(gg, D["y"], D["mask"], precond='jacobi')
    with pytest.raises(ValueError):
        _grid_model(gg, D["y"], D["mask"][:-1])
    with pytest.raises(ValueError):
        gg.models.GPGridModel(*_model_args(gg), noise_var=S2, precond='kron')   # no mask
    m = _grid_model(gg, D["y"], D["mask"])
    with pytest.raises(ValueError, match="compute_var=False"):
        m.predict_grid(compute_var=True)


def _model_args(gg):
    d = len(MS)
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=0.1) for _ in range(d)]
    xg = [np.linspace(0, 1, MS[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    return xg, np.zeros((960, 1)), gg.kern.GridKernel(kerns)
