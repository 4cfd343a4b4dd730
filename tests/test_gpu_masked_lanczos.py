"""Masked Lanczos and the SLQ log det of an incomplete grid on the MI355X:
gg_lanczos_probe_masked, linalg.lanczos_tridiag(mask=), linalg.slq_logdet(mask=)
and GPGridModel(mask=, logdet='lanczos') against the NumPy restatement in
masked_lanczos_ref.py (itself checked against dense K_oo algebra on the CPU,
test_masked_lanczos_ref.py) and the dense log det.

Shapes, masks and sigma^2 = 0.01 as the masked CG tests: (7, 5, 3) has an odd
N = 105 (unaligned vectors, the scalar lanes), the rest even N (16-byte lanes);
d = 2, 3, 4, unequal factor orders, 10 - 60 % missing; make_mask forces the first
and last grid point missing (the lane edges).
Tolerances: the first 12 alphas at rtol 1e-8 and betas at 1e-7, as
test_fold_lanczos_vs_oracle for the unmasked probe; per-probe SLQ estimates
1e-5 |log det| (the CPU figure between two NumPy routes is 3.4e-7 at most);
the estimator within three standard errors of its own 16 probes.
"""
import ctypes

import numpy as np
import pytest

import masked_lanczos_ref as mlr
import masked_ref as mr

pytestmark = pytest.mark.gpu

S2 = 0.01


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


def check_tridiag(a, b, ao, bo):
    k = min(a.size, ao.size, 12)
    assert k >= 2
    np.testing.assert_allclose(a[:k], ao[:k], rtol=1e-8)
    np.testing.assert_allclose(b[:k - 1], bo[:k - 1], rtol=1e-7)


# ------------------------------------------------------------ tridiagonal
@pytest.mark.parametrize("ms,frac", mlr.CASES)
def test_masked_tridiag_vs_numpy(gg, ms, frac):
    C = mlr.case(ms, frac, S2)
    F, mask = C["F"], C["mask"]
    K = gg.tensors.KronMatrix(F, sym=True)
    a, b = gg.linalg.lanczos_tridiag(K, S2, 20, seed=7, probe=2, mask=mask)
    ao, bo = mlr.masked_lanczos(F, mask, S2, 7, 2, 20)
    k = min(a.size, ao.size, 12)
    print("masked Lanczos", ms, frac, "alpha", np.max(np.abs(a[:k] / ao[:k] - 1)),
          "beta", np.max(np.abs(b[:k - 1] / bo[:k - 1] - 1)))
    assert a.size == 20 and b.size == 19
    check_tridiag(a, b, ao, bo)
    assert gg.linalg.lanczos_tridiag.n_observed == int(mask.sum())


@pytest.mark.parametrize("ms", [(9, 8, 7), (20, 18, 16, 12)])
def test_all_ones_mask_is_the_unmasked_probe(gg, ms):
    K = gg.tensors.KronMatrix(mr.rbf_factors(ms), sym=True)
    n = int(np.prod(ms))
    a, b = gg.linalg.lanczos_tridiag(K, S2, 20, seed=7, probe=2, mask=np.ones(n, dtype=bool))
    au, bu = gg.linalg.lanczos_tridiag(K, S2, 20, seed=7, probe=2)
    assert gg.linalg.lanczos_tridiag.n_observed == n
    check_tridiag(a, b, au, bu)


def test_mask_kinds_and_alignment(gg):
    """numpy bool / uint8 and device tensors; a device mask one byte into an
    allocation (mask_dev at any alignment) gives the same tridiagonal."""
    import torch
    C = mlr.case((12, 10, 8), 0.3, S2)
    mask = C["mask"]
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    ref = gg.linalg.lanczos_tridiag(K, S2, 12, seed=7, probe=2, mask=mask)
    md = torch.from_numpy(mask.copy()).cuda()
    buf = torch.zeros(mask.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = md.to(torch.uint8)
    assert buf[1:].data_ptr() % 2 == 1
    for m in (mask.astype(np.uint8), 3 * mask.astype(np.uint8), md, md.to(torch.uint8), buf[1:]):
        a, b = gg.linalg.lanczos_tridiag(K, S2, 12, seed=7, probe=2, mask=m)
        assert np.array_equal(a, ref[0]) and np.array_equal(b, ref[1])
        assert gg.linalg.lanczos_tridiag.n_observed == int(mask.sum())


def test_timed_twin(gg):
    C = mlr.case((12, 10, 8), 0.3, S2)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    work = gg.device.empty(4 * 960)
    a, b = gg.linalg.lanczos_tridiag(K, S2, 12, seed=7, probe=2, mask=C["mask"], work=work)
    out = gg.linalg.lanczos_tridiag(K, S2, 12, seed=7, probe=2, mask=C["mask"], work=work,
                                    timed=True)
    assert len(out) == 3
    assert np.array_equal(out[0], a) and np.array_equal(out[1], b)
    assert len(out[2]) == 12 and all(ms > 0 for ms in out[2])


# ------------------------------------------------------------ SLQ
@pytest.mark.parametrize("ms,frac", mlr.CASES)
def test_masked_slq_vs_numpy_and_dense(gg, ms, frac):
    C = mlr.case(ms, frac, S2)
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    mean, ests = gg.linalg.slq_logdet(K, S2, probes=16, steps=40, seed=3, mask=C["mask"])
    mo, eo = C["slq"]
    se = float(np.std(ests)) / 4.0
    print("masked SLQ", ms, frac, "mean", mean, "numpy", mo, "dense", C["ld"], "se", se,
          "per-probe", np.max(np.abs(ests - eo)) / abs(C["ld"]))
    assert ests.shape == (16,)
    assert np.max(np.abs(ests - eo)) <= 1e-5 * abs(C["ld"])
    assert abs(mean - C["ld"]) <= 3.0 * se


# ------------------------------------------------------------ model
MS = (16, 16, 8)


def _grid_model(gg, y, mask, **kw):
    """GPGridModel whose operator has masked_ref.rbf_factors(MS) (cov_grid
    reverses the input dimensions: input j is factor d - 1 - j)."""
    d = len(MS)
    ls = [0.1 * (1 + 0.05 * i) for i in range(d)]
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=ls[d - 1 - j]) for j in range(d)]
    xg = [np.linspace(0, 1, MS[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    kw.setdefault("cg_rtol", 1e-11)
    return gg.models.GPGridModel(xg, y.reshape(-1, 1), gg.kern.GridKernel(kerns), noise_var=S2,
                                 solver='cg', mask=mask, **kw)


@pytest.fixture(scope="module")
def many_missing():
    """(16, 16, 8) with 60 % missing: 1229 missing points (make_mask's 1229
    draws already hold the first grid point), above the exact log det's
    exact_missing_max = 1024, 819 observed; the dense LML."""
    C = mlr.case(MS, 0.6, S2)
    mask = C["mask"]
    y = np.random.default_rng(1).standard_normal(mask.size)
    o = np.nonzero(mask)[0]
    Koo = mr.dense_K(C["F"])[np.ix_(o, o)] + S2 * np.eye(o.size)
    lml = -0.5 * (float(y[o].dot(np.linalg.solve(Koo, y[o]))) + C["ld"]
                  + o.size * np.log(2 * np.pi))
    return dict(mask=mask, y=y, lml=lml)


def test_model_lanczos_where_exact_is_refused(gg, many_missing):
    D = many_missing
    assert int((~D["mask"]).sum()) == 1229 and int(D["mask"].sum()) == 819
    m = _grid_model(gg, D["y"], D["mask"], logdet='exact')
    with pytest.raises(ValueError, match="exact_missing_max"):
        m.log_likelihood()
    m = _grid_model(gg, D["y"], D["mask"], logdet='lanczos', slq_probes=16, slq_steps=40, seed=3)
    lml = float(np.squeeze(m.log_likelihood()))
    assert m.slq_estimates.shape == (16,)
    se = float(np.std(m.slq_estimates)) / 4.0
    print("LML", lml, "dense", D["lml"], "se(log det)", se)
    assert abs(lml - D["lml"]) <= 0.5 * 3.0 * se + 1e-6 * abs(D["lml"])


def test_model_lanczos_optimize(gg, many_missing):
    D = many_missing
    m = _grid_model(gg, D["y"], D["mask"], logdet='lanczos', slq_probes=16, slq_steps=40, seed=3,
                    cg_rtol=1e-10)
    before = float(np.squeeze(m.log_likelihood()))
    m.optimize(max_iters=2)
    after = float(np.squeeze(m.log_likelihood()))
    print("optimize: LML", before, "->", after)
    assert np.isfinite(after) and after >= before


# ------------------------------------------------------------ errors
def test_masked_lanczos_errors(gg, many_missing):
    C = mlr.case((7, 5, 3), 0.2, S2)
    mask = C["mask"]
    K = gg.tensors.KronMatrix(C["F"], sym=True)
    lt = gg.linalg.lanczos_tridiag
    with pytest.raises(ValueError):
        lt(K, S2, 5, mask=mask[:-1])                        # wrong length
    with pytest.raises(ValueError):
        lt(K, S2, 5, mask=np.zeros(105, bool))              # no observed point
    with pytest.raises(ValueError):
        lt(K, S2, 5, mask=gg.device.torch().zeros(105, dtype=gg.device.torch().uint8,
                                                  device="cuda"))   # counted by the library
    with pytest.raises(ValueError):
        lt(K, S2, 0, mask=mask)                             # steps = 0
    with pytest.raises(ValueError):
        gg.linalg.slq_logdet(K, S2, mask=mask[:-1])
    D = many_missing
    d = len(MS)
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=0.1) for _ in range(d)]
    xg = [np.linspace(0, 1, MS[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    with pytest.raises(ValueError, match="slq"):            # a complete grid uses 'slq'
        gg.models.GPGridModel(xg, D["y"].reshape(-1, 1), gg.kern.GridKernel(kerns),
                              noise_var=S2, logdet='lanczos')
    with pytest.raises(ValueError, match="lanczos"):        # the message lists every choice
        _grid_model(gg, D["y"], D["mask"], logdet='slq')


def test_masked_lanczos_abi_errors(gg):
    import torch
    from gp_grief_amd import native
    L = native.lib()
    C = mlr.case((7, 5, 3), 0.2, S2)
    K = gg.tensors.KronMatrix(C["F"], sym=True)._device()
    work = gg.device.empty(4 * 105)
    md = torch.from_numpy(C["mask"].copy()).cuda().to(torch.uint8)
    a, b = (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
    done, nobs = ctypes.c_int(), ctypes.c_int64()

    def call(kh, shift, mp, steps):
        return L.gg_lanczos_probe_masked(kh, shift, mp, 7, 2, steps, native.dptr(work), a, b,
                                         ctypes.byref(done), ctypes.byref(nobs),
                                         native.stream_ptr())
    mp = ctypes.c_void_p(md.data_ptr())
    assert call(K.h, S2, None, 4) == native.GG_ERR_VALUE          # NULL mask
    rng = np.random.default_rng(0)
    R = gg.tensors.KronMatrix([rng.standard_normal((3, 4)), rng.standard_normal((5, 2))])._device()
    assert call(R.h, S2, mp, 4) == native.GG_ERR_VALUE            # non-square operator
    assert call(K.h, S2, mp, 0) == native.GG_ERR_VALUE            # steps < 1
    assert call(K.h, -1.0, mp, 4) == native.GG_ERR_VALUE          # shift < 0
    assert call(K.h, S2, mp, 4) == native.GG_OK
    assert nobs.value == int(C["mask"].sum()) and done.value == 4
    sm = (ctypes.c_double * 4)()
    assert L.gg_lanczos_probe_masked_timed(K.h, S2, mp, 7, 2, 4, native.dptr(work), a, b,
                                           ctypes.byref(done), ctypes.byref(nobs), None,
                                           native.stream_ptr()) == native.GG_ERR_VALUE
    assert L.gg_lanczos_probe_masked_timed(K.h, S2, mp, 7, 2, 4, native.dptr(work), a, b,
                                           ctypes.byref(done), ctypes.byref(nobs), sm,
                                           native.stream_ptr()) == native.GG_OK
