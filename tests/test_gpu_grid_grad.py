"""The analytic LML gradient of GPGridModel on the device, layer by layer,
against the dense NumPy reference of tests/grid_grad_ref.py:

  gg_cov_grad_param   elementwise against np.longdouble,
                      |got - ref| <= (D + 12)(1 + t) u |ref| for the
                      lengthscale derivative: grief_abi_ref.cov_bound's D + 8
                      plus the derivative's own operations, at most four (the
                      scale by r or r^2 with its constant, the division by the
                      lengthscale, the product with the rest); the variance
                      derivative is k at unit variance and meets cov_bound
                      itself.
  gg_kron_trace_ratio against the long-double grid sum,
                      |got - ref| <= (2 d + 66) u sum|term|: 2 d + 2 roundings
                      of one term, 64 for the sums.  The launch runs one work
                      item per (head, segment of the last factor): segments of
                      at most 16 points wherever the heads alone do not fill
                      the device, so a thread's chain is <= 16 additions at
                      every shape of the issue (16 at 84^3; chain + 34 <= 64
                      with the block's and the row reduction's levels).  Two
                      added shapes leave that regime and state their chain:
                      (512, 256, 40) runs whole 40-point runs (bound 2 d + 2 +
                      74), and (2048, 1024, 1024) -- N = 2^31, the 64-bit index
                      path -- runs 128-point segments in 32 grid-stride passes
                      (chain 4096), checked at shift 0 against the closed form
                      prod_f sum_i num_f[i] / lam_f[i].
  linalg.trace_grad   per-probe values against the NumPy estimator on
                      oracle.cg.probe_signs, 10 rtol cond(A) sum|terms|.
  GPGridModel         grad_method='adjoint' against the dense gradient,
                      1e3 u cond(K + s I) sum|parts| on the complete grid; the
                      masked gradient against the dense data-fit term minus
                      half the mean of the NumPy probe values.
"""
import ctypes

import numpy as np
import pytest

import grid_grad_ref as G
import grief_abi_ref as R
import masked_ref as MR

pytestmark = pytest.mark.gpu

LD = np.longdouble
GG_OK, GG_ERR_VALUE = 0, -1


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


class Buf(object):
    """A float64 array inside a device buffer with 64 NaNs before and after."""

    def __init__(self, region, guard=64):
        import torch
        region = np.ascontiguousarray(region, dtype=np.float64)
        self.shape, self.lo = region.shape, guard
        self.h0 = np.full(guard + region.size + guard, np.nan)
        self.h0[guard:guard + region.size] = region.reshape(-1)
        self.d = torch.from_numpy(self.h0.copy()).cuda()

    def ptr(self):
        return ctypes.c_void_p(self.d.data_ptr() + 8 * self.lo)

    def read(self, written=True):
        """The array now; the guards (and, written=False, the array) must hold
        the bits they held."""
        flat = self.d.cpu().numpy()
        n = int(np.prod(self.shape))
        a, b = flat.copy(), self.h0.copy()
        if written:
            a[self.lo:self.lo + n] = b[self.lo:self.lo + n] = 0
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "written outside the output"
        return flat[self.lo:self.lo + n].reshape(self.shape).copy()


def within(got, ref, bound, what):
    got = np.asarray(got)
    assert not np.any(np.isnan(got)), "%s: NaN in the result" % (what,)
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    worst = float(np.max(err / np.where(bound > 0, bound, 1))) if err.size else 0.0
    print("%s: worst err / bound %.4f" % (what, worst))
    assert np.all(err <= bound), "%s: err / bound %.3g" % (what, worst)


# ------------------------------------------------------- gg_cov_grad_param
COV_SHAPES = [(1, 1), (7, 5), (65, 33)]
COV_VAR = 1.3


def run_grad_param(nat, kind, ls, D, x, z, which):
    nx, nz = x.shape[0], z.shape[0]
    xb, zb, ob = Buf(x), Buf(z), Buf(np.full((nx, nz), np.nan))
    st = nat.lib().gg_cov_grad_param(kind, COV_VAR, ls, D, xb.ptr(), nx, zb.ptr(), nz, which,
                                     ob.ptr(), nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    xb.read(written=False)
    zb.read(written=False)
    return ob.read()


@pytest.mark.parametrize("D", (1, 3))
@pytest.mark.parametrize("kind", range(4))
def test_cov_grad_param(nat, kind, D):
    """All kinds, both parameters, D in {1, 3}, 1 x 1 / 7 x 5 / 65 x 33 (several
    blocks), lengthscales 0.3 and 2: |got - ref| <= (D + 12)(1 + t) u |ref|
    (cov_bound's D + 8 and the derivative's four extra operations); the
    variance derivative meets cov_bound."""
    for ls in (0.3, 2.0):
        for nx, nz in COV_SHAPES:
            x, z = R.cov_problem(kind, D, ls, nx, nz, COV_VAR)[:2]
            for which in (0, 1):
                ref, t = G.grad_param_ref(kind, COV_VAR, ls, x, z, which)
                bound = R.cov_bound(D, ref, t) if which == 0 else G.grad_param_bound(D, ref, t)
                got = run_grad_param(nat, kind, ls, D, x, z, which)
                within(got, ref, bound, "gg_cov_grad_param kind %d D %d ls %g %dx%d which %d"
                       % (kind, D, ls, nx, nz, which))


@pytest.mark.parametrize("D", (1, 3))
def test_cov_grad_param_delta_rbf(nat, D):
    """l = 1e-7: the lengthscale derivative is exactly 0, the variance
    derivative exactly the delta."""
    rng = np.random.default_rng(40 + D)
    z = rng.random((5, D))
    x = rng.random((7, D))
    x[::3] = z[:3]
    hit = (x[:, None, :] == z[None, :, :]).all(-1)
    assert hit.sum() >= 3
    assert np.array_equal(run_grad_param(nat, 0, 1e-7, D, x, z, 1), np.zeros((7, 5)))
    assert np.array_equal(run_grad_param(nat, 0, 1e-7, D, x, z, 0), np.where(hit, 1.0, 0.0))


def test_cov_grad_param_empty_and_errors(nat):
    L, s = nat.lib(), nat.stream_ptr()
    x, z, ob = Buf(np.ones((4, 2))), Buf(np.ones((3, 2))), Buf(np.full((4, 3), np.nan))
    assert L.gg_cov_grad_param(0, 1.0, 0.3, 2, x.ptr(), 0, z.ptr(), 3, 1, ob.ptr(), s) == GG_OK
    assert L.gg_cov_grad_param(0, 1.0, 0.3, 2, x.ptr(), 4, z.ptr(), 0, 0, ob.ptr(), s) == GG_OK
    for kind, which, dims, xp, zp, op in [(-1, 0, 2, x.ptr(), z.ptr(), ob.ptr()),
                                          (4, 0, 2, x.ptr(), z.ptr(), ob.ptr()),
                                          (0, 2, 2, x.ptr(), z.ptr(), ob.ptr()),
                                          (0, -1, 2, x.ptr(), z.ptr(), ob.ptr()),
                                          (0, 0, 0, x.ptr(), z.ptr(), ob.ptr()),
                                          (0, 0, 2, None, z.ptr(), ob.ptr()),
                                          (0, 0, 2, x.ptr(), None, ob.ptr()),
                                          (0, 0, 2, x.ptr(), z.ptr(), None)]:
        assert L.gg_cov_grad_param(kind, 1.0, 0.3, dims, xp, 4, zp, 3, which, op, s) \
            == GG_ERR_VALUE
    ob.read(written=False)


def test_kernel_cov_grad_param(gg):
    """Stationary.cov_grad_param: numpy in, numpy out; device tensors stay on
    the device; kernels with children raise."""
    import torch
    g = np.linspace(0.0, 1.0, 7).reshape(-1, 1)
    k = gg.kern.Matern52(1, variance=1.3, lengthscale=0.27)
    out = k.cov_grad_param(g)
    ref = G.dk_1d("Matern52", g, 1.3, 0.27)
    for name in ('variance', 'lengthscale'):
        assert isinstance(out[name], np.ndarray) and out[name].shape == (7, 7)
        assert np.allclose(out[name], ref[name], rtol=1e-13, atol=1e-15)
    od = k.cov_grad_param(torch.from_numpy(g).cuda(), torch.from_numpy(g[:3]).cuda())
    assert od['lengthscale'].is_cuda and tuple(od['lengthscale'].shape) == (7, 3)
    assert np.allclose(od['lengthscale'].cpu().numpy(), ref['lengthscale'][:, :3], rtol=1e-13,
                       atol=1e-15)
    with pytest.raises(NotImplementedError):
        (k * gg.kern.RBF(1)).cov_grad_param(g)


def test_cov_grid_grad_order_and_positions(gg):
    """One entry per kernel parameter, in GridKernel.parameters' order, at the
    reversed factor position; dim_noise_var does not enter."""
    p = G.mixed_problem((6, 5, 4))
    gk = gg.kern.GridKernel(p.kernels(gg))
    got = gk.cov_grid_grad(p.xg, dim_noise_var=1e-3)
    ref = p.dfactors()
    assert len(got) == gk.parameters.size == len(ref)
    for (pos, dk), (rpos, rdk) in zip(got, ref):
        assert pos == rpos and dk.shape == rdk.shape
        assert np.allclose(dk, rdk, rtol=1e-13, atol=1e-15)
    with pytest.raises(NotImplementedError):
        gg.kern.GridKernel(p.kernels(gg), radial_kernel=True).cov_grid_grad(p.xg, 1e-12)


# ----------------------------------------------------- gg_kron_trace_ratio
TRACE_SHAPES = [(7,), (5, 4), (6, 5, 4), (3, 4, 2, 5), (4, 1, 3), (2,) * 12, (33, 17, 9),
                (84, 84, 84)]
SHIFT = 0.3


def trace_inputs(ms, P):
    rng = np.random.default_rng(1000 * len(ms) + sum(ms) + P)
    lam = rng.uniform(0.5, 2.0, sum(ms))
    num = rng.uniform(-1.0, 1.0, (P, sum(ms)))        # mixed sign
    return lam, num


def run_trace(nat, ms, lam, num, shift, P=None):
    lb, nb = Buf(lam), Buf(num)
    P = num.shape[0] if P is None else P
    out = (ctypes.c_double * (P + 2))(*([np.nan] * (P + 2)))
    st = nat.lib().gg_kron_trace_ratio(len(ms), nat.i64_array(ms), lb.ptr(), float(shift), P,
                                       nb.ptr(), ctypes.cast(ctypes.byref(out, 8),
                                                             ctypes.POINTER(ctypes.c_double)),
                                       nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    lb.read(written=False)
    nb.read(written=False)
    res = np.array(out[:])
    assert np.isnan(res[0]) and np.isnan(res[-1]), "written outside out[0 .. P)"
    return res[1:-1]


@pytest.mark.parametrize("P", (1, 5, 33))
@pytest.mark.parametrize("ms", TRACE_SHAPES, ids=lambda ms: "x".join(map(str, ms)))
def test_trace_ratio(nat, ms, P):
    """Mixed-sign numerators against the long-double grid sum, (2 d + 66) u
    sum|term|; every shape keeps a thread's chain <= 16 additions (16 at 84^3,
    whose last factor is cut into 6 segments over 166 blocks); P = 33 runs five
    row chunks of 7 in the one launch, the last with two rows past P."""
    assert G.trace_ratio_chain(ms) <= 16
    lam, num = trace_inputs(ms, P)
    ref, scale = G.trace_ratio_ref(ms, lam, num, SHIFT)
    got = run_trace(nat, ms, lam, num, SHIFT)
    within(got, ref, G.trace_ratio_bound(len(ms), scale), "gg_kron_trace_ratio %r P %d" % (ms, P))


@pytest.mark.parametrize("ms,P", [((1024, 1024, 2), 5), ((512, 256, 40), 2)],
                         ids=("two_passes", "whole_runs"))
def test_trace_ratio_other_geometries(nat, ms, P):
    """(1024, 1024, 2): 2^20 items, two grid-stride passes of 2-point runs
    (chain 4).  (512, 256, 40): the heads fill the device, whole 40-point runs
    per item: chain 40, so the sums' share of the bound is 40 + 34 = 74."""
    chain = G.trace_ratio_chain(ms)
    assert chain == {2: 4, 40: 40}[ms[-1]]
    lam, num = trace_inputs(ms, P)
    ref, scale = G.trace_ratio_ref(ms, lam, num, SHIFT)
    got = run_trace(nat, ms, lam, num, SHIFT)
    within(got, ref, G.trace_ratio_bound(len(ms), scale, chain),
           "gg_kron_trace_ratio %r P %d" % (ms, P))


def test_trace_ratio_past_2_31(nat):
    """N = 2^31: the 64-bit index path (128-point segments, 32 grid-stride
    passes: chain 4096).  At shift 0 the grid sum factorises, prod_f sum_i
    num_f[i] / lam_f[i]: the reference and the scale in closed form.  Rows:
    lam itself (every term 1, the sum N), all ones, mixed sign."""
    ms = (2048, 1024, 1024)
    chain = G.trace_ratio_chain(ms)
    assert chain == 4096 and int(np.prod(ms)) == 1 << 31
    lam, num = trace_inputs(ms, 3)
    num[0], num[1] = lam, 1.0
    off = np.concatenate([[0], np.cumsum(ms)])
    ref, scale = np.ones(3, dtype=LD), np.ones(3, dtype=LD)
    for f in range(3):
        q = num[:, off[f]:off[f + 1]].astype(LD) / lam[off[f]:off[f + 1]].astype(LD)
        ref *= q.sum(axis=1)
        scale *= np.abs(q).sum(axis=1)
    assert abs(ref[0] - LD(2.0) ** 31) < 1e-6
    got = run_trace(nat, ms, lam, num, 0.0)
    within(got, ref, G.trace_ratio_bound(3, scale, chain), "gg_kron_trace_ratio 2^31")


@pytest.mark.parametrize("ms", TRACE_SHAPES, ids=lambda ms: "x".join(map(str, ms)))
def test_trace_ratio_lam_over_lam_is_n(nat, ms):
    """The numerator row equal to lam at shift 0: every term is 1, the sum N."""
    lam = trace_inputs(ms, 1)[0]
    n = int(np.prod(ms))
    got = run_trace(nat, ms, lam, lam[None, :], 0.0)
    within(got, np.array([LD(n)]), G.trace_ratio_bound(len(ms), np.array([LD(n)])),
           "lam / lam %r" % (ms,))


def test_trace_ratio_is_bitwise_reproducible(nat):
    for ms, P in (((33, 17, 9), 5), ((84, 84, 84), 33)):
        lam, num = trace_inputs(ms, P)
        a = run_trace(nat, ms, lam, num, SHIFT)
        b = run_trace(nat, ms, lam, num, SHIFT)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_trace_ratio_status_codes(nat):
    L, s = nat.lib(), nat.stream_ptr()
    ms = (6, 5, 4)
    lam, num = trace_inputs(ms, 2)
    assert run_trace(nat, ms, lam, num, SHIFT, P=0).size == 0      # OK, nothing written
    lb, nb = Buf(lam), Buf(num)
    out = (ctypes.c_double * 2)()
    m = nat.i64_array(ms)
    assert L.gg_kron_trace_ratio(3, m, lb.ptr(), SHIFT, 2, nb.ptr(), out, s) == GG_OK
    for d, mm, lp, P, npt, op in [(3, m, None, 2, nb.ptr(), out),
                                  (3, m, lb.ptr(), 2, None, out),
                                  (3, m, lb.ptr(), 2, nb.ptr(), None),
                                  (3, m, lb.ptr(), -1, nb.ptr(), out),
                                  (0, m, lb.ptr(), 2, nb.ptr(), out),
                                  (17, nat.i64_array((1,) * 17), lb.ptr(), 2, nb.ptr(), out),
                                  (3, nat.i64_array((6, 0, 4)), lb.ptr(), 2, nb.ptr(), out)]:
        assert L.gg_kron_trace_ratio(d, mm, lp, SHIFT, P, npt, op, s) == GG_ERR_VALUE
    m16 = (2, 1, 2, 1) * 4
    lam, num = trace_inputs(m16, 3)
    ref, scale = G.trace_ratio_ref(m16, lam, num, SHIFT)
    within(run_trace(nat, m16, lam, num, SHIFT), ref, G.trace_ratio_bound(16, scale), "d = 16")


# ------------------------------------------------------ complete-grid model
MS = (6, 5, 4)


@pytest.fixture(scope="module")
def complete():
    """The (6, 5, 4) RBF / Matern32 / Matern52 problem and its dense gradient."""
    p = G.mixed_problem(MS)
    fit, tr = G.dense_parts(p)
    return dict(p=p, grad=fit - 0.5 * tr, parts=np.abs(fit) + 0.5 * np.abs(tr),
                cond=float(np.linalg.cond(G.dense_A(p))), lml=G.dense_lml(p))


def grid_model(gg, p, **kw):
    gk = gg.kern.GridKernel(p.kernels(gg))
    return gg.models.GPGridModel(p.xg, p.y, gk, noise_var=p.s, **kw)


@pytest.mark.parametrize("kw", [dict(solver='exact'), dict(solver='cg', cg_rtol=1e-13)],
                         ids=("exact", "cg"))
def test_model_gradient_complete_grid(gg, complete, kw):
    """grad_method='adjoint' against the dense gradient:
    1e3 u cond(K + s I) sum|parts| per free parameter; the same gradient, bit
    for bit, for logdet='exact' and logdet='slq' (the traces are exact either
    way)."""
    C = complete
    p = C["p"]
    m = grid_model(gg, p, grad_method='adjoint', **kw)
    ll, g = m.log_likelihood(return_gradient=True)
    tol = 1e3 * G.U53 * C["cond"] * C["parts"]
    err = np.abs(g - C["grad"])
    print("cond %.3g; err / tol per free parameter: %s" % (C["cond"], (err / tol)[p.free]))
    assert g.shape == (1 + 2 * p.d,) and np.all(np.isfinite(g))
    assert np.all(err[p.free] <= tol[p.free])
    assert abs(float(np.squeeze(ll)) - C["lml"]) <= 1e3 * G.U53 * C["cond"] * abs(C["lml"])
    m2 = grid_model(gg, p, grad_method='adjoint', logdet='slq', **kw)
    g2 = m2.log_likelihood(return_gradient=True)[1]
    assert np.array_equal(g, g2)


def test_model_checkgrad_and_optimize(gg, complete):
    """checkgrad (forward differences at 1e-6 against the analytic gradient, 3
    decimals of the ratio) passes at this point away from the optimum --
    test_grid_grad_ref.py shows the dense forward differences within 1e-3
    there -- and five L-BFGS iterations on the analytic gradient do not lower
    the LML."""
    m = grid_model(gg, complete["p"], grad_method='adjoint')
    assert m.checkgrad()
    before = float(np.squeeze(m.log_likelihood()))
    m.optimize(max_iters=5)
    after = float(np.squeeze(m.log_likelihood()))
    print("LML %.6f -> %.6f" % (before, after))
    assert after >= before


# ------------------------------------------------------------------ masked
RTOL = 1e-12


@pytest.fixture(scope="module")
def masked():
    p = G.mixed_problem(MS)
    p.mask = MR.make_mask(p.N, 0.2)
    fit, tr = G.dense_parts(p)
    return dict(p=p, fit=fit, tr=tr, cond=float(np.linalg.cond(G.dense_A(p))))


def kron_ops(gg, p):
    F = p.factors()
    K = gg.tensors.KronMatrix(F, sym=True)
    dKs = [gg.tensors.KronMatrix(G.replaced(F, pos, dKf), sym=True) for pos, dKf in p.dfactors()]
    return K, dKs


def test_trace_grad_unit_vectors_give_the_exact_traces(gg, masked):
    """Z = the unit vectors of the observed points: the column sums are
    tr(A^-1) and tr(A^-1 dK_oo), 10 rtol cond(A) sum|terms|."""
    D = masked
    p = D["p"]
    o = np.nonzero(p.mask)[0]
    Z = np.zeros((p.N, o.size))
    Z[o, np.arange(o.size)] = 1.0
    K, dKs = kron_ops(gg, p)
    means, per = gg.linalg.trace_grad(K, dKs, p.s, mask=p.mask, rtol=RTOL, Z=Z)
    ref, absref = G.probe_estimates(p, 0, Z=Z)
    tol = 10 * RTOL * D["cond"] * absref.sum(axis=0)
    err = np.abs(per.sum(axis=0) - D["tr"])
    print("cond(A) %.3g; err / tol %s" % (D["cond"], err / tol))
    assert per.shape == (o.size, 1 + len(dKs))
    assert np.all(err <= tol)
    assert np.allclose(means, per.mean(axis=0), rtol=1e-15, atol=0)


def test_trace_grad_default_probes_match_numpy(gg, masked):
    """per_probe on probe_signs(seed, j, N) * mask, elementwise, 10 rtol
    cond(A) |terms|; a device mask and Z give the same values."""
    import torch
    D = masked
    p = D["p"]
    K, dKs = kron_ops(gg, p)
    means, per = gg.linalg.trace_grad(K, dKs, p.s, mask=p.mask, probes=5, seed=3, rtol=RTOL)
    ref, absref = G.probe_estimates(p, 3, probes=5)
    tol = 10 * RTOL * D["cond"] * absref
    print("worst err / tol %.3g" % float(np.max(np.abs(per - ref) / tol)))
    assert per.shape == (5, 1 + len(dKs))
    assert np.all(np.abs(per - ref) <= tol)
    Z = np.stack([G.probe_signs(3, j, p.N) for j in range(5)], axis=1)
    per2 = gg.linalg.trace_grad(K, dKs, p.s, mask=torch.from_numpy(p.mask).cuda(), rtol=RTOL,
                                Z=torch.from_numpy(Z).cuda())[1]
    assert np.array_equal(per, per2)


def test_trace_grad_without_mask(gg, complete):
    """No mask: KronCG solves; the estimator on the full probes."""
    p = complete["p"]
    K, dKs = kron_ops(gg, p)
    per = gg.linalg.trace_grad(K, dKs[:2], p.s, probes=3, seed=1, rtol=RTOL)[1]
    ref, absref = G.probe_estimates(p, 1, probes=3)
    tol = 10 * RTOL * complete["cond"] * absref[:, :3]
    assert np.all(np.abs(per - ref[:, :3]) <= tol)


@pytest.mark.parametrize("logdet", ("exact", "lanczos"))
def test_model_gradient_masked(gg, masked, logdet):
    """_adjoint_gradient = the dense data-fit term minus half the mean of the
    NumPy probe values (same seed, same probes), 10 rtol cond(A) sum|terms|;
    grad_estimates is (probes, 1 + kernel parameters); a second model gives
    the same bits."""
    D = masked
    p = D["p"]
    kw = dict(mask=p.mask, logdet=logdet, grad_method='adjoint', cg_rtol=RTOL, grad_probes=6,
              seed=2)
    m = grid_model(gg, p, **kw)
    ll, g = m._adjoint_gradient(m.parameters)
    ref, absref = G.probe_estimates(p, 2, probes=6)
    want = D["fit"] - 0.5 * ref.mean(axis=0)
    tol = 10 * RTOL * D["cond"] * (np.abs(D["fit"]) + 0.5 * absref.mean(axis=0))
    err = np.abs(g - want)
    print("err / tol per free parameter: %s" % (err / tol)[p.free])
    assert m.grad_estimates.shape == (6, 1 + 2 * p.d)
    assert np.all(np.abs(m.grad_estimates - ref) <= 10 * RTOL * D["cond"] * absref)
    assert np.all(err[p.free] <= tol[p.free]) and np.all(np.isfinite(g))
    m2 = grid_model(gg, p, **kw)
    g2 = m2.log_likelihood(return_gradient=True)[1]
    assert np.array_equal(g, g2) and np.array_equal(m.grad_estimates, m2.grad_estimates)


def test_grad_probes_default_is_slq_probes(gg, masked):
    p = masked["p"]
    m = grid_model(gg, p, mask=p.mask, grad_method='adjoint', slq_probes=3)
    m.log_likelihood(return_gradient=True)
    assert m.grad_estimates.shape == (3, 1 + 2 * p.d)


# ------------------------------------------------------------- constructor
def test_constructor(gg, complete):
    p = complete["p"]
    assert grid_model(gg, p).grad_method == 'finite_difference'
    assert grid_model(gg, p, grad_method='adjoint').grad_method == 'adjoint'
    gk = gg.kern.GridKernel(p.kernels(gg), radial_kernel=True)
    with pytest.raises(ValueError, match="adjoint"):
        gg.models.GPGridModel(p.xg, p.y, gk, noise_var=p.s, grad_method='adjoint')
    gk = gg.kern.GridKernel([k * gg.kern.RBF(1) for k in p.kernels(gg)])
    with pytest.raises(ValueError, match="adjoint"):
        gg.models.GPGridModel(p.xg, p.y, gk, noise_var=p.s, grad_method='adjoint')
    with pytest.raises(ValueError, match="grad_method"):
        grid_model(gg, p, grad_method='autodiff')
