"""Structured kernel interpolation on the MI355X: the stencil kernel, interp /
spread against a dense W, the CG on the points, SLQ from the CG's
coefficients and GPSKIModel, against the NumPy restatement in ski_ref.py.

Shapes are the smallest at which each kernel can still go wrong: one-cell
domains (every stencil is the whole axis), unequal orders, n = 1, odd n, more
points than nodes, empty nodes, one crowded cell (rows of the inverted index
long enough for the split path), buffers off 16-byte alignment.
Tolerances: interp / spread 1e-12 max|input| (256 terms x 1.1e-16 x 1.25^4 ~
7e-14 for interp; spread rows stay <= 6000 entries, the same margin).
"""
import ctypes

import numpy as np
import pytest

import ski_ref as sr
from oracle.cg import probe_signs

pytestmark = pytest.mark.gpu

ORDERS = {"cubic": 4, "linear": 2}
S2 = 0.05


def lml_of(model):
    return float(np.squeeze(model.log_likelihood()))


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


def axes(ms, lo=-0.3, hi=1.2):
    return [np.linspace(lo + 0.05 * f, hi + 0.1 * f, m).reshape(-1, 1) for f, m in enumerate(ms)]


def edge_points(xg, order):
    """Points on nodes, on cell boundaries and on both domain edges of every
    axis (the other coordinates mid-domain)."""
    pad = 1 if order == 4 else 0
    mid = [0.5 * (g[pad, 0] + g[len(g) - 1 - pad, 0]) for g in xg]
    P = []
    for f, g in enumerate(xg):
        for j in range(pad, len(g) - pad):
            p = list(mid)
            p[f] = g[j, 0]
            P.append(p)
    return np.array(P)


def raw_stencils(gg, xg, X, order, first, w):
    """gg_ski_stencils into the given device tensors: (status, outside)."""
    import torch
    native = gg.native
    d = len(xg)
    ax = [sr.axis_params(g) for g in xg]
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).cuda()
    out = ctypes.c_int64(-1)
    st = native.lib().gg_ski_stencils(
        d, native.i64_array([a[2] for a in ax]), (ctypes.c_double * d)(*[a[0] for a in ax]),
        (ctypes.c_double * d)(*[a[1] for a in ax]), order, native.dptr(Xd), X.shape[0],
        ctypes.c_void_p(first.data_ptr()), native.dptr(w), ctypes.byref(out),
        native.stream_ptr())
    torch.cuda.synchronize()
    return st, out.value


# ------------------------------------------------------------------- stencils
STENCIL_GRIDS = [("cubic", (4,)), ("cubic", (4, 4)), ("cubic", (7, 4, 5)),
                 ("cubic", (5, 4, 6, 4)), ("linear", (2,)), ("linear", (2, 3)),
                 ("linear", (3, 2, 4)), ("linear", (2, 3, 2, 2))]


def check_stencils(gg, kind, ms, X):
    order = ORDERS[kind]
    xg = axes(ms)
    W = gg.linalg.GridInterp(xg, X, order=kind)
    first, w, nout = sr.stencils(xg, X, order)
    assert nout == 0
    assert (W.n, W.N, W.nnz) == (X.shape[0], int(np.prod(ms)), X.shape[0] * order ** len(ms))
    assert np.array_equal(W.first.cpu().numpy().reshape(first.shape), first)
    err = np.max(np.abs(W.w.cpu().numpy().reshape(w.shape) - w))
    assert err <= 1e-14, err


@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("kind,ms", STENCIL_GRIDS)
def test_stencils_match_reference(gg, kind, ms, n):
    check_stencils(gg, kind, ms, sr.domain_points(axes(ms), n, ORDERS[kind], seed=len(ms) + n))


@pytest.mark.parametrize("kind,ms", STENCIL_GRIDS)
def test_stencils_on_nodes_boundaries_and_edges(gg, kind, ms):
    check_stencils(gg, kind, ms, edge_points(axes(ms), ORDERS[kind]))


@pytest.mark.parametrize("kind", ["cubic", "linear"])
def test_point_outside_is_refused_and_output_untouched(gg, kind):
    import torch
    order = ORDERS[kind]
    xg = axes((6, 5))
    X = sr.domain_points(xg, 9, order, seed=1)
    lo, h, m = sr.axis_params(xg[1])
    pad = 1 if order == 4 else 0
    X[3, 1] = lo + pad * h - 1e-9 * h
    X[7, 1] = lo + (m - 1 - pad) * h + 1e-9 * h
    X[8, 0] = np.nan
    first = torch.full((9 * 2,), -7, dtype=torch.int32, device="cuda")
    w = torch.full((9 * 2 * order,), -7.0, dtype=torch.float64, device="cuda")
    st, out = raw_stencils(gg, xg, X, order, first, w)
    assert st == gg.native.GG_ERR_VALUE and out == 3
    assert bool((first == -7).all()) and bool((w == -7.0).all())
    with pytest.raises(ValueError, match="3 point"):
        gg.linalg.GridInterp(xg, X, order=kind)
    # on the edge itself: accepted
    X[3, 1], X[7, 1], X[8, 0] = lo + pad * h, lo + (m - 1 - pad) * h, X[0, 0]
    st, out = raw_stencils(gg, xg, X, order, first, w)
    assert st == 0 and out == 0


def test_refusals_of_the_operator(gg):
    X5 = np.full((3, 5), 0.5)
    with pytest.raises(ValueError, match="256"):
        gg.linalg.GridInterp(axes((4,) * 5, 0, 1), X5, order='cubic')
    with pytest.raises(ValueError, match="256"):
        gg.linalg.GridInterp(axes((2,) * 9, 0, 1), np.full((3, 9), 0.5), order='linear')
    with pytest.raises(ValueError, match="needs 4"):
        gg.linalg.GridInterp(axes((5, 3)), np.full((3, 2), 0.5), order='cubic')
    with pytest.raises(ValueError, match="evenly"):
        gg.linalg.GridInterp([np.array([0.0, 0.1, 0.2, 0.31, 0.4])], np.full((3, 1), 0.2))
    with pytest.raises(ValueError, match="order"):
        gg.linalg.GridInterp(axes((5,)), np.full((3, 1), 0.2), order='quintic')
    with pytest.raises(ValueError):
        gg.linalg.GridInterp(axes((5, 5)), np.full((3, 1), 0.2))


# ------------------------------------------------------------ interp / spread
def crowded(xg, n, order, seed=0):
    """n points inside one cell."""
    rng = np.random.default_rng(seed)
    pad = 1 if order == 4 else 0
    return np.stack([g[pad, 0] + (g[pad + 1, 0] - g[pad, 0]) * rng.uniform(0, 1, n) for g in xg],
                    axis=1)


APPLY_CASES = [("cubic", (8,), 1), ("cubic", (8,), 2), ("cubic", (8,), 65),
               ("cubic", (7, 5), 129), ("cubic", (6, 5, 4), 300), ("cubic", (4, 4, 4, 4), 300),
               ("cubic", (5, 4, 6, 4), 300), ("linear", (2, 3, 2, 2, 3, 2), 77),
               ("cubic", (5, 4), 500), ("linear", (5, 4), 500), ("cubic", (40, 30), 7),
               ("linear", (9,), 33)]

_dense = {}


def dense_case(kind, ms, n, crowd=False):
    key = (kind, ms, n, crowd)
    if key not in _dense:
        order = ORDERS[kind]
        xg = axes(ms)
        X = crowded(xg, n, order) if crowd else sr.domain_points(xg, n, order, seed=n)
        Wd = sr.dense_W(xg, X, order)
        Wd.setflags(write=False)
        _dense[key] = (xg, X, Wd)
    return _dense[key]


def check_apply(gg, kind, xg, X, Wd):
    import torch
    W = gg.linalg.GridInterp(xg, X, order=kind)
    n, N = Wd.shape
    rng = np.random.default_rng(7)
    g, p = rng.standard_normal(N), rng.standard_normal(n)
    t = W.interp(g)
    s = W.spread(p)
    assert t.shape == (n,) and s.shape == (N,)
    assert np.max(np.abs(t - Wd @ g)) <= 1e-12 * np.max(np.abs(g))
    assert np.max(np.abs(s - Wd.T @ p)) <= 1e-12 * np.max(np.abs(p))
    # nodes that no point touches come back exactly 0 (written, not left over)
    empty = ~(Wd != 0).any(axis=0)
    out = torch.full((N,), np.nan, dtype=torch.float64, device="cuda")
    W.spread(torch.from_numpy(p).cuda(), out=out)
    so = out.cpu().numpy()
    assert np.array_equal(so, s)
    assert np.all(so[empty] == 0.0)
    # adjointness
    lhs, rhs = float(t @ p), float(g @ s)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(t) * np.linalg.norm(p))
    return W, g, p, t, s


@pytest.mark.parametrize("kind,ms,n", APPLY_CASES)
def test_interp_and_spread_match_dense_W(gg, kind, ms, n):
    xg, X, Wd = dense_case(kind, ms, n)
    check_apply(gg, kind, xg, X, Wd)


@pytest.mark.parametrize("kind,ms", [("cubic", (9,)), ("cubic", (6, 5)), ("linear", (4, 3))])
def test_spread_long_rows_take_the_split_path(gg, kind, ms):
    xg, X, Wd = dense_case(kind, ms, 5000, crowd=True)
    W = check_apply(gg, kind, xg, X, Wd)[0]
    assert W.long_rows == ORDERS[kind] ** len(ms) and W.max_row == 5000
    assert W.chunks == W.long_rows * 10


def test_mixed_long_and_short_rows(gg):
    xg = axes((9, 7))
    X = np.vstack([crowded(xg, 1500, 4, seed=1), sr.domain_points(xg, 301, 4, seed=2)])
    Wd = sr.dense_W(xg, X, 4)
    W = check_apply(gg, "cubic", xg, X, Wd)[0]
    assert 0 < W.long_rows < W.N and W.max_row <= 6000


def test_spread_is_bitwise_reproducible(gg):
    import torch
    xg = axes((9, 7))
    X = np.vstack([crowded(xg, 1500, 4, seed=1), sr.domain_points(xg, 301, 4, seed=2)])
    p = torch.from_numpy(np.random.default_rng(3).standard_normal(X.shape[0])).cuda()
    W1 = gg.linalg.GridInterp(xg, X)
    a, b = W1.spread(p).clone(), W1.spread(p).clone()
    W2 = gg.linalg.GridInterp(xg, torch.from_numpy(X).cuda())
    c = W2.spread(p)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(W1.rowptr, W2.rowptr) and torch.equal(W1.point, W2.point)
    assert torch.equal(W1.wprod, W2.wprod)


@pytest.mark.parametrize("n", [129, 300])
def test_buffers_off_16_byte_alignment(gg, n):
    import torch
    xg, X, Wd = dense_case("cubic", (7, 5), n)
    W = gg.linalg.GridInterp(xg, X)
    N = W.N
    rng = np.random.default_rng(5)
    g, p = rng.standard_normal(N), rng.standard_normal(n)
    gb = torch.zeros(N + 1, dtype=torch.float64, device="cuda")
    pb = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    tb = torch.full((n + 3,), 9.0, dtype=torch.float64, device="cuda")
    sb = torch.full((N + 3,), 9.0, dtype=torch.float64, device="cuda")
    assert gb[1:].data_ptr() % 16 == 8 and tb[1:n + 1].data_ptr() % 16 == 8
    gb[1:] = torch.from_numpy(g).cuda()
    pb[1:] = torch.from_numpy(p).cuda()
    W.interp(gb[1:], out=tb[1:n + 1])
    W.spread(pb[1:], out=sb[1:N + 1])
    tb, sb = tb.cpu().numpy(), sb.cpu().numpy()
    assert np.max(np.abs(tb[1:n + 1] - Wd @ g)) <= 1e-12 * np.max(np.abs(g))
    assert np.max(np.abs(sb[1:N + 1] - Wd.T @ p)) <= 1e-12 * np.max(np.abs(p))
    assert tb[0] == 9.0 and np.all(tb[n + 1:] == 9.0)
    assert sb[0] == 9.0 and np.all(sb[N + 1:] == 9.0)


# ------------------------------------------------------------------------- CG
# Iteration counts and iterates are compared with the reference CG, so the
# system must be one on which the reference's own trajectory is stable against
# rounding.  With lengthscales of several cells and a small shift it is not:
# run on the CPU with A v and with W (K (W^T v)), the reference differs from
# itself by one to three iterations (41 / 42, 31 / 28, 27 / 30 at shift 0.05,
# l = 0.3) -- W K W^T has rank <= N and a fast-decaying spectrum, the Ritz
# values converge within ten steps and rounding is amplified from there.  At
# shift 1 and lengthscales of about one cell the two orders agree in the count
# and to 5e-11 in x, with the residual 5 % or more off the tolerance on either
# side of the last iteration.
CG_S2 = 1.0
CG_CASES = [((12, 10), 150, [0.06, 0.05]), ((6, 5, 4), 90, [0.08, 0.07, 0.06]),
            ((6, 5, 4), 91, [0.08, 0.07, 0.06])]
_cg = {}


def cg_problem(ms, n, ls):
    """(xg, X, factors, dense A, b): computed once per shape, left unchanged."""
    key = (ms, n)
    if key not in _cg:
        xg = [np.linspace(0, 1, m).reshape(-1, 1) for m in ms]
        X = sr.domain_points(xg, n, 4, seed=n)
        F = sr.rbf_factors(xg, ls)
        A = sr.dense_wkw(sr.dense_W(xg, X, 4), F) + CG_S2 * np.eye(n)
        b = np.random.default_rng(11).standard_normal(n)
        A.setflags(write=False)
        _cg[key] = (xg, X, F, A, b)
    return _cg[key]


def operator(gg, F):
    # KronMatrix lists the slowest factor first; grid axis 0 is the fastest
    return gg.tensors.KronMatrix(F[::-1], sym=True)


@pytest.mark.parametrize("ms,n,ls", CG_CASES)
def test_cg_matches_reference_and_dense(gg, ms, n, ls):
    xg, X, F, A, b = cg_problem(ms, n, ls)
    rtol = 1e-8
    W = gg.linalg.GridInterp(xg, X)
    x, info = gg.linalg.cg(operator(gg, F), b, shift=CG_S2, rtol=rtol, interp=W)
    xr, info_r, it_r, _, _ = sr.cg_coeffs(lambda v: A @ v, b, rtol=rtol)
    assert info == 0 and info_r == 0
    assert gg.linalg.cg.last.iters == it_r
    assert x.shape == b.shape and rel(x, xr) <= 1e-9
    lam = np.linalg.eigvalsh(A)
    assert rel(x, np.linalg.solve(A, b)) <= lam[-1] / lam[0] * rtol


def test_cg_ill_conditioned_against_dense_solve(gg):
    """sigma^2 = 0.05 and lengthscales of several cells (kappa about 1300): no
    trajectory comparison (see above), the converged solve against the dense
    one within kappa * rtol."""
    ms, n, ls, rtol = (12, 10), 150, [0.3, 0.25], 1e-10
    xg = [np.linspace(0, 1, m).reshape(-1, 1) for m in ms]
    X = sr.domain_points(xg, n, 4, seed=n)
    F = sr.rbf_factors(xg, ls)
    A = sr.dense_wkw(sr.dense_W(xg, X, 4), F) + S2 * np.eye(n)
    b = np.random.default_rng(11).standard_normal(n)
    W = gg.linalg.GridInterp(xg, X)
    x, info = gg.linalg.cg(operator(gg, F), b, shift=S2, rtol=rtol, interp=W)
    lam = np.linalg.eigvalsh(A)
    assert info == 0 and lam[-1] / lam[0] > 1000
    assert np.linalg.norm(b - A @ x) <= 10 * rtol * np.linalg.norm(b)
    assert rel(x, np.linalg.solve(A, b)) <= lam[-1] / lam[0] * rtol


def test_cg_single_point(gg):
    xg = [np.linspace(0, 1, 5).reshape(-1, 1)]
    X = np.array([[0.43]])
    F = sr.rbf_factors(xg, [0.3])
    a = float(sr.dense_wkw(sr.dense_W(xg, X, 4), F)[0, 0]) + S2
    W = gg.linalg.GridInterp(xg, X)
    x, info = gg.linalg.cg(operator(gg, F), np.array([2.0]), shift=S2, rtol=1e-12, interp=W)
    assert info == 0 and gg.linalg.cg.last.iters == 1
    assert abs(x[0] - 2.0 / a) <= 1e-13 * abs(2.0 / a)


def test_cg_restart_and_polling_change_no_bit(gg):
    import torch
    xg, X, F, A, b = cg_problem(*CG_CASES[0])
    W = gg.linalg.GridInterp(xg, X)
    K = operator(gg, F)
    bd = torch.from_numpy(b).cuda()
    s = gg.linalg.SKICG(K, W, CG_S2, max_steps=8)
    x1 = s.solve(bd, rtol=1e-9, check_every=0)[0].clone()
    it1 = s.status()[0]
    a1, b1 = s.coefficients()
    other = s.solve(bd * 2.0 + 1.0, rtol=1e-6)[0].clone()   # another b in between
    assert not torch.equal(other, x1)
    x2, it2, conv2, res2, tol2 = s.solve(bd, rtol=1e-9, check_every=1)
    a2, b2 = s.coefficients()
    assert conv2 and it2 == it1 and res2 < tol2
    assert torch.equal(x1, x2)
    assert a1.size == 8 and np.array_equal(a1, a2) and np.array_equal(b1, b2)
    x3 = gg.linalg.SKICG(K, W, CG_S2).solve(bd, rtol=1e-9, check_every=3)[0]
    assert torch.equal(x1, x3)
    # once converged, more iterations change nothing
    s.iterate(5)
    assert s.status()[0] == it1 and torch.equal(s.x, x1)
    # the coefficients are the reference CG's
    _, _, _, ar, br = sr.cg_coeffs(lambda v: A @ v, b, rtol=1e-9)
    assert np.max(np.abs(a1 / ar[:8] - 1)) < 1e-9 and np.max(np.abs(b1 / br[:8] - 1)) < 1e-8


def test_cg_refusals(gg):
    import torch
    native = gg.native
    L = native.lib()
    xg, X, F, A, b = cg_problem(*CG_CASES[0])
    W = gg.linalg.GridInterp(xg, X)
    K = operator(gg, F)
    s = gg.linalg.SKICG(K, W, CG_S2)
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros(150, dtype=torch.float64, device="cuda")
    null = ctypes.c_void_p()
    sp = native.stream_ptr()
    E = native.GG_ERR_VALUE
    we = ctypes.c_int64()
    h = ctypes.c_void_p()
    assert L.gg_skicg_work_elems(null, W.h, ctypes.byref(we)) == E
    assert L.gg_skicg_work_elems(K._device().h, null, ctypes.byref(we)) == E
    assert L.gg_skicg_create(K._device().h, W.h, CG_S2, null, 4, ctypes.byref(h)) == E
    assert L.gg_skicg_create(K._device().h, W.h, 0.0, native.dptr(s.work), 4,
                             ctypes.byref(h)) == E
    assert L.gg_skicg_create(K._device().h, W.h, CG_S2, native.dptr(s.work), -1,
                             ctypes.byref(h)) == E
    assert L.gg_skicg_iterate(s.h, 3, 0, sp) == E          # not started
    assert L.gg_skicg_start(s.h, null, native.dptr(xd), 1e-8, 0.0, sp) == E
    assert L.gg_skicg_start(s.h, native.dptr(bd), null, 1e-8, 0.0, sp) == E
    for rtol, atol in ((-1e-8, 0.0), (1e-8, -1.0), (float("nan"), 0.0), (1e-8, float("nan"))):
        assert L.gg_skicg_start(s.h, native.dptr(bd), native.dptr(xd), rtol, atol, sp) == E
    assert L.gg_ski_interp(null, native.dptr(bd), native.dptr(xd), sp) == E
    assert L.gg_ski_spread(W.h, null, native.dptr(xd), sp) == E
    torch.cuda.synchronize()
    assert bool((xd == 0).all())
    it, conv, res, tol = s.status()
    assert it == 0 and not conv
    mask = np.ones(W.N, dtype=bool)
    for kw in (dict(mask=mask), dict(noise=np.ones(W.N)), dict(comm=True), dict(basis='grid'),
               dict(precond='kron')):
        with pytest.raises(ValueError, match="interp="):
            gg.linalg.cg(K, b, shift=CG_S2, interp=W, **kw)
    with pytest.raises(ValueError, match="interp="):
        gg.linalg.slq_logdet(K, CG_S2, interp=W, mask=mask)
    with pytest.raises(ValueError):
        gg.linalg.cg(K, np.ones(W.N), shift=CG_S2, interp=W)   # b has n entries, not N
    Kbad = operator(gg, sr.rbf_factors([np.linspace(0, 1, 5)] * 2, [0.3, 0.3]))
    with pytest.raises(ValueError):
        gg.linalg.SKICG(Kbad, W, CG_S2)


# ------------------------------------------------------------------------ SLQ
_slq = {}


def slq_problem():
    if not _slq:
        ms, n = (9, 8), 60
        xg = [np.linspace(0, 1, m).reshape(-1, 1) for m in ms]
        X = sr.domain_points(xg, n, 4, seed=2)
        F = sr.rbf_factors(xg, [0.3, 0.25])
        A = sr.dense_wkw(sr.dense_W(xg, X, 4), F) + S2 * np.eye(n)
        lam, Q = np.linalg.eigh(A)
        _slq["p"] = (xg, X, F, A, (Q * np.log(lam)) @ Q.T, float(np.sum(np.log(lam))))
    return _slq["p"]


def test_slq_per_probe(gg):
    xg, X, F, A, logA, exact = slq_problem()
    W = gg.linalg.GridInterp(xg, X)
    mean, ests = gg.linalg.slq_logdet(operator(gg, F), S2, probes=16, steps=40, seed=0, interp=W)
    assert ests.shape == (16,) and abs(mean - ests.mean()) < 1e-12 * abs(mean)
    for j in range(16):
        z = probe_signs(0, j, 60)
        ref = sr.slq_probe(A, z, 40)
        dense = float(z @ logA @ z)
        e_ref, e_dense = abs(ests[j] - ref) / abs(ref), abs(ests[j] - dense) / abs(dense)
        print("probe %d: vs reference %.2e, vs dense %.2e" % (j, e_ref, e_dense))
        assert e_ref <= 1e-9
        # the reference alone, on the CPU: its largest relative error against
        # the dense z^T log(A) z over these 16 probes is 5.6e-14 (40 steps on 60
        # points: the quadrature has converged, what is left is rounding at a
        # condition number of 547); ten times that is allowed
        assert e_dense <= 5.6e-13


def test_slq_mean_within_probe_error(gg):
    xg, X, F, A, logA, exact = slq_problem()
    W = gg.linalg.GridInterp(xg, X)
    # seed 0: the reference alone lands 0.50 standard errors from the dense
    # slogdet on the CPU (-136.33 against -135.14)
    mean, ests = gg.linalg.slq_logdet(operator(gg, F), S2, probes=16, steps=40, seed=0, interp=W)
    se = ests.std(ddof=1) / np.sqrt(16)
    assert abs(mean - exact) <= 4 * se


# ---------------------------------------------------------------------- model
_model = {}


def model_problem():
    if not _model:
        ms, n, ls = (10, 9), 120, [0.3, 0.25]
        xg = [np.linspace(0, 1, m).reshape(-1, 1) for m in ms]
        X = sr.domain_points(xg, n, 4, seed=4)
        F = sr.rbf_factors(xg, ls)
        Wd = sr.dense_W(xg, X, 4)
        A = sr.dense_wkw(Wd, F) + S2 * np.eye(n)
        rng = np.random.default_rng(12)
        y = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, 1]) + 0.2 * rng.standard_normal(n)
        Xs = rng.uniform(0.2, 0.8, (5, 2))
        _model["p"] = (xg, X, F, Wd, A, y, Xs, ls)
    return _model["p"]


def grid_kernel(gg, ls):
    return gg.kern.GridKernel([gg.kern.RBF(1, lengthscale=l) for l in ls])


def ski_model(gg, **kw):
    xg, X, F, Wd, A, y, Xs, ls = model_problem()
    return gg.models.GPSKIModel(X, y.reshape(-1, 1), grid_kernel(gg, ls), xg, noise_var=S2, **kw)


def test_model_exact_matches_dense(gg):
    import oracle
    xg, X, F, Wd, A, y, Xs, ls = model_problem()
    m = ski_model(gg, logdet='exact')
    lml, alpha, logdet = sr.dense_lml(A, y)
    assert abs(lml_of(m) - lml) <= 1e-8 * abs(lml)
    assert rel(m._alpha.cpu().numpy(), alpha) <= 1e-8
    mean, var = m.predict(Xs)
    # exact cross-covariance to the nodes for the mean, W (Kronecker row) for
    # the variance
    Kd = sr.dense_K(F)
    cross = np.ones((Xs.shape[0], 1))
    for f in range(2):
        kf = oracle.cov_1d("RBF", Xs[:, f], xg[f][:, 0], 1.0, ls[f])
        cross = (kf[:, :, None] * cross[:, None, :]).reshape(Xs.shape[0], -1)
    mean_ref = cross @ (Wd.T @ alpha)
    ks = Wd @ cross.T
    var_ref = 1.0 - np.einsum("ij,ij->j", ks, np.linalg.solve(A, ks)) + S2
    assert mean.shape == (5, 1) and var.shape == (5, 1)
    assert rel(mean, mean_ref) <= 1e-8 and rel(var, var_ref) <= 1e-8
    pg = m.predict_grid()
    assert pg.shape == (90, 1) and rel(pg, Kd @ (Wd.T @ alpha)) <= 1e-8
    K = m._operator()
    assert np.array_equal(pg[:, 0], K.matvec_device(m.W.spread(m._alpha)).cpu().numpy())


def test_model_slq_and_cg(gg):
    xg, X, F, Wd, A, y, Xs, ls = model_problem()
    m = ski_model(gg, logdet='slq', slq_probes=16, slq_steps=50, seed=0, cg_rtol=1e-12)
    lml, alpha, logdet = sr.dense_lml(A, y)
    got = lml_of(m)
    assert m.cg_iters > 0 and rel(m._alpha.cpu().numpy(), alpha) <= 1e-8
    se = m.slq_estimates.std(ddof=1) / 4.0
    # the LML's only inexact term is -1/2 log det
    assert abs(got - lml) <= 0.5 * 4 * se
    assert lml_of(ski_model(gg, logdet='slq', slq_probes=16, seed=0, cg_rtol=1e-12)) == got   # deterministic
    mean, var = m.predict(Xs[:2])
    me, ve = ski_model(gg, logdet='exact').predict(Xs[:2])
    assert rel(mean, me) <= 1e-8 and rel(var, ve) <= 1e-8
    with pytest.raises(ValueError, match="exact_max"):
        ski_model(gg, logdet='exact', exact_max=100)
    with pytest.raises(ValueError):
        ski_model(gg, logdet='lanczos')


def test_model_on_nodes_equals_masked_grid_model(gg):
    xg, _, F, _, _, _, _, ls = model_problem()
    m0, m1 = 10, 9
    rng = np.random.default_rng(13)
    interior = [(i, j) for i in range(1, m0 - 1) for j in range(1, m1 - 1)]
    pick = rng.choice(len(interior), 30, replace=False)
    nodes = np.array([interior[k][0] + m0 * interior[k][1] for k in pick])
    X = np.array([[xg[0][interior[k][0], 0], xg[1][interior[k][1], 0]] for k in pick])
    y = rng.standard_normal(30)
    mask = np.zeros(m0 * m1, dtype=bool)
    mask[nodes] = True
    Y = np.zeros((m0 * m1, 1))
    Y[nodes, 0] = y
    ms = gg.models.GPSKIModel(X, y.reshape(-1, 1), grid_kernel(gg, ls), xg, noise_var=S2,
                              logdet='exact')
    mg = gg.models.GPGridModel(xg, Y, grid_kernel(gg, ls), noise_var=S2, solver='cg', mask=mask,
                               logdet='exact', cg_rtol=1e-12)
    ls_, lg = lml_of(ms), lml_of(mg)
    assert abs(ls_ - lg) <= 1e-8 * abs(lg)
    ag = mg._alpha.cpu().numpy()
    assert rel(ms._alpha.cpu().numpy(), ag[nodes]) <= 1e-8
    mc = gg.models.GPSKIModel(X, y.reshape(-1, 1), grid_kernel(gg, ls), xg, noise_var=S2,
                              cg_rtol=1e-12)
    mc.fit()
    assert rel(mc._alpha.cpu().numpy(), ag[nodes]) <= 1e-8


def test_model_exact_follows_a_kernel_parameter_change(gg):
    """Only a lengthscale changes (what every finite-difference step does):
    LML and alpha are those of the dense reference at the new parameters, and
    the finite-difference gradient sees every kernel parameter."""
    xg, X, F, Wd, A, y, Xs, ls = model_problem()
    m = ski_model(gg, logdet='exact')
    l0 = lml_of(m)
    p = m.parameters
    names = [n for k in m.kern.kern_list for n in k.parameter_list]
    i = 1 + names.index('lengthscale')          # the first kernel's lengthscale
    assert p[i] == ls[0]
    p[i] = 0.2
    m.parameters = p
    A2 = sr.dense_wkw(Wd, sr.rbf_factors(xg, [0.2, ls[1]])) + S2 * np.eye(len(y))
    lml2, alpha2, _ = sr.dense_lml(A2, y)
    assert abs(lml2 - l0) > 1e-3 * abs(l0)      # the change is visible at all
    assert abs(lml_of(m) - lml2) <= 1e-8 * abs(lml2)
    assert rel(m._alpha.cpu().numpy(), alpha2) <= 1e-8
    # back again: the first factorisation's values, not a stale cache
    p[i] = ls[0]
    m.parameters = p
    assert abs(lml_of(m) - l0) <= 1e-12 * abs(l0)
    ll, grad = m.log_likelihood(return_gradient=True)
    free = m._free_indicies
    assert free.sum() >= 4 and np.all(np.abs(grad[free]) > 1e-6)
    # the same through the CG / SLQ path
    mc = ski_model(gg, logdet='slq', cg_rtol=1e-12)
    mc.fit()
    p = mc.parameters
    p[i] = 0.2
    mc.parameters = p
    mc.fit()
    assert rel(mc._alpha.cpu().numpy(), alpha2) <= 1e-8


def test_model_optimize_does_not_lower_lml(gg):
    m = ski_model(gg, logdet='exact')
    before = lml_of(m)
    m.optimize(max_iters=3)
    assert lml_of(m) >= before


def test_model_exports(gg):
    import gp_grief.models
    import gp_grief.linalg
    assert gp_grief.models.GPSKIModel is gg.models.GPSKIModel
    assert gp_grief.linalg.GridInterp is gg.linalg.GridInterp
    assert gp_grief.linalg.SKICG is gg.linalg.SKICG
