"""linalg: the reference's helpers plus the device Krylov solvers.

Host utilities with the reference's behaviour (gp_grief/linalg.py):
  solve_schur, solve_chol :10-50   (dense helpers of the reference's GPRegressionModel)
  solver_counter          :53-71   (iteration callback / best-parameter backup)
  log_kron                :74-89
  uniquetol               :92-104
  LogexpTransformation    :107-125
Device solvers (no reference implementation exists):
  cg            -- scipy.sparse.linalg.cg's recurrence on (K + shift I), every
                   vector op and scalar on the MI355X (gg_cg_*).
  MaskedKronCG  -- the same CG on (W K W + shift I) x = W b, W = diag(mask): the
                   grid with missing observations (gg_cgm_*; cg(mask=...)),
                   optionally preconditioned by the Kronecker eigenpairs.
  slq_logdet    -- stochastic Lanczos quadrature, Lanczos on the device
                   (gg_lanczos_probe); the k x k tridiagonal eigensolve of the
                   quadrature is host-side (k <= a few hundred).  With mask=:
                   Lanczos on (W K W + shift I) from probes zeroed at the
                   missing points (gg_lanczos_probe_masked), the estimator of
                   log det(K_oo + shift I) on an incomplete grid.
  trace_grad    -- Hutchinson estimates of tr(A^-1) and tr(A^-1 dK) for the
                   marginal likelihood's gradient, from the same masked probes
                   as slq_logdet: one resident CG solve per probe.
  GridPosteriorSampler -- joint draws of the latent field's posterior on the
                   grid (gg_sample.hip): one Kronecker matvec per draw in the
                   eigenbasis on a complete grid, Matheron's rule (one CG
                   solve per draw) with a mask or the CG solver.
Every one of the masked solvers takes noise=: per-point noise variances, the
system W K W + diag(noise) (gg_cgm_set_noise, gg_lanczos_probe_masked_noise,
gg_sample_residual_noise).
  LaplaceNewton -- the mode of a Laplace approximation with a Poisson or
                   binomial likelihood on the grid: Newton steps whose solve is
                   the weighted masked CG with noise 1 / w, the likelihood as
                   one fused streaming pass (gg_lik_newton).
"""
import ctypes
import logging
import sys

import numpy as np

logger = logging.getLogger(__name__)


class solver_counter:
    """Iteration counter usable as a solver / optimiser callback (linalg.py:53-71)."""

    def __init__(self, disp=True):
        self._disp = disp
        self.niter = 0
        self.backup = None

    def __call__(self, rk=None, msg='', store=None):
        self.niter += 1
        if self._disp:
            logger.info('iter %3i. %s' % (self.niter, msg))
            sys.stdout.flush()
        if store is not None:
            self.backup = store


def solve_schur(Q, t, x, shift=0.0):
    """(K + shift I) y = x for a dense K = Q diag(t) Q^T (linalg.py:10-32);
    the Kronecker form is KronMatrix.solve_schur (device).  Dense host helper
    of the reference's GPRegressionModel, kept for the import surface."""
    if x.shape != (Q.shape[0], 1):
        raise ValueError('x is the wrong shape, must be (%d,1)' % Q.shape[0])
    y = np.dot(Q.T, x)
    y = y / np.reshape(t + shift, y.shape)
    return np.dot(Q, y)


def solve_chol(U, x):
    """y = U \\ (U^T \\ x) for an upper Cholesky factor U (linalg.py:35-50);
    dense host helper (the models use the device gg_potrs)."""
    from scipy.linalg import solve_triangular
    if x.shape != (U.shape[0], 1):
        raise ValueError('x is the wrong shape, must be (%d,1)' % U.shape[0])
    y = solve_triangular(U, x, trans=1, lower=False, check_finite=False)
    return solve_triangular(U, y, trans=0, lower=False, check_finite=False)


def log_kron(a, b, a_logged=False, b_logged=False):
    """log(kron(a, b)) for 1-D a, b without forming the product (linalg.py:74-89)."""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.ndim == b.ndim == 1, "currenly only working for 1d arrays"
    if not a_logged:
        a = np.log(a)
    if not b_logged:
        b = np.log(b)
    return (a.reshape((-1, 1)) + b.reshape((1, -1))).reshape(-1)


def uniquetol(x, tol=1e-6, relative=False):
    assert x.ndim == 1
    if relative:
        tol = np.float64(tol) * np.ptp(x)
    return x[~(np.triu(np.abs(x[:, None] - x) <= tol, 1)).any(0)]


class LogexpTransformation:
    """Softplus transform for positive parameters (linalg.py:107-125)."""
    _lim_val = 36.
    _log_lim_val = np.log(np.finfo(np.float64).max)

    def inverse_transform(self, x):
        return np.where(x > self._lim_val, x,
                        np.log1p(np.exp(np.clip(x, -self._log_lim_val, self._lim_val))))

    def transform(self, f):
        return np.where(f > self._lim_val, f, np.log(np.expm1(f)))

    def transform_grad(self, f, grad_f):
        return grad_f * np.where(f > self._lim_val, 1., -np.expm1(-f))


# ---------------------------------------------------------------- device CG
class CGResult(object):
    def __init__(self, x, info, iters, resid, tol):
        self.x, self.info, self.iters, self.resid, self.tol = x, info, iters, resid, tol


class KronCG(object):
    """Resident CG state for (K + shift I) x = b on one MI355X.

    The operator and all CG vectors (x, r, three p buffers, q + one matvec
    scratch) live in HBM; no host synchronisation inside an iteration.

    recurrence="fused" (default for d >= 2): an iteration is the d mode
    products plus one scalar kernel -- r -= alpha q, p = r + beta p (and r.r)
    ride on the first mode product, the x update on the second / third, p.q /
    r.q / q.q on the last; beta comes from |r - alpha q|^2 expanded
    (gg_vec.hip).  xdefer (fusion layouts 0 / 1; default 2): x is updated in
    deferred pairs of steps, two steps in one pass -- 2: each pair applied to
    half of x in each of the next two iterations (every side launch carries one
    pass), 1: the whole pair every other iteration, 0: every iteration (True =
    2, False = 0).  rq (layout 0; default 1): beta's r.q from the conjugacy
    identity p.q - beta p.q_prev (the prologue sums p.q_prev; the last
    epilogue does not read r), 0: r.q read in the epilogue.
    recurrence="textbook":
    scipy's operation order, with a separate x / r update pass.  Both leave
    iterate() in the textbook state.
    """

    def __init__(self, K, shift, recurrence="fused", fusion=None, xdefer=None, rq=None,
                 basis=None):
        from . import device as dev
        from . import native
        self.K = K
        self.shift = float(shift)
        self._dk = K._device()
        L = native.lib()
        we = ctypes.c_int64()
        native.check(L.gg_cg_work_elems(self._dk.h, ctypes.byref(we)))
        self.work = dev.empty(we.value)
        h = ctypes.c_void_p()
        native.check(L.gg_cg_create(self._dk.h, self.shift, native.dptr(self.work),
                                    ctypes.byref(h)), "gg_cg_create")
        self.h = h
        if recurrence not in ("fused", "textbook"):
            raise ValueError("recurrence must be 'fused' or 'textbook'")
        if recurrence == "textbook":
            native.check(L.gg_cg_set_recurrence(h, 0), "gg_cg_set_recurrence")
        f = ctypes.c_int()
        native.check(L.gg_cg_get_recurrence(h, ctypes.byref(f)))
        self.recurrence = "fused" if f.value else "textbook"
        if fusion is not None:
            native.check(L.gg_cg_set_fusion(h, int(fusion)), "gg_cg_set_fusion")
        native.check(L.gg_cg_get_fusion(h, ctypes.byref(f)))
        self.fusion = f.value
        if xdefer is not None:
            # True: the library default (2, balanced); an int selects 0 / 1 / 2
            mode = (2 if xdefer else 0) if isinstance(xdefer, bool) else int(xdefer)
            native.check(L.gg_cg_set_xdefer(h, mode), "gg_cg_set_xdefer")
        native.check(L.gg_cg_get_xdefer(h, ctypes.byref(f)))
        self.xdefer = f.value
        if rq is not None:
            native.check(L.gg_cg_set_rq(h, int(bool(rq))), "gg_cg_set_rq")
        native.check(L.gg_cg_get_rq(h, ctypes.byref(f)))
        self.rq = f.value
        if basis is not None:
            # "block": the parity-block basis (default where it exists), "grid": off
            if basis not in ("block", "grid"):
                raise ValueError("basis must be 'block' or 'grid'")
            native.check(L.gg_cg_set_basis(h, int(basis == "block")), "gg_cg_set_basis")
        native.check(L.gg_cg_get_basis(h, ctypes.byref(f)))
        self.basis = "block" if f.value else "grid"
        # the block basis's x window (x_defer mode 3, GG_CG_XWIN; 0: not in effect)
        native.check(L.gg_cg_get_xwin(h, ctypes.byref(f)))
        self.xwin = f.value
        # r derived from the window's directions (no r in memory; GG_CG_RDERIVE)
        native.check(L.gg_cg_get_rderive(h, ctypes.byref(f)))
        self.rderive = bool(f.value)
        self.n = int(K.shape[0])
        self.x = None

    def start(self, b_dev, rtol=1e-5, atol=0.0, x_out=None):
        from . import device as dev
        from . import native
        if b_dev.numel() != self.n:
            raise ValueError("b must have %d entries" % self.n)
        self.b = dev.ensure_aligned(b_dev.reshape(-1))
        self.x = dev.empty(self.n) if x_out is None else x_out
        native.check(native.lib().gg_cg_start(self.h, native.dptr(self.b), native.dptr(self.x),
                                              float(rtol), float(atol), native.stream_ptr()),
                     "gg_cg_start")

    def iterate(self, n_iter, check_every=0, close=True):
        """n_iter iterations; close=False leaves the fused recurrence open
        (its last r update and deferred x steps pending, continued by the next
        call) -- close() (or a later iterate(close=True)) restores the
        textbook state before x or the counts are read."""
        from . import native
        n_iter = min(int(n_iter), 2 ** 31 - 1)
        name = "gg_cg_iterate" if close else "gg_cg_iterate_open"
        native.check(getattr(native.lib(), name)(self.h, n_iter, min(int(check_every), n_iter),
                                                 native.stream_ptr()), name)

    def close(self):
        """Apply the pending r update and deferred x steps (gg_cg_close)."""
        from . import native
        native.check(native.lib().gg_cg_close(self.h, native.stream_ptr()), "gg_cg_close")

    def status(self):
        from . import native
        it, conv = ctypes.c_int(), ctypes.c_int()
        res, tol = ctypes.c_double(), ctypes.c_double()
        native.check(native.lib().gg_cg_status(self.h, ctypes.byref(it), ctypes.byref(conv),
                                               ctypes.byref(res), ctypes.byref(tol),
                                               native.stream_ptr()))
        return it.value, bool(conv.value), res.value, tol.value

    def calibrate(self, reps=5):
        """The fused prologue's six streams alone over this handle's buffers
        (gg_cg_calibrate; after start, before the iterations): (ms per pass,
        [r, p_old, p_new, q addresses mod 2 MiB])."""
        from . import native
        ms = ctypes.c_double()
        off = (ctypes.c_int64 * 4)()
        native.check(native.lib().gg_cg_calibrate(self.h, int(reps), ctypes.byref(ms), off,
                                                  native.stream_ptr()), "gg_cg_calibrate")
        return ms.value, [int(v) for v in off]

    def cancels(self):
        """Cancelled betas since start (gg_cg_cancels; synchronising)."""
        from . import native
        v = ctypes.c_int()
        native.check(native.lib().gg_cg_cancels(self.h, ctypes.byref(v), native.stream_ptr()),
                     "gg_cg_cancels")
        return v.value

    def profile(self, enable=True):
        """Record HIP events around every mode product of later iterations."""
        from . import native
        native.check(native.lib().gg_cg_profile(self.h, int(bool(enable))), "gg_cg_profile")

    def launches(self):
        """Kernel launches per matvec (d; d - 1 in the block basis)."""
        from . import native
        v = ctypes.c_int()
        native.check(native.lib().gg_cg_launches(self.h, ctypes.byref(v)))
        return v.value

    def profile_read(self):
        """(profiled matvecs, [summed ms per launch position]) (synchronising)."""
        from . import native
        d = self.launches()
        nm = ctypes.c_int()
        buf = (ctypes.c_double * 16)()
        native.check(native.lib().gg_cg_profile_read(self.h, ctypes.byref(nm), buf, 16),
                     "gg_cg_profile_read")
        return nm.value, [buf[k] for k in range(d)]

    def __del__(self):
        try:
            from . import native
            if getattr(self, "h", None) is not None and self.h.value:
                native.load().gg_cg_destroy(self.h)
        except Exception:
            pass


def _mask_to_device(mask, n):
    """(uint8 device tensor of n entries, observed count) from a bool / uint8
    mask, numpy or device; nonzero = observed."""
    from . import device as dev
    t = dev.torch()
    if isinstance(mask, t.Tensor):
        m = mask.detach().reshape(-1)
    else:
        m = t.from_numpy(np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0))
    if m.numel() != n:
        raise ValueError("mask must have %d entries, not %d" % (n, m.numel()))
    m = (m != 0).to(device=dev.device(), dtype=t.uint8).contiguous()
    n_obs = int(m.sum().item())
    if n_obs == 0:
        raise ValueError("mask has no observed point")
    return m, n_obs


def _is_device_doubles(x):
    """A contiguous float64 device tensor: usable where it lies."""
    from . import device as dev
    t = dev.torch()
    return isinstance(x, t.Tensor) and x.is_cuda and x.dtype == t.float64 and x.is_contiguous()


def _noise_to_device(noise, n, mask_dev=None, check=True):
    """(n float64 device doubles, geometric mean over the observed points) of a
    per-point noise vector, numpy or device; a contiguous float64 device
    tensor is used where it lies (any 8-byte alignment).  Refuses a value that
    is not positive and finite at an observed point (one device reduction);
    at the missing points it is not looked at (NaN allowed).  check=False: no
    reduction and no mean (None)."""
    from . import device as dev
    t = dev.torch()
    nd = noise.detach().reshape(-1) if _is_device_doubles(noise) else dev.to_device(noise)
    if nd.numel() != n:
        raise ValueError("noise must have %d entries, not %d" % (n, nd.numel()))
    if not check:
        return nd, None
    seen = nd if mask_dev is None else t.where(mask_dev != 0, nd, t.ones_like(nd))
    if not bool(((seen > 0) & t.isfinite(seen)).all().item()):
        raise ValueError("noise must be positive and finite at every observed point")
    count = n if mask_dev is None else int((mask_dev != 0).sum().item())
    return nd, float(t.exp(t.log(seen).sum() / count).item())


def _all_ones_mask(n):
    from . import device as dev
    t = dev.torch()
    return t.ones(n, dtype=t.uint8, device=dev.device())


class MaskedKronCG(object):
    """Resident CG state for (W K W + shift I) x = W b, W = diag(mask), on one
    MI355X (gg_cgm_*): the grid GP with missing observations.  x is zero at the
    missing points and solves (K_oo + shift I) x_o = b_o on the observed ones;
    b at the missing points is ignored (it may be NaN).  Runs in the grid basis
    (W is not diagonal in the parity-block basis) with the textbook
    recurrence; start / iterate / status as KronCG.

    precond='kron': z = W Q diag(1 / (lam + shift)) Q^T r from the per-factor
    eigenpairs K.schur() -- the exact inverse on the full grid, two more Kron
    matvecs per iteration (fewer iterations at low missing fractions).

    noise (N positive doubles, numpy or device; a contiguous float64 device
    tensor is used where it lies): per-point noise variances, the system (W K W
    + D) x = W b with D = diag(noise) (gg_cgm_set_noise) -- x solves (K_oo +
    D_oo) x_o = b_o.  noise at the missing points is ignored (NaN allowed);
    mask=None then means every point observed.  The diagonal has one source of
    truth: shift must be 0 or None with noise= (ValueError otherwise).
    precond_shift (noise= only; a positive number): the scalar stand-in for
    the noise in the 'kron' preconditioner, 1 / (lam + precond_shift) -- it is
    no part of the system.  None takes the geometric mean of noise over the
    observed points, a heuristic whose effect on the iteration count has not
    been measured.  self.shift holds the stand-in (it is what gg_cgm_create
    is given).
    """

    def __init__(self, K, shift, mask, precond=None, noise=None, precond_shift=None):
        from . import device as dev
        from . import native
        if precond not in (None, 'kron'):
            raise ValueError("precond must be None or 'kron'")
        self.K = K
        self.n = int(K.shape[0])
        if noise is not None and mask is None:
            mask = _all_ones_mask(self.n)
        self.mask, self.n_observed = _mask_to_device(mask, self.n)
        self.noise = None
        if noise is not None:
            if shift is not None and float(shift) != 0.0:
                raise ValueError("noise= is the whole diagonal: shift must be 0 (or None); the "
                                 "preconditioner's stand-in is precond_shift=")
            self.noise, gmean = _noise_to_device(noise, self.n, self.mask)
            shift = gmean if precond_shift is None else float(precond_shift)
            if not shift > 0.0:
                raise ValueError("precond_shift must be positive")
        elif precond_shift is not None:
            raise ValueError("precond_shift= needs noise=")
        self.shift = float(shift)
        self._dk = K._device()
        L = native.lib()
        we = ctypes.c_int64()
        native.check(L.gg_cgm_work_elems(self._dk.h, ctypes.byref(we)), "gg_cgm_work_elems")
        self.work = dev.empty(we.value)
        h = ctypes.c_void_p()
        native.check(L.gg_cgm_create(self._dk.h, self.shift,
                                     ctypes.c_void_p(self.mask.data_ptr()),
                                     native.dptr(self.work), ctypes.byref(h)), "gg_cgm_create")
        self.h = h
        if self.noise is not None:
            native.check(L.gg_cgm_set_noise(h, native.dptr(self.noise)), "gg_cgm_set_noise")
        self.precond = precond
        if precond == 'kron':
            Q, T = K.schur()
            lam = [np.asarray(e, dtype=np.float64).reshape(-1) for e in T.diag().K]
            self._Q, self._qd = Q, Q._device()
            self._lam = dev.to_device(np.concatenate(lam))
            native.check(L.gg_cgm_set_precond(h, self._qd.h, native.dptr(self._lam)),
                         "gg_cgm_set_precond")
        self.x = None

    def start(self, b_dev, rtol=1e-5, atol=0.0, x_out=None):
        from . import device as dev
        from . import native
        if b_dev.numel() != self.n:
            raise ValueError("b must have %d entries" % self.n)
        self.b = b_dev.reshape(-1)
        self.x = dev.empty(self.n) if x_out is None else x_out
        native.check(native.lib().gg_cgm_start(self.h, native.dptr(self.b), native.dptr(self.x),
                                               float(rtol), float(atol), native.stream_ptr()),
                     "gg_cgm_start")

    def iterate(self, n_iter, check_every=0):
        from . import native
        n_iter = min(int(n_iter), 2 ** 31 - 1)
        native.check(native.lib().gg_cgm_iterate(self.h, n_iter, min(int(check_every), n_iter),
                                                 native.stream_ptr()), "gg_cgm_iterate")

    def status(self):
        from . import native
        it, conv = ctypes.c_int(), ctypes.c_int()
        res, tol = ctypes.c_double(), ctypes.c_double()
        native.check(native.lib().gg_cgm_status(self.h, ctypes.byref(it), ctypes.byref(conv),
                                                ctypes.byref(res), ctypes.byref(tol),
                                                native.stream_ptr()), "gg_cgm_status")
        return it.value, bool(conv.value), res.value, tol.value

    def solve(self, b_dev, rtol=1e-5, atol=0.0, maxiter=None, check_every=None, x_out=None):
        """start + iterate to convergence: (x, iterations, converged, |r|, tol)."""
        if maxiter is None:
            maxiter = self.n * 10
        if check_every is None:
            check_every = 10 if self.n >= 1 << 20 else 50
        self.start(b_dev, rtol, atol, x_out=x_out)
        self.iterate(maxiter, check_every=check_every)
        return (self.x,) + self.status()

    def __del__(self):
        try:
            from . import native
            if getattr(self, "h", None) is not None and self.h.value:
                native.load().gg_cgm_destroy(self.h)
        except Exception:
            pass


def _even_axis(g, order, f):
    """(lo, h, m) of grid axis f, refused unless evenly spaced to 1e-9 h."""
    a = np.asarray(g, dtype=np.float64).reshape(-1)
    m = int(a.size)
    if m < order:
        raise ValueError("grid axis %d has %d nodes, %s interpolation needs %d"
                         % (f, m, 'cubic' if order == 4 else 'linear', order))
    h = (a[-1] - a[0]) / (m - 1)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("grid axis %d must be increasing and finite" % f)
    if np.max(np.abs(a - (a[0] + h * np.arange(m)))) > 1e-9 * h:
        raise ValueError("grid axis %d is not evenly spaced (structured kernel interpolation "
                         "needs evenly spaced axes)" % f)
    return float(a[0]), float(h), m


class GridInterp(object):
    """The sparse interpolation operator W (n x N) of structured kernel
    interpolation (KISS-GP, Wilson & Nickisch 2015) between the nodes of the
    grid xg (a list of d evenly spaced axes, input dimension 0 fastest like Y
    and mask of GPGridModel) and n scattered points X (n, d; numpy or device):
    cov(X, X) is approximated by W K W^T, K the grid operator.  order 'cubic'
    (Keys' cubic convolution, 4^d nodes per point, d <= 4) or 'linear' (2^d
    nodes, d <= 8).

    Every point must lie inside the interpolation domain -- for 'cubic' one
    cell inside the grid's ends on every axis (1 <= (x - lo) / h <= m - 2), for
    'linear' between the ends.  There is no clamping and no extrapolation: a
    point outside raises ValueError with the count.  Pad the grid by one cell
    around the data (InducingGrid(beyond_domain=) does that).

    interp(g): W g, grid -> points.  spread(p): W^T p, points -> grid, without
    atomics through an inverted index built here once (bitwise reproducible).
    n, N, nnz: points, nodes, entries of W.  Holds the stencil tables, the
    index and the library handle (gg_ski_*)."""

    SPLIT = 512   # rows of the inverted index longer than this are summed in chunks

    def __init__(self, xg, X, order='cubic'):
        from . import device as dev
        from . import native
        if order not in ('cubic', 'linear'):
            raise ValueError("order must be 'cubic' or 'linear'")
        self.order = order
        o = 4 if order == 'cubic' else 2
        d = len(xg)
        if o ** d > 256:
            raise ValueError("%s interpolation supports d <= %d (order^d <= 256), not d = %d"
                             % (order, 4 if o == 4 else 8, d))
        axes = [_even_axis(g, o, f) for f, g in enumerate(xg)]
        t = dev.torch()
        if isinstance(X, t.Tensor):
            if X.dim() != 2 or X.shape[1] != d:
                raise ValueError("X must be (n, %d)" % d)
            Xd = dev.to_device(X)
        else:
            X = np.asarray(X, dtype=np.float64)
            if X.ndim != 2 or X.shape[1] != d:
                raise ValueError("X must be (n, %d)" % d)
            Xd = dev.to_device(X)
        n = int(Xd.numel()) // d
        if n < 1:
            raise ValueError("X holds no point")
        self.d, self.n = d, n
        self.m = [a[2] for a in axes]
        self.N = int(np.prod(self.m))
        S = o ** d
        self.nnz = n * S
        L = native.lib()
        ms = native.i64_array(self.m)
        lo = (ctypes.c_double * d)(*[a[0] for a in axes])
        h = (ctypes.c_double * d)(*[a[1] for a in axes])
        device = dev.device()
        self.first = t.empty(n * d, dtype=t.int32, device=device)
        self.w = dev.empty(n * d * o)
        out = ctypes.c_int64()
        native.check(L.gg_ski_stencils(d, ms, lo, h, o, native.dptr(Xd), n,
                                       ctypes.c_void_p(self.first.data_ptr()),
                                       native.dptr(self.w), ctypes.byref(out),
                                       native.stream_ptr()), "gg_ski_stencils")
        # the inverted index of W^T: the entries sorted stably by node (within
        # a node in point order), an int64 row pointer
        node = t.empty(self.nnz, dtype=t.int64, device=device)
        wprod = dev.empty(self.nnz)
        native.check(L.gg_ski_expand(d, ms, o, n, ctypes.c_void_p(self.first.data_ptr()),
                                     native.dptr(self.w), ctypes.c_void_p(node.data_ptr()),
                                     native.dptr(wprod), native.stream_ptr()), "gg_ski_expand")
        node, perm = t.sort(node, stable=True)
        self.point = t.div(perm, S, rounding_mode='floor').to(t.int32)
        self.wprod = wprod[perm]
        del wprod, perm
        self.rowptr = t.searchsorted(node, t.arange(self.N + 1, dtype=t.int64, device=device))
        del node
        lens = self.rowptr[1:] - self.rowptr[:-1]
        self.max_row = int(lens.max().item())
        long_node = t.nonzero(lens > self.SPLIT).reshape(-1)
        nlong = int(long_node.numel())
        nchunks = 0
        self._long = None
        ptrs = [None] * 5
        if nlong:
            per = (lens[long_node] + self.SPLIT - 1) // self.SPLIT
            coff = t.zeros(nlong + 1, dtype=t.int64, device=device)
            coff[1:] = t.cumsum(per, 0)
            nchunks = int(coff[-1].item())
            row = t.repeat_interleave(t.arange(nlong, dtype=t.int64, device=device), per)
            k = t.arange(nchunks, dtype=t.int64, device=device) - coff[row]
            cb = self.rowptr[long_node[row]] + k * self.SPLIT
            ce = t.minimum(cb + self.SPLIT, self.rowptr[long_node[row] + 1])
            csum = dev.empty(nchunks)
            self._long = (long_node.contiguous(), coff, cb.contiguous(), ce.contiguous(), csum)
            ptrs = [ctypes.c_void_p(a.data_ptr()) for a in self._long]
        self.long_rows, self.chunks = nlong, nchunks
        hd = ctypes.c_void_p()
        native.check(L.gg_ski_create(d, ms, o, n, ctypes.c_void_p(self.first.data_ptr()),
                                     native.dptr(self.w), ctypes.c_void_p(self.rowptr.data_ptr()),
                                     ctypes.c_void_p(self.point.data_ptr()),
                                     native.dptr(self.wprod), self.SPLIT, nlong, ptrs[0], ptrs[1],
                                     nchunks, ptrs[2], ptrs[3], ptrs[4], ctypes.byref(hd)),
                     "gg_ski_create")
        self.h = hd

    def _apply(self, fn, v, n_in, n_out, out, what):
        from . import device as dev
        from . import native
        was_dev = dev.is_device_array(v)
        vd = v.detach().reshape(-1) if _is_device_doubles(v) else dev.to_device(v)
        if vd.numel() != n_in:
            raise ValueError("%s: the input must have %d entries, not %d"
                             % (what, n_in, vd.numel()))
        if out is None:
            od = dev.empty(n_out)
        else:
            if not _is_device_doubles(out) or out.numel() != n_out:
                raise ValueError("%s: out must be a contiguous float64 device tensor of %d "
                                 "entries" % (what, n_out))
            if out.data_ptr() == vd.data_ptr():
                raise ValueError("%s: out must not be the input" % what)
            od = out
        native.check(fn(self.h, native.dptr(vd), native.dptr(od), native.stream_ptr()), what)
        if out is not None or was_dev:
            return od
        return dev.to_host(od).reshape((n_out,) + np.shape(v)[1:])

    def interp(self, g, out=None):
        """W g: the N grid values interpolated to the n points (numpy in, numpy
        out; device in or out=, the device tensor)."""
        from . import native
        return self._apply(native.lib().gg_ski_interp, g, self.N, self.n, out, "gg_ski_interp")

    def spread(self, p, out=None):
        """W^T p: the n point values spread onto the N nodes; nodes that no
        point touches get exactly 0."""
        from . import native
        return self._apply(native.lib().gg_ski_spread, p, self.n, self.N, out, "gg_ski_spread")

    def __del__(self):
        try:
            from . import native
            if getattr(self, "h", None) is not None and self.h.value:
                native.load().gg_ski_destroy(self.h)
        except Exception:
            pass


class SKICG(object):
    """Resident CG state for (W K W^T + shift I) x = b over the n scattered
    points of a GridInterp W (gg_skicg_*): structured kernel interpolation on
    the Kronecker operator K.  Grid basis, textbook recurrence, x0 = 0; start /
    iterate / status / solve as MaskedKronCG.  coefficients() returns the
    (alpha_j, beta_j) of the current solve's iterations (at most max_steps are
    kept), from which tridiag() rebuilds the Lanczos tridiagonal."""

    def __init__(self, K, W, shift, max_steps=1024):
        from . import device as dev
        from . import native
        if not isinstance(W, GridInterp):
            raise ValueError("W must be a GridInterp")
        if int(K.shape[0]) != W.N or int(K.shape[1]) != W.N:
            raise ValueError("K must be %d x %d, the grid of W" % (W.N, W.N))
        self.K, self.W = K, W
        self.n = W.n
        self.shift = float(shift)
        self.max_steps = int(max_steps)
        self._dk = K._device()
        L = native.lib()
        we = ctypes.c_int64()
        native.check(L.gg_skicg_work_elems(self._dk.h, W.h, ctypes.byref(we)),
                     "gg_skicg_work_elems")
        self.work = dev.empty(we.value)
        h = ctypes.c_void_p()
        native.check(L.gg_skicg_create(self._dk.h, W.h, self.shift, native.dptr(self.work),
                                       self.max_steps, ctypes.byref(h)), "gg_skicg_create")
        self.h = h
        self.x = None

    def start(self, b_dev, rtol=1e-5, atol=0.0, x_out=None):
        from . import device as dev
        from . import native
        if b_dev.numel() != self.n:
            raise ValueError("b must have %d entries" % self.n)
        self.b = b_dev.reshape(-1)
        self.x = dev.empty(self.n) if x_out is None else x_out
        native.check(native.lib().gg_skicg_start(self.h, native.dptr(self.b),
                                                 native.dptr(self.x), float(rtol), float(atol),
                                                 native.stream_ptr()), "gg_skicg_start")

    def iterate(self, n_iter, check_every=0):
        from . import native
        n_iter = min(int(n_iter), 2 ** 31 - 1)
        native.check(native.lib().gg_skicg_iterate(self.h, n_iter, min(int(check_every), n_iter),
                                                   native.stream_ptr()), "gg_skicg_iterate")

    def status(self):
        from . import native
        it, conv = ctypes.c_int(), ctypes.c_int()
        res, tol = ctypes.c_double(), ctypes.c_double()
        native.check(native.lib().gg_skicg_status(self.h, ctypes.byref(it), ctypes.byref(conv),
                                                  ctypes.byref(res), ctypes.byref(tol),
                                                  native.stream_ptr()), "gg_skicg_status")
        return it.value, bool(conv.value), res.value, tol.value

    def solve(self, b_dev, rtol=1e-5, atol=0.0, maxiter=None, check_every=None, x_out=None):
        """start + iterate to convergence: (x, iterations, converged, |r|, tol)."""
        if maxiter is None:
            maxiter = self.n * 10
        if check_every is None:
            check_every = 10 if max(self.n, self.W.N) >= 1 << 20 else 50
        self.start(b_dev, rtol, atol, x_out=x_out)
        self.iterate(maxiter, check_every=check_every)
        return (self.x,) + self.status()

    def coefficients(self):
        """(alphas, betas) of the current solve's iterations, numpy."""
        from . import native
        k = self.max_steps
        a = (ctypes.c_double * max(k, 1))()
        b = (ctypes.c_double * max(k, 1))()
        got = ctypes.c_int()
        native.check(native.lib().gg_skicg_coefficients(self.h, k, a, b, ctypes.byref(got),
                                                        native.stream_ptr()),
                     "gg_skicg_coefficients")
        return np.array(a[:got.value]), np.array(b[:got.value])

    def __del__(self):
        try:
            from . import native
            if getattr(self, "h", None) is not None and self.h.value:
                native.load().gg_skicg_destroy(self.h)
        except Exception:
            pass


def cg_tridiag(alphas, betas):
    """The Lanczos tridiagonal of the Krylov space a CG run spanned, from its
    coefficients: T_jj = 1 / alpha_j + beta_{j-1} / alpha_{j-1}, T_{j,j+1} =
    sqrt(beta_j) / alpha_j.  (diagonal, off-diagonal), host."""
    a = np.asarray(alphas, dtype=np.float64)
    b = np.asarray(betas, dtype=np.float64)
    k = a.size
    diag = 1.0 / a
    diag[1:] += b[:k - 1] / a[:k - 1]
    return diag, np.sqrt(b[:k - 1]) / a[:k - 1]


def _refuse_with_interp(**given):
    for name, v in given.items():
        if v is not None:
            raise ValueError("interp=: the CG on scattered points runs on one GPU in the grid "
                             "basis without a mask, per-point noise or a preconditioner; %s= "
                             "cannot be combined" % name)


def cg(K, b, shift=0.0, rtol=1e-5, atol=0.0, maxiter=None, check_every=None, callback=None,
       recurrence=None, fusion=None, basis=None, comm=None, decomposition="auto",
       mask=None, precond=None, noise=None, interp=None):
    """Solve (K + shift I) x = b with CG on the device (x0 = 0).

    Same stopping rule and iterates as scipy.sparse.linalg.cg (recurrence:
    see KronCG; None = "fused", or "textbook" with mask=).  b: numpy
    (N,1)/(N,) or a CUDA tensor; x is returned in the same kind.  `callback`
    (e.g. a solver_counter) is called once per completed iteration, after the
    solve, with no arguments beyond the counter protocol (the iterates stay on
    the device).  Returns (x, info) like scipy: info = 0 converged, else the
    number of iterations run.

    comm (multi-GPU, one process per GPU): a torch.distributed process group,
    True for the default group, or an exchange object -- every rank calls cg
    with the same K and b and gets the whole x; the solve is sharded by
    distributed.solve (decomposition "auto": the parity-block basis's blocks
    over 2^K ranks where it exists, else the even / odd parity blocks, else
    factor 0 sharded).

    mask (bool / uint8, N entries, numpy or device; nonzero = observed): the
    grid with missing observations -- CG on (W K W + shift I) x = W b, W =
    diag(mask) (MaskedKronCG): x is 0 at the missing points and (K_oo + shift
    I)^-1 b_o on the observed ones, b there is ignored (NaN allowed).  Grid
    basis, textbook recurrence, one GPU: mask cannot be combined with comm=,
    basis='block' or an explicit recurrence='fused'.  precond='kron' (needs
    mask): the Kronecker eigenpair preconditioner of MaskedKronCG.

    noise (N positive doubles, numpy or device): per-point noise variances --
    CG on (W K W + D) x = W b, D = diag(noise) (MaskedKronCG(noise=); without
    mask= every point is observed): x is (K_oo + D_oo)^-1 b_o on the observed
    points; noise at the missing ones is ignored (NaN allowed).  The diagonal
    has one source of truth: shift must be 0 (or omitted) with noise=.  The
    rules of mask= hold (no comm=, basis='block', recurrence='fused' or
    fusion); precond='kron' is allowed.

    interp (a GridInterp W over K's grid): scattered data by structured kernel
    interpolation -- CG on (W K W^T + shift I) x = b over W.n points (SKICG); b
    and x have W.n entries.  Cannot be combined with mask=, noise=, comm=,
    basis= or precond= (ValueError).
    """
    from . import device as dev
    if interp is not None:
        _refuse_with_interp(mask=mask, noise=noise, comm=comm, basis=basis, precond=precond,
                            recurrence=None if recurrence == "textbook" else recurrence,
                            fusion=fusion)
        was_dev = dev.is_device_array(b)
        bd = dev.to_device(b)
        if bd.numel() != interp.n:
            raise ValueError('b is the wrong shape, must have %d entries' % interp.n)
        solver = SKICG(K, interp, shift, max_steps=0)
        x, it, conv, res, tol = solver.solve(bd, rtol, atol, maxiter=maxiter,
                                             check_every=check_every)
        if callback is not None:
            for _ in range(it):
                callback()
        info = 0 if conv else it
        out = x.reshape(tuple(b.shape)) if was_dev else dev.to_host(x).reshape(np.shape(b))
        cg.last = CGResult(out, info, it, res, tol)
        return out, info
    n = int(K.shape[0])
    if precond is not None and mask is None and noise is None:
        raise ValueError("precond= needs mask= (on a complete grid solve_schur is exact)")
    if noise is not None and shift is not None and float(shift) != 0.0:
        raise ValueError("noise= is the whole diagonal: shift must be 0 (or omitted)")
    if mask is not None or noise is not None:
        what = "mask=" if mask is not None else "noise="
        if comm is not None:
            raise ValueError("%s: the masked CG runs on one GPU, comm= cannot be combined"
                             % what)
        if basis == "block":
            raise ValueError("%s: W is not diagonal in the parity-block basis; use "
                             "basis='grid' (or None)" % what)
        if recurrence not in (None, "textbook"):
            raise ValueError("%s: the masked CG runs the textbook recurrence; "
                             "recurrence='fused' cannot be combined" % what)
        if fusion is not None:
            raise ValueError("%s: the masked CG has no fusion layouts" % what)
        if precond not in (None, 'kron'):
            raise ValueError("precond must be None or 'kron'")
    was_dev = dev.is_device_array(b)
    bd = dev.to_device(b)
    if bd.numel() != n:
        raise ValueError('b is the wrong shape, must have %d entries' % n)
    if maxiter is None:
        maxiter = n * 10
    if check_every is None:
        check_every = 10 if n >= 1 << 20 else 50
    if recurrence is None and mask is None and noise is None:
        recurrence = "fused"
    if comm is not None:
        from . import distributed
        # the sharded solve runs its own recurrence (fused, layout 0, in the
        # decomposition's basis): a non-default choice cannot be honoured there
        if recurrence != "fused" or fusion not in (None, 0) or basis is not None:
            raise ValueError("comm=: the sharded CG runs the fused recurrence (layout 0) in "
                             "the decomposition's own basis; recurrence / fusion / basis "
                             "cannot be chosen")
        x, info, it, how = distributed.solve(K, bd, shift, comm, rtol, atol, maxiter,
                                             check_every, decomposition)
        if callback is not None:
            for _ in range(it):
                callback()
        out = (x.reshape(tuple(b.shape)) if b.numel() == n else x) if was_dev else \
            dev.to_host(x).reshape(np.shape(b))
        res, tol = getattr(distributed.solve, "last_resid", (None, None))
        cg.last = CGResult(out, info, it, res, tol)
        cg.last.decomposition = how
        return out, info
    if mask is not None or noise is not None:
        solver = MaskedKronCG(K, shift, mask, precond=precond, noise=noise)
        solver.start(bd, rtol, atol)
        solver.iterate(maxiter, check_every=check_every)
        it, conv, res, tol = solver.status()
        if callback is not None:
            for _ in range(it):
                callback()
        info = 0 if conv else it
        x = solver.x
        if was_dev:
            out = x.reshape(tuple(b.shape)) if b.numel() == n else x
        else:
            out = dev.to_host(x).reshape(np.shape(b))
        cg.last = CGResult(out, info, it, res, tol)
        return out, info
    solver = KronCG(K, shift, recurrence, fusion=fusion, basis=basis)
    solver.start(bd, rtol, atol)
    # one call: the library polls the device's done flag every check_every
    # iterations and stops issuing work once converged
    solver.iterate(maxiter, check_every=check_every)
    it, conv, res, tol = solver.status()
    if callback is not None:
        for _ in range(it):
            callback()
    info = 0 if conv else it
    x = solver.x
    if was_dev:
        out = x.reshape(tuple(b.shape)) if b.numel() == n else x
    else:
        out = dev.to_host(x).reshape(np.shape(b))
    cg.last = CGResult(out, info, it, res, tol)
    return out, info


def lanczos_info(K):
    """(block, launches): whether gg_lanczos_probe runs the probe in the
    operator's parity-block basis (round 6; GG_LZ_BASIS=0 keeps the grid
    layout) and its launches per step."""
    from . import native
    b, L = ctypes.c_int(), ctypes.c_int()
    native.check(native.lib().gg_lanczos_info(K._device().h, ctypes.byref(b), ctypes.byref(L)),
                 "gg_lanczos_info")
    return bool(b.value), L.value


def lanczos_tridiag(K, shift, steps, seed=0, probe=0, work=None, timed=False, mask=None,
                    noise=None):
    """Device Lanczos on (K + shift I) from a Rademacher probe: (alphas, betas).

    work: optional device workspace of >= 4 N elements (allocated here
    otherwise).  timed=True also returns the per-step HIP-event times (ms, one
    per step run) and the summed time of each mode-product position
    (gg_lanczos_probe_timed): (alphas, betas, step_ms, launch_ms); the
    once-per-probe closing pass (the last beta's streaming pass, after the
    last step) is left in lanczos_tridiag.closing_ms.

    mask (bool / uint8, N entries, numpy or device; nonzero = observed; a
    device uint8 tensor is used where it lies, at any alignment): Lanczos on
    (W K W + shift I), W = diag(mask), from the same probe zeroed at the
    missing points and normalised by the observed count
    (gg_lanczos_probe_masked) -- the tridiagonal of (K_oo + shift I).  The
    count the library made is left in lanczos_tridiag.n_observed; timed=True
    returns (alphas, betas, step_ms).

    noise (N positive doubles, numpy or device; a contiguous float64 device
    tensor is used where it lies and, like a device mask, is not checked
    again): Lanczos on (W K W + D), D = diag(noise), the tridiagonal of K_oo +
    D_oo (gg_lanczos_probe_masked_noise; without mask= every point is
    observed).  shift must be 0 and timed=True is not offered."""
    from . import device as dev
    from . import native
    dk = K._device()
    n = int(K.shape[0])
    if noise is not None:
        if shift is not None and float(shift) != 0.0:
            raise ValueError("noise= is the whole diagonal: shift must be 0")
        shift = 0.0
        if timed:
            raise ValueError("noise=: the probe has no timed twin")
        if mask is None:
            mask = _all_ones_mask(n)
    if mask is not None:
        steps = int(steps)
        if steps < 1:
            raise ValueError("Lanczos needs steps >= 1")
        md = _mask_device_bytes(mask, n)
    if noise is not None:
        # a device vector is taken as it is, like a device mask
        nd = _noise_to_device(noise, n, md, check=not _is_device_doubles(noise))[0]
    if work is None:
        work = dev.empty(4 * n)
    elif int(work.numel()) < 4 * n:
        raise ValueError("Lanczos workspace needs %d elements" % (4 * n))
    a = (ctypes.c_double * steps)()
    b = (ctypes.c_double * steps)()
    done = ctypes.c_int()
    if mask is not None:
        nobs = ctypes.c_int64()
        args = (dk.h, float(shift), ctypes.c_void_p(md.data_ptr()), int(seed), int(probe), steps,
                native.dptr(work), a, b, ctypes.byref(done), ctypes.byref(nobs))
        if noise is not None:
            native.check(native.lib().gg_lanczos_probe_masked_noise(
                dk.h, native.dptr(nd), *(args[2:] + (native.stream_ptr(),))),
                "gg_lanczos_probe_masked_noise")
        elif timed:
            sm = (ctypes.c_double * steps)()
            native.check(native.lib().gg_lanczos_probe_masked_timed(
                *(args + (sm, native.stream_ptr()))), "gg_lanczos_probe_masked_timed")
        else:
            native.check(native.lib().gg_lanczos_probe_masked(*(args + (native.stream_ptr(),))),
                         "gg_lanczos_probe_masked")
        lanczos_tridiag.n_observed = int(nobs.value)
        k = done.value
        out = np.array(a[:k]), np.array(b[:max(k - 1, 0)])
        if timed:
            return out + ([sm[j] for j in range(steps)],)
        return out
    if timed:
        d = len(dk._keep)
        sm = (ctypes.c_double * steps)()
        lm = (ctypes.c_double * (d + 1))()
        native.check(native.lib().gg_lanczos_probe_timed(
            dk.h, float(shift), int(seed), int(probe), int(steps), native.dptr(work), a, b,
            ctypes.byref(done), sm, lm, native.stream_ptr()), "gg_lanczos_probe_timed")
    else:
        native.check(native.lib().gg_lanczos_probe(dk.h, float(shift), int(seed), int(probe),
                                                   int(steps), native.dptr(work), a, b,
                                                   ctypes.byref(done), native.stream_ptr()),
                     "gg_lanczos_probe")
    k = done.value
    out = np.array(a[:k]), np.array(b[:max(k - 1, 0)])
    if timed:
        lanczos_tridiag.closing_ms = lm[d]
        return out + ([sm[j] for j in range(steps)], [lm[i] for i in range(d)])
    return out


lanczos_tridiag.closing_ms = None
lanczos_tridiag.n_observed = None


def _mask_device_bytes(mask, n):
    """The mask as n device bytes for the masked probe: a contiguous device
    uint8 / bool tensor is taken where it lies (any alignment, no copy and no
    count: the library counts), anything else goes through _mask_to_device."""
    from . import device as dev
    t = dev.torch()
    if isinstance(mask, t.Tensor) and mask.is_cuda and mask.dtype in (t.uint8, t.bool) \
            and mask.is_contiguous():
        if mask.numel() != n:
            raise ValueError("mask must have %d entries, not %d" % (n, mask.numel()))
        return mask.detach().reshape(-1)
    return _mask_to_device(mask, n)[0]


def _slq_logdet_interp(K, shift, probes, steps, seed, W):
    """SLQ for log det(W K W^T + shift I): per probe z = gg_probe_fill(seed,
    probe) of length n, `steps` CG iterations with rtol = atol = 0, T from the
    coefficients, n e_1^T log(T) e_1."""
    from . import device as dev
    from . import native
    n = W.n
    steps = max(1, min(int(steps), n))
    solver = SKICG(K, W, shift, max_steps=steps)
    z, x = dev.empty(n), dev.empty(n)
    ests = []
    for j in range(probes):
        native.check(native.lib().gg_probe_fill(int(seed), j, native.dptr(z), n,
                                                native.stream_ptr()), "gg_probe_fill")
        solver.start(z, 0.0, 0.0, x_out=x)
        solver.iterate(steps)
        a, b = solver.coefficients()
        # an exactly invariant Krylov space ends the recurrence early (rho = 0)
        ok = np.isfinite(a) & np.isfinite(b) & (a > 0)
        k = int(a.size if ok.all() else np.argmin(ok))
        diag, off = cg_tridiag(a[:k], b[:k])
        T = np.diag(diag) + np.diag(off, 1) + np.diag(off, -1)
        theta, U = np.linalg.eigh(T)
        ests.append(float(n) * float(np.sum(U[0, :] ** 2 * np.log(theta))))
    return float(np.mean(ests)), np.array(ests)


def slq_logdet(K, shift, probes=8, steps=30, seed=0, mask=None, noise=None, interp=None):
    """Stochastic Lanczos quadrature estimate of log det(K + shift I):
    (mean, per-probe estimates).

    mask (as lanczos_tridiag): the estimate of log det(K_oo + shift I) on the
    observed points -- each probe's quadrature is scaled by the observed count
    and steps is capped at it; its cost is probes x steps Kronecker matvecs
    whatever the number of missing points.

    noise (as lanczos_tridiag; checked once here): the estimate of
    log det(K_oo + D_oo), D = diag(noise); shift must be 0.

    interp (a GridInterp W): the estimate of log det(W K W^T + shift I) over the
    W.n scattered points, from `steps` iterations of the CG on the points per
    probe (SKICG with rtol = atol = 0) whose coefficients give the Lanczos
    tridiagonal (cg_tridiag); cannot be combined with mask= or noise=."""
    if interp is not None:
        _refuse_with_interp(mask=mask, noise=noise)
        return _slq_logdet_interp(K, shift, probes, steps, seed, interp)
    n = int(K.shape[0])
    scale, kw = n, {}
    if noise is not None and mask is None:
        mask = _all_ones_mask(n)
    if mask is not None:
        from . import device as dev
        md, scale = _mask_to_device(mask, n)
        steps = min(int(steps), scale)
        kw = dict(work=dev.empty(4 * n), mask=md)
        if noise is not None:
            kw["noise"] = _noise_to_device(noise, n, md)[0]
    ests = []
    for j in range(probes):
        a, b = lanczos_tridiag(K, shift, steps, seed=seed, probe=j, **kw)
        T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
        theta, U = np.linalg.eigh(T)
        ests.append(float(scale) * float(np.sum(U[0, :] ** 2 * np.log(theta))))
    return float(np.mean(ests)), np.array(ests)


def trace_grad(K, dKs, shift, mask=None, probes=8, seed=0, rtol=1e-10, Z=None, solver=None,
               noise=None, noise_scale=None):
    """Probe estimates of the traces in the marginal likelihood's gradient:
    (means, per_probe) with A = W K W + shift I, W = diag(mask) (the identity
    without a mask).  per_probe is probes x (1 + len(dKs)): column 0 is
    z^T A^-1 z (the noise's trace, tr A_oo^-1 in expectation), column 1 + k is
    (A^-1 z)^T W dK_k W z (tr(A_oo^-1 dK_k,oo) in expectation); means is the
    column mean.

    dKs: KronMatrix operators (K with one factor replaced by its derivative).
    Probe j is the Rademacher vector gg_probe_fill(seed, j) zeroed at the
    missing points -- the vectors slq_logdet(mask=) starts from.  Z (N x k,
    numpy or device) replaces them (probes = k; also zeroed at the missing
    points): the unit vectors of the observed points give per-probe values that
    sum to the exact traces.  Each probe is one solve on a resident
    MaskedKronCG (KronCG without a mask) to rtol plus len(dKs) Kronecker
    matvecs and dots; the vectors are reused across probes.  solver: a resident
    MaskedKronCG / KronCG of (K, shift, mask) to solve with instead of a new
    one (GPGridModel passes its own, with its preconditioner).

    noise, noise_scale (given together; N doubles each, numpy or device): the
    per-point noise noise = noise_var * noise_scale, A = W K W + diag(noise)
    (MaskedKronCG(noise=); shift must then be 0).
    Column 0 becomes (A^-1 z)^T (noise_scale o z), the estimate of tr(A_oo^-1
    diag(noise_scale)_oo): the trace in the derivative by noise_var.  With
    solver= the solver's own noise is used and only noise_scale is needed."""
    from . import dense
    from . import device as dev
    from . import native
    n = int(K.shape[0])
    t = dev.torch()
    wd = None
    if noise is None and solver is not None:
        noise = getattr(solver, "noise", None)
    if (noise is None) != (noise_scale is None):
        raise ValueError("noise= and noise_scale= are given together")
    if noise is not None and solver is None:
        if shift is not None and float(shift) != 0.0:
            raise ValueError("noise= is the whole diagonal: shift must be 0")
        solver = MaskedKronCG(K, None, mask, noise=noise)
    if noise is not None:
        mask = solver.mask
        nsd = dev.to_device(noise_scale)
        if nsd.numel() != n:
            raise ValueError("noise_scale must have %d entries" % n)
        # a select: noise_scale at a missing point may be NaN
        nsd = t.where(solver.mask != 0, nsd, t.zeros_like(nsd))
    if mask is not None:
        if solver is None:
            solver = MaskedKronCG(K, shift, mask)
        wd = solver.mask.to(t.float64)
    elif solver is None:
        solver = KronCG(K, shift)
    if Z is not None:
        Zd = Z if dev.is_device_array(Z) else t.from_numpy(
            np.ascontiguousarray(np.asarray(Z, dtype=np.float64))).to(dev.device())
        if Zd.dim() != 2 or int(Zd.shape[0]) != n:
            raise ValueError("Z must be (%d, k)" % n)
        probes = int(Zd.shape[1])
    maxiter = n * 10
    check_every = 10 if n >= 1 << 20 else 50
    z, x, w = dev.empty(n), dev.empty(n), dev.empty(n)
    per = np.empty((int(probes), 1 + len(dKs)))
    for j in range(int(probes)):
        if Z is None:
            native.check(native.lib().gg_probe_fill(int(seed), j, native.dptr(z), n,
                                                    native.stream_ptr()), "gg_probe_fill")
        else:
            z.copy_(Zd[:, j])
        if wd is not None:
            dense.scale_rows(z, wd, 0)
        solver.start(z, rtol, 0.0, x_out=x)
        solver.iterate(maxiter, check_every=check_every)
        it, conv = solver.status()[:2]
        if not conv:
            logger.info('trace_grad: probe %d did not converge in %d iterations' % (j, it))
        if noise is not None:
            t.mul(z, nsd, out=w)
            per[j, 0] = dense.dot(x, w)
        else:
            per[j, 0] = dense.dot(z, x)
        for k, dK in enumerate(dKs):
            dK.matvec_device(z, out=w)
            per[j, 1 + k] = dense.dot(x, w)
    return per.mean(axis=0), per


class GridPosteriorSampler(object):
    """Joint draws of the posterior of the latent field f at all N grid points,
    y = f + noise observed with variance `shift` on the whole grid or, with
    mask=, on its observed points.

    Draw k is a function of (seed, k) alone: its normals are streams 2k (the
    prior / eigenbasis normals) and 2k + 1 (the noise normals) of
    gg_normal_fill's counter-based generator, regenerated inside the fused
    passes and never stored, so k < 32768.  Three routes:

      complete grid, solver='exact' (the default without a mask): the posterior
        is diagonal in the eigenbasis K = Q diag(t) Q^T; c = t / (t + s) Q^T y +
        sqrt(t s / (t + s)) z (gg_kron_posterior_coeffs) and the draw is Q c --
        one streaming pass and one Kronecker matvec, exactly Gaussian.
      complete grid, solver='cg': Matheron's rule in grid space.  f = Q (sqrt(t)
        z) is a prior draw (gg_kron_prior_coeffs), b = y - f - sqrt(s) e
        (gg_sample_residual), alpha = (K + s I)^-1 b by linalg.cg's resident
        solver (KronCG), and the draw is f + K alpha (gg_sample_accumulate).
      mask=: the same with b zeroed at the missing points and alpha from
        MaskedKronCG (masked_cg: a resident solver of (K, shift, mask) to
        reuse, e.g. the model's; else one is made with precond).

    y_dev: N doubles on the device (at the missing points it is not read: NaN
    allowed).  rtol: the CG's relative tolerance.  schur: (Q, T) of K.schur()
    to reuse.  The work vectors (three of N doubles, two in the eigenbasis
    route besides Q^T y) are held across draws.

    noise (N positive doubles, numpy or device): per-point noise variances, y =
    f + e with e_i ~ N(0, noise_i) at the observed points.  Matheron's route
    only (solver='exact' raises): b = y - f - sqrt(noise) o e
    (gg_sample_residual_noise) and alpha from MaskedKronCG(noise=); without
    mask= every point is observed.  shift must then be 0 or None; a masked_cg
    given must carry the noise itself.
    """

    MAX_DRAWS = 32768

    def __init__(self, K, shift, y_dev, mask=None, solver=None, precond=None, rtol=1e-10,
                 seed=0, masked_cg=None, schur=None, noise=None):
        from . import device as dev
        from . import native
        if noise is None and masked_cg is not None:
            noise = getattr(masked_cg, "noise", None)
        if solver is None:
            solver = 'exact' if mask is None and masked_cg is None and noise is None else 'cg'
        if solver not in ('exact', 'cg'):
            raise ValueError("solver must be 'exact' or 'cg'")
        if noise is not None and solver == 'exact':
            raise ValueError("noise=: the eigenbasis does not diagonalise K + diag(noise); "
                             "use solver='cg' (Matheron's rule)")
        masked = mask is not None or masked_cg is not None or noise is not None
        if masked and solver == 'exact':
            raise ValueError("mask=: solver='exact' does not apply to an incomplete grid; "
                             "use solver='cg'")
        if precond is not None and not masked:
            raise ValueError("precond= needs mask=")
        self.K = K
        self.shift = 0.0 if shift is None else float(shift)
        if noise is not None and masked_cg is None and self.shift != 0.0:
            raise ValueError("noise= is the whole diagonal: shift must be 0 (or None)")
        if noise is None and not self.shift > 0.0:
            raise ValueError("shift (the noise variance) must be positive")
        self.n = int(K.shape[0])
        self.rtol = float(rtol)
        self.seed = int(seed)
        self.y = dev.ensure_aligned(dev.to_device(y_dev))
        if self.y.numel() != self.n:
            raise ValueError("y must have %d entries" % self.n)
        self.Q, T = K.schur() if schur is None else schur
        lam = [np.asarray(e, dtype=np.float64).reshape(-1) for e in T.diag().K]
        self._d = len(lam)
        self._ms = native.i64_array([l.size for l in lam])
        self._lam = dev.to_device(np.concatenate(lam))
        self.mask = self._cg = self.noise = None
        if masked:
            self.route = 'matheron'
            self._cg = masked_cg if masked_cg is not None else \
                (MaskedKronCG(K, self.shift, mask, precond=precond) if noise is None else
                 MaskedKronCG(K, None, mask, precond=precond, noise=noise))
            if noise is not None:
                if self._cg.n != self.n or self._cg.noise is None:
                    raise ValueError("masked_cg solves another system")
                self.shift = self._cg.shift
            elif self._cg.n != self.n or self._cg.shift != self.shift or \
                    getattr(self._cg, "noise", None) is not None:
                raise ValueError("masked_cg solves another system")
            self.mask = self._cg.mask
            self.noise = self._cg.noise
        elif solver == 'cg':
            self.route = 'matheron'
            self._cg = KronCG(K, self.shift)
        else:
            self.route = 'eigen'
            self._yt = self.Q.matvec_device(self.y, transpose=True)
        self._c = dev.empty(self.n)          # coefficients, then b, then K alpha
        self._f = dev.empty(self.n)          # the prior draw (eigen route: the draw)
        self._alpha = dev.empty(self.n) if self.route == 'matheron' else None
        self.cg_iters = []

    def _streams(self, k):
        k = int(k)
        if k < 0 or k >= self.MAX_DRAWS:
            raise ValueError("draw index must be in [0, %d): draw k uses streams 2k and 2k + 1 "
                             "of 65536" % self.MAX_DRAWS)
        return 2 * k, 2 * k + 1

    def _terms(self, k):
        """(f, w) with draw k = f + w; w is None in the eigenbasis route."""
        from . import native
        L, sp = native.lib(), native.stream_ptr
        s0, s1 = self._streams(k)
        if self.route == 'eigen':
            native.check(L.gg_kron_posterior_coeffs(
                self._d, self._ms, native.dptr(self._lam), self.shift, native.dptr(self._yt),
                self.seed, s0, native.dptr(self._c), sp()), "gg_kron_posterior_coeffs")
            self.Q.matvec_device(self._c, out=self._f)
            return self._f, None
        native.check(L.gg_kron_prior_coeffs(
            self._d, self._ms, native.dptr(self._lam), self.seed, s0, native.dptr(self._c),
            sp()), "gg_kron_prior_coeffs")
        self.Q.matvec_device(self._c, out=self._f)
        mp = None if self.mask is None else ctypes.c_void_p(self.mask.data_ptr())
        if self.noise is not None:
            native.check(L.gg_sample_residual_noise(
                native.dptr(self.y), native.dptr(self._f), native.dptr(self.noise), mp,
                self.seed, s1, native.dptr(self._c), self.n, sp()), "gg_sample_residual_noise")
        else:
            native.check(L.gg_sample_residual(
                native.dptr(self.y), native.dptr(self._f), mp, float(np.sqrt(self.shift)),
                self.seed, s1, native.dptr(self._c), self.n, sp()), "gg_sample_residual")
        cg_ = self._cg
        cg_.start(self._c, self.rtol, 0.0, x_out=self._alpha)
        cg_.iterate(self.n * 10, check_every=10 if self.n >= 1 << 20 else 50)
        it, conv = cg_.status()[:2]
        if not conv:
            logger.info('posterior draw %d: CG did not converge in %d iterations' % (k, it))
        self.cg_iters.append(it)
        # the solve is over: its right-hand side's buffer takes K alpha
        self.K.matvec_device(self._alpha, out=self._c)
        return self._f, self._c

    def draw(self, k, out=None):
        """Draw k (N doubles on the device; into out when given)."""
        from . import device as dev
        from . import native
        if out is not None and (out.numel() != self.n or not out.is_contiguous()):
            raise ValueError("out must be a contiguous device vector of %d entries" % self.n)
        f, w = self._terms(k)
        if w is None:
            if out is None:
                return f.clone()
            out.reshape(-1).copy_(f)
            return out
        x = dev.empty(self.n) if out is None else out
        native.check(native.lib().gg_sample_accumulate(
            native.dptr(f), native.dptr(w), native.dptr(x), None, None, 0, self.n,
            native.stream_ptr()), "gg_sample_accumulate")
        return x

    def moments(self, n_samples):
        """(mean, var) of draws 0 .. n_samples - 1, each N doubles on the device:
        the sample mean and the unbiased sample variance, streamed through
        Welford's update (gg_sample_accumulate) without keeping a draw."""
        from . import device as dev
        from . import native
        S = int(n_samples)
        if S < 2:
            raise ValueError("the sample variance needs n_samples >= 2")
        self._streams(S - 1)
        mean, m2 = dev.empty(self.n), dev.empty(self.n)
        scale = 1.0
        for k in range(S):
            f, w = self._terms(k)
            if w is None:
                # the eigenbasis draw has one term: fold x + x and halve at the
                # end (scaling by two is exact in every step of the update)
                w, scale = f, 0.5
            native.check(native.lib().gg_sample_accumulate(
                native.dptr(f), native.dptr(w), None, native.dptr(mean), native.dptr(m2), k + 1,
                self.n, native.stream_ptr()), "gg_sample_accumulate")
        mean *= scale
        m2 *= scale * scale / (S - 1)
        return mean, m2


# ------------------------------------------------- Laplace approximation
LIKELIHOODS = {"poisson": 0, "binomial": 1}


def likelihood_constant(kind, y, aux, mask):
    """The f-independent part of sum_o log p (host; once per model): Poisson
    sum y log e - lgamma(y + 1), binomial sum lgamma(t + 1) - lgamma(y + 1) -
    lgamma(t - y + 1) over the observed points -- what gg_lik_newton leaves out
    of its sums[0]."""
    from scipy.special import gammaln
    m = np.asarray(mask).reshape(-1) != 0
    y = np.asarray(y, dtype=np.float64).reshape(-1)[m]
    e = np.ones(y.size) if aux is None else np.asarray(aux, dtype=np.float64).reshape(-1)[m]
    if kind == LIKELIHOODS["poisson"]:
        return float(np.sum(y * np.log(e) - gammaln(y + 1)))
    return float(np.sum(gammaln(e + 1) - gammaln(y + 1) - gammaln(e - y + 1)))


class LaplaceNewton(object):
    """The mode of psi(a) = sum_o log p(y_i | f_i) - 1/2 a^T K a, f = K a, for a
    log-concave likelihood on the grid ('poisson', log link; 'binomial', logit
    link): Newton's method in the (K + W^-1) form (Rasmussen & Williams Alg.
    3.1) on one MI355X.

    A step from a: b = select(mask, f + g / w, 0) and noise = 1 / w by one fused
    pass (gg_lik_newton), a_full = (W_mask K W_mask + diag(noise))^-1 b by the
    weighted masked CG from x0 = 0, then a <- a + s (a_full - a) with s = 1,
    halved (at most max_halvings times) while psi does not rise; each trial is
    one axpy, one Kronecker matvec and one read-only gg_lik_newton, whose five
    sums (40 bytes) are the only thing the host reads.  The solver is ONE
    MaskedKronCG built on the noise buffer: the handle keeps the pointer and
    the CG's kernels read the buffer afresh every iteration (gg_cgm_set_noise
    caches nothing derived from it), so a step rewrites it in place and solves
    again.  Its positivity check runs once, on the noise of a = 0.

    Stop rule: converged when |(g - a)_o| <= newton_tol max(1, |g_o|) (a = g at
    the mode); stalled when an accepted step raised psi by less than 1e-14
    |psi|, or no halving raised it -- psi's double-precision resolution, which
    a large Poisson problem reaches near a relative residual of 1e-9.  A trial
    that meets the stop rule is accepted whatever psi says: psi is concave, so
    a = g to the tolerance identifies the mode, while the last quadratic step
    gains about |g - a|^2, which the rounding of psi's sums hides once the
    residual is near 1e-6.

    y, aux (exposure / trials; None = 1), mask: N entries, numpy or device;
    values at the missing points are never used (NaN allowed).  const: the
    likelihood's f-independent normaliser (likelihood_constant), added to psi.
    precond='kron' goes to the solver; its scalar stand-in for the noise is
    the geometric mean of the noise at a = 0 and stays fixed over the steps --
    a heuristic whose effect on the iteration count has not been measured.

    mode(a0=None) runs the iteration (a0: a warm start, zeroed at the missing
    points) and leaves a, f, noise, b (device), psi, sum_log_w, newton_iters,
    newton_converged, newton_stalled, cg_iters (one entry per step) and
    halvings on the object.
    """

    def __init__(self, K, y, likelihood, aux=None, mask=None, precond=None, cg_rtol=1e-10,
                 newton_tol=1e-8, max_newton=50, max_halvings=20, const=0.0):
        from . import device as dev
        from . import native
        if likelihood not in LIKELIHOODS:
            raise ValueError("likelihood must be 'poisson' or 'binomial', not %r" % (likelihood,))
        self.kind = LIKELIHOODS[likelihood]
        self.K = K
        self.n = n = int(K.shape[0])
        t = dev.torch()
        self.mask = _all_ones_mask(n) if mask is None else _mask_to_device(mask, n)[0]
        self.y = dev.ensure_aligned(dev.to_device(y))
        self.aux = None if aux is None else dev.ensure_aligned(dev.to_device(aux))
        if self.y.numel() != n or (self.aux is not None and self.aux.numel() != n):
            raise ValueError("y and aux must have %d entries" % n)
        self.cg_rtol, self.newton_tol = float(cg_rtol), float(newton_tol)
        self.max_newton, self.max_halvings = int(max_newton), int(max_halvings)
        self.const = float(const)
        self.noise, self.b = dev.empty(n), dev.empty(n)
        self.a, self.f = dev.zeros(n), dev.zeros(n)
        self._a_try, self._f_try, self._x = dev.empty(n), dev.empty(n), dev.empty(n)
        self._sums = t.zeros(5, dtype=t.float64, device=self.a.device)
        self._partials = dev.empty(native.GG_LIK_PARTIALS)
        # the noise of a = 0 (f = 0): what the solver's one positivity check sees
        self._pass(self.f, self.a, write=True)
        self.solver = MaskedKronCG(K, None, self.mask, precond=precond, noise=self.noise)
        self.newton_iters, self.newton_converged, self.newton_stalled = 0, False, False
        self.cg_iters, self.halvings = [], []
        self.psi = self.sum_log_w = None

    def set_operator(self, K):
        """Another K of the same factor orders (new hyperparameters): a new
        solver on the same noise buffer; a and f stay for the warm start."""
        if int(K.shape[0]) != self.n:
            raise ValueError("K must have %d rows" % self.n)
        self.K = K
        self.solver = MaskedKronCG(K, None, self.mask, precond=self.solver.precond,
                                   noise=self.noise, precond_shift=self.solver.shift)

    def _pass(self, f, a, write):
        """gg_lik_newton at (f, a): the five sums on the host."""
        from . import native
        native.check(native.lib().gg_lik_newton(
            self.kind, native.dptr(self.y), None if self.aux is None else native.dptr(self.aux),
            native.dptr(f), native.dptr(a), ctypes.c_void_p(self.mask.data_ptr()),
            native.dptr(self.noise) if write else None, native.dptr(self.b) if write else None,
            native.dptr(self._sums), native.dptr(self._partials), self.n, native.stream_ptr()),
            "gg_lik_newton")
        return self._sums.cpu().numpy()

    def _stop(self, sums):
        # on finite sums only: an overflowed trial has inf <= inf
        return bool(np.all(np.isfinite(sums))
                    and np.sqrt(sums[3]) <= self.newton_tol * max(1.0, np.sqrt(sums[4])))

    def mode(self, a0=None):
        from . import dense
        from . import device as dev
        t = dev.torch()
        if a0 is None:
            self.a.zero_()
        else:
            a0 = dev.to_device(a0)
            if a0.numel() != self.n:
                raise ValueError("a0 must have %d entries" % self.n)
            t.where(self.mask != 0, a0, t.zeros_like(a0), out=self.a)
        K = self.K
        K.matvec_device(self.a, out=self.f)
        sums = self._pass(self.f, self.a, write=True)
        psi = sums[0] + self.const - 0.5 * sums[1]
        self.newton_iters, self.newton_converged, self.newton_stalled = 0, False, False
        self.cg_iters, self.halvings = [], []
        small_gain = False
        with np.errstate(invalid="ignore"):
            while True:
                if self._stop(sums):
                    self.newton_converged = True
                    break
                if small_gain or self.newton_iters >= self.max_newton:
                    self.newton_stalled = small_gain
                    break
                x, it, conv = self.solver.solve(self.b, rtol=self.cg_rtol, x_out=self._x)[:3]
                if not conv:
                    logger.info('Laplace Newton step %d: CG did not converge in %d iterations'
                                % (self.newton_iters, it))
                self.cg_iters.append(it)
                dense.axpby(-1.0, self.a, 1.0, x)    # the full step's direction
                s, accepted = 1.0, False
                for h in range(self.max_halvings + 1):
                    self._a_try.copy_(self.a)
                    dense.axpby(s, x, 1.0, self._a_try)
                    K.matvec_device(self._a_try, out=self._f_try)
                    sums_try = self._pass(self._f_try, self._a_try, write=False)
                    psi_try = sums_try[0] + self.const - 0.5 * sums_try[1]
                    if psi_try > psi or self._stop(sums_try):
                        accepted = True
                        break
                    s *= 0.5
                if not accepted:
                    self.newton_stalled = True
                    break
                self.halvings.append(h)
                small_gain = psi_try - psi < 1e-14 * abs(psi_try)
                self.a, self._a_try = self._a_try, self.a
                self.f, self._f_try = self._f_try, self.f
                psi = psi_try
                sums = self._pass(self.f, self.a, write=True)
                self.newton_iters += 1
        self.psi, self.sum_log_w = float(psi), float(sums[2])
        self.sums = sums
        return self.a
