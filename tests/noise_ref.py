"""NumPy restatement of the grid GP with per-point noise (test infrastructure
only).

The variance of observation i is noise_i = noise_var * noise_scale[i]; with W =
diag(mask) and D = diag(noise) the system is A = W K W + D, A x = W b, x zero at
the missing points.  weighted_cg is the (optionally preconditioned) CG the
device runs (gg_cgm_set_noise) with its split arithmetic p.K p + sum d p^2,
oracle.cg_solve's stopping rule and iteration count; weighted_lanczos /
weighted_slq are the recurrence of gg_lanczos_probe_masked_noise from
gg_probe_fill's probes.  Dense K_oo + D_oo algebra (dense_*) is the ground
truth the tests compare both against.  noise at the missing points is never
used: every function selects it away first.
"""
import numpy as np

import oracle
import masked_ref as mr

NOISE_VAR = 0.01

# (shape, fraction missing): the converged-solve cases; frac 0 is the complete
# grid (no mask: every point observed)
CG_CASES = [((7, 5, 3), 0.2), ((12, 10, 8), 0.1), ((12, 10, 8), 0.3), ((12, 10, 8), 0.0)]


def noise_scale(n):
    """exp(uniform(log 0.1, log 10)) from default_rng(3): two decades wide."""
    return np.exp(np.random.default_rng(3).uniform(np.log(0.1), np.log(10.0), n))


def make_mask(n, frac):
    """masked_ref.make_mask, or all ones for frac == 0."""
    return mr.make_mask(n, frac) if frac > 0 else np.ones(n, dtype=bool)


def _diag(mask, noise):
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    return mask, np.where(mask, np.asarray(noise, dtype=np.float64).reshape(-1), 0.0)


def geometric_mean(mask, noise):
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    return float(np.exp(np.mean(np.log(np.asarray(noise, dtype=np.float64).reshape(-1)[mask]))))


def weighted_cg(F, b, mask, noise, rtol=1e-5, atol=0.0, maxiter=None, precond=None,
                shift=None):
    """(x, info, iters) of CG on (W K W + D) x = W b, x0 = 0.

    precond None or 'kron': z = W Q diag(1 / (lam + shift)) Q^T r, shift the
    geometric mean of noise over the observed points unless given.  p.A p is
    formed as the device forms it, p.(K p) + sum_i d_i p_i^2, and the residual
    update uses select(mask, K p + d p, 0).  The stopping test is on the true
    |r|, seen after each update (oracle.cg_solve's count)."""
    mask, d = _diag(mask, noise)
    b = np.where(mask, np.asarray(b, dtype=np.float64).reshape(-1), 0.0)
    n = b.size
    if maxiter is None:
        maxiter = 10 * n
    bnorm = np.linalg.norm(b)
    tol = max(float(atol), float(rtol) * float(bnorm))
    x = np.zeros(n)
    if bnorm == 0:
        return x, 0, 0
    if precond == 'kron':
        if shift is None:
            shift = geometric_mean(mask, noise)
        Q, lam = mr.factor_eigh(F)
        QT = [q.T for q in Q]
        dinv = 1.0 / (mr.kron_eigs(lam) + shift)

        def M(r):
            return np.where(mask, oracle.kron_matvec(Q, dinv * oracle.kron_matvec(QT, r)), 0.0)
    elif precond is None:
        def M(r):
            return r
    else:
        raise ValueError("precond must be None or 'kron'")
    r = b.copy()
    z = M(r)
    rho = float(r.dot(z))
    p = z.copy()
    for it in range(maxiter):
        if np.linalg.norm(r) < tol:
            return x, 0, it
        t = oracle.kron_matvec(F, p)
        pq = float(p.dot(t)) + float(np.sum(d * p * p))
        alpha = rho / pq
        x += alpha * p
        r -= alpha * np.where(mask, t + d * p, 0.0)
        z = M(r)
        rho_new = float(r.dot(z))
        p = z + (rho_new / rho) * p
        rho = rho_new
    if np.linalg.norm(r) < tol:
        return x, 0, maxiter
    return x, maxiter, maxiter


def weighted_op(F, mask, noise):
    """v -> where(mask, K v, 0) + d v on vectors that are zero off the mask."""
    mask, d = _diag(mask, noise)
    return lambda v: np.where(mask, oracle.kron_matvec(F, v), 0.0) + d * v


def weighted_lanczos(F, mask, noise, seed, probe, steps):
    """(alphas, betas) of Lanczos on W K W + D from
    where(mask, probe_signs(seed, probe, N), 0)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    z = np.where(mask, oracle.cg.probe_signs(seed, probe, mask.size), 0.0)
    return oracle.lanczos_tridiag(weighted_op(F, mask, noise), z, steps)


def weighted_slq(F, mask, noise, probes=8, steps=30, seed=0):
    """(mean, per-probe estimates) of log det(K_oo + D_oo): n_obs times each
    probe's quadrature, steps capped at n_obs."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    n_obs = int(mask.sum())
    steps = min(int(steps), n_obs)
    ests = []
    for j in range(probes):
        a, b = weighted_lanczos(F, mask, noise, seed, j, steps)
        ests.append(oracle.cg.quadrature_logdet(a, b, float(n_obs)))
    return float(np.mean(ests)), np.array(ests)


def dense_A(F, mask, noise):
    """(K_oo + D_oo, observed indices)."""
    mask, d = _diag(mask, noise)
    o = np.nonzero(mask)[0]
    return mr.dense_K(F)[np.ix_(o, o)] + np.diag(d[o]), o


def dense_solve(F, b, mask, noise, A=None):
    """x with x_o = (K_oo + D_oo)^-1 b_o and 0 at the missing points."""
    Aoo, o = dense_A(F, mask, noise) if A is None else A
    x = np.zeros(np.asarray(mask).size)
    x[o] = np.linalg.solve(Aoo, np.asarray(b, dtype=np.float64).reshape(-1)[o])
    return x


def dense_logdet(F, mask, noise, A=None):
    Aoo, _ = dense_A(F, mask, noise) if A is None else A
    return float(np.linalg.slogdet(Aoo)[1])


def lml(y, alpha, logdet, mask):
    """-1/2 (y_o^T alpha_o + log det + n log 2 pi)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return -0.5 * (float(y[mask].dot(np.asarray(alpha).reshape(-1)[mask])) + logdet
                   + int(mask.sum()) * np.log(2 * np.pi))


def dense_lml(F, y, mask, noise, A=None):
    """The Gaussian log density of y_o under N(0, K_oo + D_oo)."""
    A = dense_A(F, mask, noise) if A is None else A
    return lml(y, dense_solve(F, y, mask, noise, A), dense_logdet(F, mask, noise, A), mask)


def noise_trace_estimates(F, mask, noise, scale, probes, seed, A=None):
    """Per-probe (A^-1 z)^T (scale o z), z = where(mask, probe_signs(seed, j), 0):
    column 0 of linalg.trace_grad(noise=, noise_scale=); and the sums of the
    absolute terms (what a relative error bound is taken of)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    A = dense_A(F, mask, noise) if A is None else A
    sc = np.where(mask, np.asarray(scale, dtype=np.float64).reshape(-1), 0.0)
    out, absout = [], []
    for j in range(probes):
        z = np.where(mask, oracle.cg.probe_signs(seed, j, mask.size), 0.0)
        terms = dense_solve(F, z, mask, noise, A) * sc * z
        out.append(float(terms.sum()))
        absout.append(float(np.abs(terms).sum()))
    return np.array(out), np.array(absout)


_cache = {}


def case(ms, frac):
    """dict(F, mask, scale, noise, y, A, x) for one shape and missing fraction
    at noise_var = NOISE_VAR: y from default_rng(1), x the dense solve of y.
    Computed once per session, shared and read-only (y stays writable: torch
    wraps it without a copy on its way to the device)."""
    key = (tuple(ms), frac)
    if key not in _cache:
        F = mr.rbf_factors(ms)
        n = int(np.prod(ms))
        mask = make_mask(n, frac)
        scale = noise_scale(n)
        noise = NOISE_VAR * scale
        y = np.random.default_rng(1).standard_normal(n)
        A = dense_A(F, mask, noise)
        x = dense_solve(F, y, mask, noise, A)
        for a in F + [mask, scale, noise, x, A[0], A[1]]:
            a.setflags(write=False)
        _cache[key] = dict(F=F, mask=mask, scale=scale, noise=noise, y=y, A=A, x=x)
    return _cache[key]
