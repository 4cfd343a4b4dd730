"""NumPy restatement of the Laplace approximation on a grid with Poisson /
binomial likelihoods (test infrastructure only).

Observed set o (mask), a zero at the missing points, f = K a.  The objective is
psi(a) = sum_o log p_i(f_i) - 1/2 a^T K a; a Newton step solves (W_mask K W_mask
+ diag(1 / w)) a_full = select(mask, f + g / w, 0) -- noise_ref.weighted_cg's
system -- and moves a by a halved step until psi rises.  newton() is the
driver the device runs (linalg.LaplaceNewton) with its step and stop rules;
solve='dense' replaces the CG by noise_ref.dense_solve, the ground truth.

log p is split as the device splits it: `core` depends on f, `log_norm` does
not (the lgamma terms, and y log e for the Poisson exposure) and is a
per-model constant.  newton_pass restates gg_lik_newton: the element outputs
and the five sums (sums[0] is the sum of the core).
"""
import numpy as np
from scipy.special import gammaln

import oracle
import masked_ref as mr
import noise_ref as nr

POISSON, BINOMIAL = 0, 1
KINDS = {"poisson": POISSON, "binomial": BINOMIAL}
CLAMP = 700.0

# (shape, fraction missing, amplitude): frac 0 is the complete grid
CASES = [((7, 5, 3), 0.2, 1.0), ((12, 10, 8), 0.1, 1.0), ((12, 10, 8), 0.0, 2.0)]
LIKELIHOODS = ["poisson", "binomial"]


def factors(ms, amp=1.0, ls=0.1):
    """masked_ref.rbf_factors (lengthscales ls (1 + 0.05 i)) with the variance
    amp^2 on factor 0."""
    F = []
    for i, m in enumerate(ms):
        g = np.linspace(0, 1, m)
        var = float(amp) ** 2 if i == 0 else 1.0
        F.append(oracle.cov_1d("RBF", g, g, var, ls * (1 + 0.05 * i)) + 1e-12 * np.eye(m))
    return F


def _aux(aux, n):
    return np.ones(n) if aux is None else np.asarray(aux, dtype=np.float64).reshape(-1)


def log_norm(kind, y, aux, mask):
    """The f-independent part of sum_o log p: a per-model constant."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    e = _aux(aux, y.size)
    y, e = y[mask], e[mask]
    if kind == POISSON:
        return float(np.sum(y * np.log(e) - gammaln(y + 1)))
    return float(np.sum(gammaln(e + 1) - gammaln(y + 1) - gammaln(e - y + 1)))


def point(kind, y, e, f, dtype=np.float64):
    """(core log p, g, w, 1 / w, g / w) per point, in `dtype` (np.longdouble:
    the element outputs to well below a double's ulp).  w and what derives
    from it use f clamped to +-700; no exp of a positive argument for the
    binomial."""
    y, e, f = (np.asarray(v, dtype=dtype) for v in (y, e, f))
    one = dtype(1)
    fc = np.clip(f, -CLAMP, CLAMP)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if kind == POISSON:
            rate = e * np.exp(f)
            w = e * np.exp(fc)
            return y * f - rate, y - rate, w, one / w, y / w - one
        t = np.exp(-np.abs(fc))
        tu = np.where(np.abs(f) > CLAMP, dtype(0), t)
        sig = np.where(f >= 0, one / (one + tu), tu / (one + tu))
        w = e * t / ((one + t) * (one + t))
        q = np.where(f >= 0, (one + t) / t, one + t)     # 1 / sigma(-f)
        core = y * f - e * (np.maximum(f, 0) + np.log1p(tu))
        return core, y - e * sig, w, one / w, y / w - q


def newton_pass(kind, y, aux, f, a, mask=None, precise=False):
    """gg_lik_newton: (noise, b, sums, abs_sums).  noise = 1 / w and b = f + g /
    w where observed, 1 and 0 elsewhere; sums = [sum core log p, sum a f, sum
    log w, sum (g - a)^2, sum g^2] over the observed points and abs_sums the
    sums of the absolute terms (what a rounding bound is taken of).
    precise: the element outputs computed in long double, rounded once."""
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    n = f.size
    m = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    y = np.where(m, np.asarray(y, dtype=np.float64).reshape(-1), 0.0)
    e = np.where(m, _aux(aux, n), 1.0)
    fo, ao = np.where(m, f, 0.0), np.where(m, a, 0.0)
    core, g, w, winv, gw = point(kind, y, e, fo)
    if precise:
        ld = np.longdouble
        _, _, _, winv_p, gw_p = point(kind, y, e, fo, dtype=ld)
        noise = np.where(m, winv_p.astype(np.float64), 1.0)
        b = np.where(m, (fo.astype(ld) + gw_p).astype(np.float64), 0.0)
    else:
        noise = np.where(m, winv, 1.0)
        b = np.where(m, fo + gw, 0.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        terms = [core, ao * fo, np.log(w), (g - ao) ** 2, g * g]
        sums = np.array([float(np.sum(t[m])) for t in terms])
        abs_sums = np.array([float(np.sum(np.abs(t[m]))) for t in terms])
    return noise, b, sums, abs_sums


def _stop(sums, newton_tol):
    """The stop rule, on finite sums only (an overflowed trial has inf <= inf)."""
    return bool(np.all(np.isfinite(sums))
                and np.sqrt(sums[3]) <= newton_tol * max(1.0, np.sqrt(sums[4])))


def newton(F, kind, y, aux, mask, solve="cg", cg_rtol=1e-11, newton_tol=1e-8, max_newton=50,
           max_halvings=20, a0=None, precond=None):
    """The mode of psi by Newton's method with step halving: dict(a, f, noise,
    b, sums, psi, iters, converged, stalled, cg_iters, psis, halvings).

    Stop rule: converged when |(g - a)_o| <= newton_tol max(1, |g_o|); stalled
    when an accepted step raised psi by less than 1e-14 |psi| or no halving
    raised it.  A trial is accepted when psi rises -- or when it meets the stop
    rule: psi is concave, so a = g to the tolerance identifies the mode
    whatever psi's rounding says.  The last quadratic step gains about |g -
    a|^2, which psi (a sum with terms up to 1e5 here) no longer resolves once
    the residual is near 1e-6; judged by psi alone it would be refused one
    step short of the tolerance.  solve: 'cg' (noise_ref.weighted_cg to cg_rtol, x0
    = 0) or 'dense'.  precond='kron': the preconditioner's scalar stand-in for
    the noise is the geometric mean of the noise at a = 0 on every step and
    whatever a0 is, as the device's solver fixes it when it is built."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    n = mask.size
    const = log_norm(kind, y, aux, mask)
    a = np.zeros(n) if a0 is None else np.where(mask, np.asarray(a0, dtype=np.float64), 0.0)
    f = oracle.kron_matvec(F, a)
    noise, b, sums, _ = newton_pass(kind, y, aux, f, a, mask)
    psi = sums[0] + const - 0.5 * sums[1]
    out = dict(iters=0, converged=False, stalled=False, cg_iters=[], psis=[psi], halvings=[])
    small_gain = False
    shift = None
    if precond == "kron":
        zero = np.zeros(n)
        shift = nr.geometric_mean(mask, newton_pass(kind, y, aux, zero, zero, mask)[0])
    while True:
        if _stop(sums, newton_tol):
            out["converged"] = True
            break
        if small_gain or out["iters"] >= max_newton:
            out["stalled"] = small_gain
            break
        if solve == "dense":
            a_full = nr.dense_solve(F, b, mask, noise)
        else:
            a_full, _, it = nr.weighted_cg(F, b, mask, noise, rtol=cg_rtol, precond=precond,
                                          shift=shift)
            out["cg_iters"].append(it)
        d = a_full - a
        s, accepted = 1.0, False
        for h in range(max_halvings + 1):
            a_try = a + s * d
            f_try = oracle.kron_matvec(F, a_try)
            sums_try = newton_pass(kind, y, aux, f_try, a_try, mask)[2]
            psi_try = sums_try[0] + const - 0.5 * sums_try[1]
            if psi_try > psi or _stop(sums_try, newton_tol):
                accepted = True
                break
            s *= 0.5
        if not accepted:
            out["stalled"] = True
            break
        out["halvings"].append(h)
        small_gain = psi_try - psi < 1e-14 * abs(psi_try)
        a, f, psi = a_try, f_try, psi_try
        noise, b, sums, _ = newton_pass(kind, y, aux, f, a, mask)
        out["iters"] += 1
        out["psis"].append(psi)
    out.update(a=a, f=f, noise=noise, b=b, sums=sums, psi=psi, const=const)
    return out


def laplace_lml(psi, logdet, sum_log_w):
    """psi(a^) - 1/2 [log det(K_oo + W^-1_oo) + sum_o log w_i]."""
    return psi - 0.5 * (logdet + sum_log_w)


def dense_cov(F, mask, noise):
    """The Laplace posterior covariance of f at all N points: (K^-1 + W)^-1 =
    K - K_:o (K_oo + W^-1_oo)^-1 K_o:."""
    K = mr.dense_K(F)
    Aoo, o = nr.dense_A(F, mask, noise)
    Ko = K[:, o]
    return K - Ko.dot(np.linalg.solve(Aoo, Ko.T))


def response_law(kind, mu, var, order=64):
    """(mean, variance) of exp(x) or sigma(x), x ~ N(mu, var), per point: the
    lognormal's closed form, the logistic-normal's by Gauss-Hermite."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    var = np.maximum(np.asarray(var, dtype=np.float64).reshape(-1), 0.0)
    if kind == POISSON:
        mean = np.exp(mu + 0.5 * var)
        return mean, np.expm1(var) * mean * mean
    x, wq = np.polynomial.hermite.hermgauss(order)
    z = mu[:, None] + np.sqrt(2.0 * var)[:, None] * x[None, :]
    r = 0.5 * (1.0 + np.tanh(0.5 * z))
    wq = wq / np.sqrt(np.pi)
    mean = r.dot(wq)
    return mean, np.maximum((r * r).dot(wq) - mean * mean, 0.0)


_cache = {}


def case(ms, frac, amp, lik):
    """dict(F, mask, y, aux, kind, f_true) of one case, data from default_rng(5):
    f_true a draw of the prior N(0, K); Poisson exposure exp(U(log .5, log 4)),
    y ~ Poisson(e exp f_true); binomial trials integers in 1..5, y ~ Bin(t,
    sigma(f_true)).  Once per session, shared and read-only."""
    key = (tuple(ms), frac, amp, lik)
    if key not in _cache:
        F = factors(ms, amp)
        n = int(np.prod(ms))
        mask = nr.make_mask(n, frac)
        rng = np.random.default_rng(5)
        Q, lam = mr.factor_eigh(F)
        f_true = oracle.kron_matvec(Q, np.sqrt(np.maximum(mr.kron_eigs(lam), 0.0))
                                    * rng.standard_normal(n))
        kind = KINDS[lik]
        if kind == POISSON:
            aux = np.exp(rng.uniform(np.log(0.5), np.log(4.0), n))
            y = rng.poisson(aux * np.exp(f_true)).astype(np.float64)
        else:
            aux = rng.integers(1, 6, n).astype(np.float64)
            y = rng.binomial(aux.astype(np.int64), 1.0 / (1.0 + np.exp(-f_true))).astype(
                np.float64)
        for v in F + [mask, aux, f_true]:
            v.setflags(write=False)
        _cache[key] = dict(F=F, mask=mask, y=y, aux=aux, kind=kind, f_true=f_true)
    return _cache[key]


def mode(ms, frac, amp, lik, solve="dense", **kw):
    """newton() of a case, once per (case, solver, settings)."""
    key = ("mode", tuple(ms), frac, amp, lik, solve, tuple(sorted(kw.items())))
    if key not in _cache:
        C = case(ms, frac, amp, lik)
        _cache[key] = newton(C["F"], C["kind"], C["y"], C["aux"], C["mask"], solve=solve, **kw)
    return _cache[key]
