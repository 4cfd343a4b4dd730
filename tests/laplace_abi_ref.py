"""The reference side of the Laplace likelihood C ABI's edge tests
(test_gpu_laplace_abi.py; held to itself on the CPU by test_laplace_abi_ref.py).

Everything here is laplace_ref's arithmetic evaluated in np.longdouble (64
mantissa bits and a wider exponent, so neither exp(700) nor 1 / (1e-4
exp(-700)) overflows or goes denormal on the way) and rounded once:

  edge_points   rows (y, aux, f, a) at the clamp, the saturation branches and
                the corners of the documented exposure range
  pass_ref      gg_lik_newton's element outputs and five sums, with the bound
                of b and the sums of the absolute terms
  pass_errors   the figures a test asserts on (error over bound, classes of
                the non-finite values, NaN)
  response_ref  gg_lik_response_accumulate's Welford moments
  driver_case   the LaplaceNewton cases that halve, reject an overflowed
                trial and stall, with their laplace_ref.newton runs
"""
import numpy as np

import oracle
import masked_ref as mr
import noise_ref as nr
import laplace_ref as lr

LD = np.longdouble
CLAMP = lr.CLAMP
EXP_OVERFLOW = 709.782712893384     # log of the largest double

# the tolerances test_gpu_laplace.py states for the pass
NOISE_RTOL = 1e-14
B_TOL = 1e-14          # times |f| + (|y| + w) / w
SUM_TOL = 1e-12        # times the sum of the absolute terms
# b where the stated bound is below half the spacing of the doubles at b, so
# that only the correctly rounded value meets it (binomial, y = 0, f >= 36: b = f
# - 1 - exp(f) is all exp(f) while (|y| + w) / w is 1): what the double-precision
# restatement is held to there -- its exp is within 1 ulp, and b and its
# reference are each rounded once: 1 + 1/2 + 1/2 ulp, held to 3.  The device is
# held to the stated bound everywhere.
B_ULPS = 3.0

EDGE_F = [0.0, 36.0, 37.0, 699.9999, 700.0, float(np.nextafter(700.0, np.inf)), 710.0, 745.2,
          1e4]
EDGE_AUX = [None, 1e-4, 1.0, 1e4]
# the one row whose reference b is +inf: y / w = 1e6 * 1.014e308
DESIGNATED = dict(kind=lr.POISSON, e=1e-4, f=-700.0, y=1e6)


def edge_points(kind):
    """dict(y, e, f, a, given, designated) of rows: f in +-EDGE_F (signed
    zeros included), aux in EDGE_AUX (`given` False: the rows of a call with
    aux NULL, e = 1 there), y in {0, aux, mid}; mid is aux / 2 for the
    binomial and 1.5 for the Poisson -- 1.5 / (1e-4 exp(-700)) = 1.52e308 is
    still a double, so every long-double b rounds to a finite double except at
    the `designated` row (Poisson only, appended last).  a ~ N(0, 1) from
    default_rng(23)."""
    rows = []
    for f in EDGE_F:
        for sf in (f, -f):
            for aux in EDGE_AUX:
                e = 1.0 if aux is None else aux
                mid = 0.5 * e if kind == lr.BINOMIAL else 1.5
                for y in (0.0, e, mid):
                    rows.append((y, e, sf, aux is not None, False))
    if kind == lr.POISSON:
        rows.append((DESIGNATED["y"], DESIGNATED["e"], DESIGNATED["f"], True, True))
    y, e, f, given, des = (np.array(c) for c in zip(*rows))
    a = np.random.default_rng(23).standard_normal(f.size)
    out = dict(y=y.astype(np.float64), e=e.astype(np.float64), f=f.astype(np.float64), a=a,
               given=given.astype(bool), designated=des.astype(bool))
    for v in out.values():
        v.setflags(write=False)
    return out


def clamped(f):
    return np.clip(np.asarray(f, dtype=np.float64), -CLAMP, CLAMP)


def _round(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=LD).astype(np.float64)


def pass_ref(kind, y, aux, f, a, mask=None):
    """gg_lik_newton in long double, rounded once: dict(noise, b, sums,
    abs_sums (float64); w, b_bound (long double, per point); m).  noise 1 and b
    0 at the missing points, whose inputs are never touched.  b_bound is
    B_TOL (|f| + (|y| + w) / w) -- in long double, where y / w cannot overflow."""
    f = np.asarray(f, dtype=np.float64).reshape(-1)
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    n = f.size
    m = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    y = np.where(m, np.asarray(y, dtype=np.float64).reshape(-1), 0.0)
    e = np.where(m, np.ones(n) if aux is None else np.asarray(aux, dtype=np.float64).reshape(-1),
                 1.0)
    fo, ao = np.where(m, f, 0.0).astype(LD), np.where(m, a, 0.0).astype(LD)
    core, g, w, winv, gw = lr.point(kind, y, e, fo, dtype=LD)
    if kind == lr.POISSON:
        # the rate is e times a double exp(f): inf once exp overflows, however
        # small e is (long double alone would keep 1e-4 exp(710) finite)
        over = fo > EXP_OVERFLOW
        core, g = np.where(over, -LD(np.inf), core), np.where(over, -LD(np.inf), g)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        terms = [core, ao * fo, np.log(w), (g - ao) ** 2, g * g]
        sums = np.array([_round(np.sum(t[m])) for t in terms])
        abs_sums = np.array([_round(np.sum(np.abs(t[m]))) for t in terms])
        bound = LD(B_TOL) * (np.abs(fo) + (np.abs(y.astype(LD)) + w) / w)
    return dict(noise=np.where(m, _round(winv), 1.0), b=np.where(m, _round(fo + gw), 0.0),
                sums=sums, abs_sums=abs_sums, w=w, b_bound=bound, m=m)


def same_class(x, ref):
    """x equals ref wherever ref is not finite (inf of the same sign; NaN
    never matches) and is finite wherever ref is."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nf = ~np.isfinite(ref)
    return bool(np.all(x[nf] == ref[nf]) and np.all(np.isfinite(x[~nf])))


def pass_errors(R, noise, b, sums):
    """The figures of a pass against pass_ref's R: dict(noise: worst relative
    error; b: worst error over b_bound, over every point; b_reach: the same
    over the points where b_bound is at least half the spacing of the doubles
    at the reference b, so that some double other than the reference itself
    meets it; b_ulps: worst error in units of that spacing over the other
    points, `below` of them; sums: error over abs_sums per sum, 0 where the
    reference sum is not finite; classes: the non-finite reference values are
    matched exactly and nothing else is non-finite; nan: a NaN in any output).
    Element figures over the observed points with a finite reference."""
    m = R["m"]
    noise, b, sums = (np.asarray(v, dtype=np.float64) for v in (noise, b, sums))
    nan = bool(np.isnan(noise).any() or np.isnan(b).any() or np.isnan(sums).any())
    classes = same_class(noise, R["noise"]) and same_class(b, R["b"]) and \
        same_class(sums, R["sums"])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        fin = m & np.isfinite(R["b"]) & np.isfinite(b)
        en = np.abs(noise - R["noise"]) / R["noise"]
        db = np.abs(b.astype(LD) - R["b"].astype(LD))
        eb = db / R["b_bound"]
        spacing = np.spacing(np.maximum(np.abs(R["b"]), np.finfo(np.float64).tiny))
        below = fin & (R["b_bound"] < 0.5 * spacing)
        ulps = db / spacing
        fs = np.isfinite(R["sums"]) & np.isfinite(sums)
        es = np.where(fs, np.abs(sums - R["sums"]) / np.maximum(R["abs_sums"], 1e-300), 0.0)
    pick = lambda v, k: float(np.max(v[k])) if k.any() else 0.0   # noqa: E731
    return dict(noise=pick(en, m & np.isfinite(noise)), b=pick(eb, fin),
                b_reach=pick(eb, fin & ~below), b_ulps=pick(ulps, below), below=int(below.sum()),
                sums=es, classes=bool(classes), nan=nan)


def response(kind, x, dtype=LD):
    """exp(x) or sigma(x) without an exp of a positive argument."""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(over="ignore", under="ignore"):
        if kind == lr.POISSON:
            return np.exp(x)
        t = np.exp(-np.abs(x))
        return np.where(x >= 0, dtype(1) / (dtype(1) + t), t / (dtype(1) + t))


def response_ref(kind, F, W):
    """gg_lik_response_accumulate over the draws F[k] + W[k] (S x n): Welford's
    moments in long double, rounded once: (mean, m2, same); same[i]: every
    response of point i rounds to one double, where m2 must be exactly 0."""
    F, W = np.asarray(F, dtype=np.float64), np.asarray(W, dtype=np.float64)
    r = response(kind, F + W)     # the sum of two doubles is formed in double
    mean, m2 = np.zeros(F.shape[1], dtype=LD), np.zeros(F.shape[1], dtype=LD)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for k in range(1, F.shape[0] + 1):
            d = r[k - 1] - mean
            mean = mean + d / LD(k)
            m2 = m2 + d * (r[k - 1] - mean)
        rd = _round(r)
    same = np.all(rd == rd[:1], axis=0)
    return _round(mean), _round(m2), same


def response_values(kind, n, draws=5):
    """(F, W), draws x n: N(0, 2) draws with, from point 0 on (as many as fit
    in n), the edge columns -- x = +0 and -0 on every draw; binomial: x = 40,
    745, 1e4 in turn (sigma rounds to 1 on every draw: m2 is exactly 0), x =
    -40, -745, -1e4 in turn (tiny, denormal, 0), x = 1e4 and x = -1e4 on every
    draw; Poisson: x = 700 on every draw (exp finite, m2 = 0), x = -745 and -700
    in turn, x = -745 on every draw.  The edge x is split as f + w with f = x
    and w = +-0."""
    rng = np.random.default_rng(7 + kind)
    F, W = rng.standard_normal((draws, n)), rng.standard_normal((draws, n))
    if kind == lr.BINOMIAL:
        cols = [[0.0], [-0.0], [40.0, 745.0, 1e4], [-40.0, -745.0, -1e4], [1e4], [-1e4]]
    else:
        cols = [[0.0], [-0.0], [700.0], [-745.0, -700.0], [-745.0]]
    for j, vals in enumerate(cols[:n]):
        for k in range(draws):
            F[k, j] = vals[k % len(vals)]
            W[k, j] = -0.0 if (j + k) % 2 else 0.0
    return F, W


# ------------------------------------------------------------ the driver
GRID = (7, 5, 3)
# name -> (amp, exposure scale, aux given, newton settings)
DRIVER_CASES = {
    "halving": (1.0, 30.0, True, {}),
    "overflow": (2.0, 20.0, False, {}),
}
_cache = {}


def driver_case(name):
    """dict(F, mask, y, aux, kind) of a Poisson case on the 7 x 5 x 3 grid from
    default_rng(11): make_mask(105, 0.2), f_true a draw of the prior with
    amplitude amp, exposure scale exp(U(log .5, log 4)), y ~ Poisson(e exp
    f_true); `aux given` False hands the same y over with aux = None."""
    if name not in _cache:
        amp, scale, given, _ = DRIVER_CASES[name]
        F = lr.factors(GRID, amp)
        n = int(np.prod(GRID))
        mask = nr.make_mask(n, 0.2)
        rng = np.random.default_rng(11)
        Q, lam = mr.factor_eigh(F)
        f_true = oracle.kron_matvec(Q, np.sqrt(np.maximum(mr.kron_eigs(lam), 0.0))
                                    * rng.standard_normal(n))
        aux = scale * np.exp(rng.uniform(np.log(0.5), np.log(4.0), n))
        y = rng.poisson(aux * np.exp(f_true)).astype(np.float64)
        for v in F + [mask, aux, y]:
            v.setflags(write=False)
        _cache[name] = dict(F=F, mask=mask, y=y, aux=aux if given else None, kind=lr.POISSON)
    return _cache[name]


def driver_run(name, solve="cg", **kw):
    """laplace_ref.newton of a driver case (cg_rtol 1e-11 unless given), once
    per (case, solver, settings)."""
    if solve == "cg":
        kw.setdefault("cg_rtol", 1e-11)
    key = (name, solve, tuple(sorted(kw.items())))
    if key not in _cache:
        C = driver_case(name)
        _cache[key] = lr.newton(C["F"], C["kind"], C["y"], C["aux"], C["mask"], solve=solve, **kw)
    return _cache[key]


def first_trial_sums(name):
    """The five sums of the first step's full trial (s = 1) from a = 0."""
    C = driver_case(name)
    n = C["mask"].size
    noise, b, _, _ = lr.newton_pass(C["kind"], C["y"], C["aux"], np.zeros(n), np.zeros(n),
                                    C["mask"])
    a1 = nr.dense_solve(C["F"], b, C["mask"], noise)
    return lr.newton_pass(C["kind"], C["y"], C["aux"], oracle.kron_matvec(C["F"], a1), a1,
                          C["mask"])[2]
