"""Dense NumPy restatement of the grid GP's marginal-likelihood gradient (test
infrastructure only, in the style of tests/masked_ref.py).

  dL/dtheta = 1/2 alpha^T dK alpha - 1/2 tr((K_oo + s I)^-1 dK_oo),
  alpha_o = (K_oo + s I)^-1 y_o (0 at the missing points), dK = I for the noise

with K the Kronecker product of 1-D stationary factors.  Here stand: the
analytic d k / d theta of the four kinds (float64 and np.longdouble, with the
elementwise bound the device test asserts), the dense LML and its gradient on
a complete or masked grid, the Kronecker-sum form of the trace that
gg_kron_trace_ratio streams, its long-double reference, and the probe
estimator of linalg.trace_grad on oracle.cg.probe_signs.

Factor lists are in KronMatrix order: GridKernel.cov_grid reverses the
dimensions, so dimension i of the model is factor d - 1 - i here and the flat
grid index has dimension 0 fastest.
"""
import math

import numpy as np

import oracle
from oracle.cg import probe_signs

import grief_abi_ref as R
import masked_ref as MR

LD = np.longdouble
U53 = R.U53
KINDS = R.KINDS


# ------------------------------------------------- d k / d theta, elementwise
def _dls(kind, var, ls, d2, dt):
    """(d k / d lengthscale, t) from squared distances in the float type dt,
    in the device's operation order; t as grief_abi_ref._cov (the magnitude of
    the exponent's argument)."""
    kind = R._kind(kind)
    var, ls = dt(var), dt(ls)
    if kind == "RBF":
        if ls < 1e-6:
            return np.zeros_like(d2), np.zeros_like(d2)
        r2 = d2 / (ls * ls)
        return var * np.exp(-dt(0.5) * r2) * (r2 / ls), r2 / 2
    if kind == "Exponential":
        r = np.sqrt(d2) / ls
        return var * np.exp(-r) * (r / ls), r
    if kind == "Matern32":
        r = np.sqrt(d2) / ls
        t = np.sqrt(dt(3)) * r
        return var * (dt(3) * r * r / ls) * np.exp(-t), t
    r2 = d2 / (ls * ls)
    r = np.sqrt(r2)
    t = np.sqrt(dt(5)) * r
    return var * ((dt(5) / 3) * r2 / ls) * (1 + t) * np.exp(-t), t


def grad_param_ref(kind, var, ls, x, z, which, dt=LD):
    """(d k / d theta, t), n x m in the float type dt, for x: n x D, z: m x D;
    which 0 = variance (k at unit variance), 1 = lengthscale."""
    d2 = R._d2(x, z, dt)
    if which == 0:
        return R._cov(kind, 1.0, ls, d2, dt)
    return _dls(kind, var, ls, d2, dt)


def grad_param_bound(D, ref, t):
    """|got - ref| <= (D + 12)(1 + t) u |ref| + TINY: grief_abi_ref.cov_bound's
    count (D FMAs for d2, the roundings that form the exponent's argument --
    amplified by t --, exp at 1 ulp, the polynomial, the variance) plus the
    derivative's own operations, at most four: the scale by r or r^2 (one or
    two multiplies, the Matern52 constant 5 / 3), the division by the
    lengthscale and the product with the rest.  The variance derivative is k at
    unit variance and lies inside cov_bound itself."""
    return (D + 12) * (1 + t) * U53 * np.abs(ref) + R.TINY


def dk_1d(kind, g, var, ls):
    """{'variance', 'lengthscale'}: m x m float64 derivatives of
    oracle.cov_1d(kind, g, g, var, ls)."""
    g = np.asarray(g, dtype=np.float64).reshape(-1, 1)
    return {'variance': grad_param_ref(kind, var, ls, g, g, 0, np.float64)[0],
            'lengthscale': grad_param_ref(kind, var, ls, g, g, 1, np.float64)[0]}


# ----------------------------------------------------------------- the problem
class Problem(object):
    """A d-dimensional grid GP: dimension i has m_i points on linspace(0, 1),
    kernel kinds[i] with variance var[i] and lengthscale ls[i]; only kernel 0's
    variance is a free parameter (GridKernel fixes the others).

    params = [noise, var_0, ls_0, var_1, ls_1, ...] (the model's order);
    F: factors in KronMatrix order with the jitter; dF[k] = (position, d K_f /
    d theta) for kernel parameter k."""

    def __init__(self, ms, kinds, ls, s=0.01, var=None, jitter=1e-12, seed=0, missing=0):
        self.ms, self.kinds = tuple(ms), tuple(kinds)
        self.d = len(ms)
        self.ls = [float(v) for v in ls]
        self.var = [1.0] * self.d if var is None else [float(v) for v in var]
        self.s, self.jitter = float(s), float(jitter)
        self.xg = [np.linspace(0.0, 1.0, m).reshape(-1, 1) for m in ms]
        self.N = int(np.prod(ms))
        rng = np.random.default_rng(seed)
        # dimension 0 fastest: the model's flat grid order
        mesh = np.meshgrid(*[g[:, 0] for g in self.xg[::-1]], indexing='ij')
        f = sum(np.sin(3.0 * (i + 1) * c) for i, c in enumerate(mesh[::-1]))
        self.y = (f.reshape(-1) + 0.1 * rng.standard_normal(self.N)).reshape(-1, 1)
        self.mask = None
        if missing:
            miss = np.random.default_rng(seed + 1).choice(self.N, size=missing, replace=False)
            self.mask = np.ones(self.N, dtype=bool)
            self.mask[miss] = False
        self.free = np.array([True] + [i == 0 or j == 1 for i in range(self.d)
                                       for j in range(2)])

    @property
    def params(self):
        p = [self.s]
        for v, l in zip(self.var, self.ls):
            p += [v, l]
        return np.array(p)

    def at(self, params):
        """A copy of the problem at another parameter vector."""
        q = Problem.__new__(Problem)
        q.__dict__.update(self.__dict__)
        q.s = float(params[0])
        q.var = [float(v) for v in params[1::2]]
        q.ls = [float(v) for v in params[2::2]]
        return q

    def factors(self):
        F = [oracle.cov_1d(k, g, g, v, l) + self.jitter * np.eye(g.shape[0])
             for k, g, v, l in zip(self.kinds, self.xg, self.var, self.ls)]
        return F[::-1]

    def dfactors(self):
        out = []
        for i, (k, g, v, l) in enumerate(zip(self.kinds, self.xg, self.var, self.ls)):
            dk = dk_1d(k, g, v, l)
            out += [(self.d - 1 - i, dk['variance']), (self.d - 1 - i, dk['lengthscale'])]
        return out

    def kernels(self, gg):
        """The gp_grief_amd.kern list of this problem (a fresh GridKernel's input)."""
        return [getattr(gg.kern, k)(1, variance=v, lengthscale=l)
                for k, v, l in zip(self.kinds, self.var, self.ls)]


def mixed_problem(ms, missing=0, s=0.01):
    """RBF / Matern32 / Matern52 factors, lengthscales 0.2, 0.25, 0.3: the
    setup of the issue's CPU check, away from the optimum for the data."""
    return Problem(ms, ("RBF", "Matern32", "Matern52"), (0.2, 0.25, 0.3), s=s, missing=missing)


# ------------------------------------------------------------ dense LML / grad
def _observed(p):
    return np.arange(p.N) if p.mask is None else np.nonzero(p.mask)[0]


def dense_A(p):
    """K_oo + s I."""
    o = _observed(p)
    return MR.dense_K(p.factors())[np.ix_(o, o)] + p.s * np.eye(o.size)


def replaced(F, pos, dKf):
    G = list(F)
    G[pos] = dKf
    return G


def dense_lml(p):
    o = _observed(p)
    A = dense_A(p)
    yo = p.y[o, 0]
    return float(-0.5 * (yo.dot(np.linalg.solve(A, yo)) + np.linalg.slogdet(A)[1]
                         + o.size * np.log(2 * np.pi)))


def dense_parts(p):
    """(fit, traces): fit[k] = 1/2 alpha^T dK_k alpha and traces[k] =
    tr(A^-1 dK_k,oo) over the full parameter vector (k = 0 the noise); the
    gradient is fit - traces / 2."""
    o = _observed(p)
    F = p.factors()
    Ainv = np.linalg.inv(dense_A(p))
    alpha = Ainv.dot(p.y[o, 0])
    fit, tr = [0.5 * alpha.dot(alpha)], [np.trace(Ainv)]
    for pos, dKf in p.dfactors():
        dK = MR.dense_K(replaced(F, pos, dKf))[np.ix_(o, o)]
        fit.append(0.5 * alpha.dot(dK.dot(alpha)))
        tr.append(float(np.sum(Ainv * dK)))
    return np.array(fit), np.array(tr)


def dense_grad(p):
    fit, tr = dense_parts(p)
    return fit - 0.5 * tr


def central_diff_grad(p, rel_step=1e-5):
    """Central differences of dense_lml over the free parameters (0 elsewhere)."""
    g = np.zeros(p.params.size)
    for k in np.nonzero(p.free)[0]:
        h = rel_step * p.params[k]
        a, b = p.params.copy(), p.params.copy()
        a[k] += h
        b[k] -= h
        g[k] = (dense_lml(p.at(a)) - dense_lml(p.at(b))) / (2 * h)
    return g


def forward_diff_grad(p, step=1e-6):
    """BaseModel._finite_diff_gradient's forward differences, on dense_lml."""
    g = np.zeros(p.params.size)
    base = dense_lml(p)
    for k in np.nonzero(p.free)[0]:
        a = p.params.copy()
        a[k] += step
        g[k] = (dense_lml(p.at(a)) - base) / step
    return g


# ------------------------------------------------------- Kronecker-sum traces
def trace_rows(p):
    """(lam, rows): per-factor eigenvalues and the numerator rows of
    gg_kron_trace_ratio over the full parameter vector -- all ones for the
    noise; diag(Q_f^T dK_f Q_f) in the parameter's factor and lam elsewhere."""
    Q, lam = MR.factor_eigh(p.factors())
    rows = [[np.ones_like(l) for l in lam]]
    for pos, dKf in p.dfactors():
        row = list(lam)
        row[pos] = np.einsum('ij,ij->j', Q[pos], dKf.dot(Q[pos]))
        rows.append(row)
    return lam, rows


def kron_traces(p):
    """tr((K + s I)^-1 dK_k) of the complete grid as the grid sum of
    prod_f num_f / (prod_f lam_f + s)."""
    lam, rows = trace_rows(p)
    den = MR.kron_eigs(lam) + p.s
    return np.array([np.sum(MR.kron_eigs(row) / den) for row in rows])


def trace_ratio_ref(ms, lam, num, shift):
    """(values, scales) of gg_kron_trace_ratio in np.longdouble: lam a vector
    of sum(ms) entries, num P rows of them; scales[p] = sum_g |term|."""
    off = np.concatenate([[0], np.cumsum(ms)])
    den = np.ones(1, dtype=LD)
    for f in range(len(ms)):
        den = np.kron(den, np.asarray(lam[off[f]:off[f + 1]], dtype=LD))
    den = den + LD(shift)
    vals, scales = [], []
    for row in np.atleast_2d(num):
        t = np.ones(1, dtype=LD)
        for f in range(len(ms)):
            t = np.kron(t, np.asarray(row[off[f]:off[f + 1]], dtype=LD))
        t = t / den
        if t.size <= 1 << 16:
            # exact sum of the float64 roundings' neighbours is not needed:
            # fsum over the long doubles' float64 head and tail
            hi = t.astype(np.float64)
            lo = (t - hi).astype(np.float64)
            vals.append(LD(math.fsum(hi)) + LD(math.fsum(lo)))
        else:
            vals.append(np.sum(t))
        scales.append(np.sum(np.abs(t)))
    return np.array(vals, dtype=LD), np.array(scales, dtype=LD)


def trace_ratio_bound(d, scales, chain=16):
    """|got - ref| <= (2 d + 66) u sum|term|: 2 d + 2 for one term (d - 2
    products each for the head's eigenvalues and numerators, the FMA that forms
    the denominator, the reciprocal, the last numerator's product and the
    product with the reciprocal) and 64 for the sums -- a thread's chain of at
    most `chain` additions, 6 shuffle levels and 4 waves per block, then per
    row 2 partials per thread, 6 levels and 16 waves: chain + 34.  A chain
    beyond 30 (a grid-stride pass over whole runs of a long last factor) widens
    the 64 to chain + 34."""
    return (2 * d + 2 + max(64, chain + 34)) * U53 * np.asarray(scales, dtype=LD)


def trace_ratio_chain(ms, threads=2048 * 256, items_fill=131072, seg_min=16, seg_max=128):
    """The longest chain of additions one thread of gg_kron_trace_ratio runs
    for the grid ms (its launch geometry, gg_diag.hip): segment length times
    grid-stride passes."""
    ml = int(ms[-1])
    nhead = int(np.prod(ms)) // ml
    want = -(-items_fill // nhead)
    seg = min(max(-(-ml // want), min(ml, seg_min)), seg_max)
    items = nhead * -(-ml // seg)
    nthreads = min(threads, -(-items // 256) * 256)
    return seg * -(-items // nthreads)


# --------------------------------------------------------------- probe traces
def probe_estimates(p, seed, probes=None, Z=None):
    """per_probe of linalg.trace_grad in dense NumPy: row j from z_j =
    probe_signs(seed, j, N) * mask (or column j of Z), columns [z^T A^-1 z,
    (A^-1 z)^T W dK_k W z for every kernel parameter k]."""
    o = _observed(p)
    F = p.factors()
    Ainv = np.linalg.inv(dense_A(p))
    dKs = [MR.dense_K(replaced(F, pos, dKf))[np.ix_(o, o)] for pos, dKf in p.dfactors()]
    if Z is None:
        Z = np.stack([probe_signs(seed, j, p.N) for j in range(probes)], axis=1)
    per = np.empty((Z.shape[1], 1 + len(dKs)))
    absper = np.empty_like(per)
    for j in range(Z.shape[1]):
        z = Z[o, j]
        x = Ainv.dot(z)
        per[j, 0] = z.dot(x)
        absper[j, 0] = np.abs(z).dot(np.abs(x))
        for k, dK in enumerate(dKs):
            per[j, 1 + k] = x.dot(dK.dot(z))
            absper[j, 1 + k] = np.abs(x).dot(np.abs(dK).dot(np.abs(z)))
    return per, absper
