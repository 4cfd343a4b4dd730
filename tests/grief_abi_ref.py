"""Plain np.longdouble restatement of the GRIEF basis section of the C ABI
(gg_cov, gg_grief_tables*, gg_grief_phi, gg_expand_skc): test infrastructure
only, NumPy only.

Next to each reference stand the elementwise error bound the device tests
assert (u = 2^-53; derived in tests/test_gpu_grief_abi.py), the same operation
evaluated by NumPy in float64 (tests/test_grief_abi_ref.py checks that it meets
every bound: the bounds are neither vacuous nor too tight), and the seeded
inputs both test modules share.
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
KINDS = ("RBF", "Exponential", "Matern32", "Matern52")


def _kind(kind):
    return KINDS[kind] if isinstance(kind, (int, np.integer)) else kind


def _cov(kind, var, ls, d2, dt):
    """(k, t) from squared distances d2 in the float type dt."""
    kind = _kind(kind)
    assert kind in KINDS
    var, ls = dt(var), dt(ls)
    if kind == "RBF":
        if ls < 1e-6:                       # the delta rule (stationary.py:108-134)
            return var * (d2 == 0).astype(dt), np.zeros_like(d2)
        t = d2 / (2 * ls * ls)
        return var * np.exp(-t), t
    r = np.sqrt(d2) / ls
    if kind == "Exponential":
        return var * np.exp(-r), r
    if kind == "Matern32":
        t = np.sqrt(dt(3)) * r
        return var * (1 + t) * np.exp(-t), t
    t = np.sqrt(dt(5)) * r
    return var * (1 + t + (dt(5) / 3) * (d2 / (ls * ls))) * np.exp(-t), t


def _d2(x, z, dt):
    x = np.asarray(x, dtype=dt)
    z = np.asarray(z, dtype=dt)
    x = x.reshape(x.shape[0], -1)
    z = z.reshape(z.shape[0], -1)
    d2 = np.zeros((x.shape[0], z.shape[0]), dtype=dt)
    for k in range(x.shape[1]):
        t = x[:, k:k + 1] - z[:, k].reshape(1, -1)
        d2 += t * t
    return d2


def cov_ref(kind, var, ls, x, z):
    """(k, t), both n x m long double, for x: n x D and z: m x D; t is the
    magnitude of the exponent's argument (RBF d2 / (2 l^2), Exponential r,
    Matern32 sqrt(3) r, Matern52 sqrt(5) r; 0 for the delta RBF, l < 1e-6)."""
    return _cov(kind, var, ls, _d2(x, z, LD), LD)


def cov_f64(kind, var, ls, x, z):
    return _cov(kind, var, ls, _d2(x, z, np.float64), np.float64)[0]


TINY = LD(2.0) ** -1072      # four spacings of float64's subnormals


def cov_bound(D, ref, t):
    """|got - ref| <= (D + 8)(1 + t) u |ref| + TINY.  The relative part is the
    bound proper; TINY covers gradual underflow alone (a float64 below 2^-1022
    is rounded to a multiple of 2^-1074 by exp, once more by the polynomial
    and by the variance, |var| <= 2) and is invisible for any normal result."""
    return (D + 8) * (1 + t) * U53 * np.abs(ref) + TINY


def tables_ref(kind, var, ls, x, xg, qsel):
    """(X, A): X = qsel @ k(xg, x) (u x n) and the majorant
    A = |qsel| @ (|k| (1 + t)), long double."""
    k, t = cov_ref(kind, var, ls, np.asarray(xg).reshape(-1, 1), np.asarray(x).reshape(-1, 1))
    q = np.asarray(qsel, dtype=LD)
    return q @ k, np.abs(q) @ (np.abs(k) * (1 + t))


def tables_f64(kind, var, ls, x, xg, qsel):
    k = cov_f64(kind, var, ls, np.asarray(xg).reshape(-1, 1), np.asarray(x).reshape(-1, 1))
    return np.asarray(qsel, dtype=np.float64) @ k


def tables_bound(m, A):
    """|got - X| <= (mp + 17) u A, mp = 16 ceil(m / 16)."""
    return (16 * ((m + 15) // 16) + 17) * U53 * A


def phi_ref(T, cidx, log_lam):
    """Phi[a][j] = prod_f T[a][cidx[j][f]] * exp(-log_lam[j] / 2), long double,
    for an n x U value table T."""
    T = np.asarray(T, dtype=LD)
    cidx = np.asarray(cidx)
    out = np.exp(-np.asarray(log_lam, dtype=LD) / 2).reshape(1, -1) * np.ones((T.shape[0], 1), LD)
    for f in range(cidx.shape[1]):
        out = out * T[:, cidx[:, f]]
    return out


def phi_f64(T, cidx, log_lam):
    T = np.asarray(T, dtype=np.float64)
    out = np.exp(-0.5 * np.asarray(log_lam, dtype=np.float64)).reshape(1, -1) * np.ones(
        (T.shape[0], 1))
    for f in range(cidx.shape[1]):
        out = out * T[:, cidx[:, f]]
    return out


def phi_bound(d, ref):
    """|got - ref| <= (3 d + 4) u |ref|."""
    return (3 * d + 4) * U53 * np.abs(ref)


def log_tables(T):
    """The (L, S) form of a value table as a caller builds it in float64:
    L = log|T|, S = sign(T), and L = 0, S = 0 where T == 0."""
    T = np.asarray(T, dtype=np.float64)
    S = np.sign(T)
    with np.errstate(divide="ignore"):
        L = np.where(T == 0, 0.0, np.log(np.abs(np.where(T == 0, 1.0, T))))
    L = np.where(np.isnan(T), np.nan, L)
    return L, S


def log_tables_value(L, S):
    """The value table an (L, S) pair stands for, S exp(L), in long double."""
    return np.asarray(S, dtype=LD) * np.exp(np.asarray(L, dtype=LD))


def expand_skc_ref(X, cidx, logged):
    """tensors.py:97-128 for stacked unique rows X (U x n) and cidx (p x d):
    logged -> (sum_f log|X[c_jf]|, prod_f sign(X[c_jf]) as int32, B) with the
    sign taken before the zeros are replaced and a zero counted as log 1, B =
    sum_f (1 + |log|v_f||) the magnitude the bound scales with; else the plain
    product.  Long double, p x n."""
    X = np.asarray(X, dtype=LD)
    cidx = np.asarray(cidx)
    p, n = cidx.shape[0], X.shape[1]
    if not logged:
        out = np.ones((p, n), dtype=LD)
        for f in range(cidx.shape[1]):
            out = out * X[cidx[:, f], :]
        return out
    out, B = np.zeros((p, n), dtype=LD), np.zeros((p, n), dtype=LD)
    sign = np.ones((p, n), dtype=np.int32)
    for f in range(cidx.shape[1]):
        v = X[cidx[:, f], :]
        sign = sign * np.int32(np.sign(v))
        lg = np.log(np.abs(np.where(v == 0, LD(1), v)))
        out = out + lg
        B = B + 1 + np.abs(lg)
    return out, sign, B


def expand_skc_f64(X, cidx, logged):
    X = np.asarray(X, dtype=np.float64)
    p, n = cidx.shape[0], X.shape[1]
    if not logged:
        out = np.ones((p, n))
        for f in range(cidx.shape[1]):
            out = out * X[cidx[:, f], :]
        return out
    out = np.zeros((p, n))
    sign = np.ones((p, n), dtype=np.int32)
    for f in range(cidx.shape[1]):
        v = X[cidx[:, f], :]
        sign = sign * np.int32(np.sign(v))
        out = out + np.log(np.abs(np.where(v == 0, 1.0, v)))
    return out, sign


def expand_bound(d, ref=None, B=None):
    """not logged: (d + 1) u |ref|; logged: 2 (d + 1) u sum_f (1 + |log|v_f||)."""
    if B is None:
        return (d + 1) * U53 * np.abs(ref)
    return 2 * (d + 1) * U53 * B


def kr_ref(blocks, c):
    """(out, mag): out[j] = sum_g c[g] prod_f U_f[j][g_f] (factor 0 slowest) and
    mag = sum_g |c_g| prod_f |U_f|, contracted factor by factor in long double."""
    def run(bl, cc):
        M = bl[0].shape[0]
        t = np.broadcast_to(np.asarray(cc, dtype=LD).reshape(1, -1), (M, cc.size))
        for b in reversed(bl):                      # the fastest factor first
            m = b.shape[1]
            t = (t.reshape(M, -1, m) * np.asarray(b, dtype=LD)[:, None, :]).sum(-1)
        return t.reshape(M)
    return run(blocks, c), run([np.abs(b) for b in blocks], np.abs(c))


# ------------------------------------------------------------ shared inputs
_cache = {}


def _frozen(key, make):
    if key not in _cache:
        vals = make()
        for v in vals:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = vals
    return _cache[key]


def cov_problem(kind, D, ls, nx, nz, var=1.3):
    """x (nx x D), z (nz x D) uniform in [0, 1), a known out0, and (k, t)."""
    def make():
        rng = np.random.default_rng(7919 * nx + 31 * nz + D)
        x, z = rng.random((nx, D)), rng.random((nz, D))
        out0 = rng.uniform(-2.0, 2.0, (nx, nz))
        return (x, z, out0) + cov_ref(kind, var, ls, x, z)
    return _frozen(("cov", _kind(kind), D, ls, nx, nz, var), make)


def orth_rows(m, u, seed):
    """u rows of a random m x m orthogonal matrix."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))
    return np.ascontiguousarray(q[:u, :])


def tables_problem(kind, ls, m, u, n, var=0.7, zero_row=None):
    """x (n) in [0, 1), xg = linspace(0, 1, m), qsel (u x m; row `zero_row`
    exactly zero), and (X, A)."""
    def make():
        rng = np.random.default_rng(104729 * m + 1009 * u + n)
        x = rng.random(n)
        xg = np.linspace(0.0, 1.0, m)
        q = orth_rows(m, u, 13 * m + u)
        if zero_row is not None:
            q[zero_row, :] = 0.0
        return (x, xg, q) + tables_ref(kind, var, ls, x, xg, q)
    return _frozen(("tab", _kind(kind), ls, m, u, n, var, zero_row), make)


def phi_problem(d, U, p, n):
    """A value table (n x U, uniform in [-2, 2], a few exact zeros in columns
    that are used, NaN in the columns no cidx entry names), cidx (p x d int32),
    log_lam in [-30, 5]."""
    def make():
        rng = np.random.default_rng(65537 * d + 257 * U + 17 * p + n)
        T = rng.uniform(-2.0, 2.0, (n, U))
        cidx = rng.integers(0, U, (p, d)).astype(np.int32)
        used = np.unique(cidx)
        for _ in range(3):
            T[rng.integers(0, n), used[rng.integers(0, used.size)]] = 0.0
        unused = np.setdiff1d(np.arange(U), used)
        T[:, unused] = np.nan
        return T, cidx, rng.uniform(-30.0, 5.0, p)
    return _frozen(("phi", d, U, p, n), make)


def expand_problem(d, p, n):
    """X (U x n, U = 2 d + 3) with one all-zero column and a few single zeros,
    cidx (p x d int32)."""
    def make():
        rng = np.random.default_rng(8191 * d + 127 * (p % 4099) + n)
        Ux = 2 * d + 3
        X = rng.standard_normal((Ux, n))
        X[:, n // 2] = 0.0
        for _ in range(3):
            X[rng.integers(0, Ux), rng.integers(0, n)] = 0.0
        return X, rng.integers(0, Ux, (p, d)).astype(np.int32)
    return _frozen(("skc", d, p, n), make)
