"""Plain np.longdouble restatement of the Kronecker operator section of the C
ABI (gg_kron_matvec, gg_kron_block_matvec): test infrastructure only, NumPy
only, no BLAS (long double einsum runs NumPy's own loops).

Next to each reference stands the magnitude vector the elementwise bound of
tests/test_gpu_kron_abi.py scales with, and the seeded operators both test
modules share.  tests/test_kron_abi_ref.py checks on the host that NumPy's own
float64 chain (oracle.kron_matvec, oracle.kron_matvec_T,
oracle.kron.block_matvec) meets every bound: neither vacuous nor too tight.

The bound (u = 2^-53), elementwise:

    |got - ref| <= c u mag + 2 u |shift| |x|

Grid basis.  The operator is applied as d stages, stage k one dense product
with the applied factor F_k (p_k x q_k; F_k^T for the transposed operator)
along one axis.  mag = (G_0 (x) ... (x) G_{d-1}) |x| with G_k = |F_k|, or
G_k = |F_k| + |F_k| J (J the index reversal of the contracted axis) where
gg_kron_fold_mask reports the centrosymmetric split for the axis.

  * plain stage: every output is a sum of q_k products accumulated in some
    order, with or without FMA.  Each term passes through at most q_k
    roundings (its product, then at most q_k - 1 additions), so the stage
    multiplies the running error factor by at most (1 + u)^(q_k):
    contributes q_k.
  * split stage (even / odd halves): the input is pre-added,
    e_i = x_i + x_(m-1-i), o_i = x_i - x_(m-1-i) (one rounding, relative to
    |x_i| + |x_(m-1-i)|: the J term of G_k); the half-order matrices
    (F[j][i] +- F[j][m-1-i]) / 2 are formed on the host in float64 (one
    rounding, the halving is exact); two sums of at most ceil(m / 2) <= q_k
    products; the epilogue recombines S +- T (one rounding).  Contributes at
    most q_k + 3.  (The factors of the test operators are centrosymmetric to
    the bit, so the library's symmetrised (F + J F J) / 2 is F itself.)
  * the last stage's epilogue y = acc + shift x is one fma: one rounding of
    the whole (1 more on the mag term, u |shift| |x| on the shift term; the
    bound's 2 u |shift| |x| leaves one spare).
  * one more unit covers the long double reference's own rounding
    (2^-64 sum q_k, far below u) and the second-order terms of
    (1 + u)^c - 1 <= c u / (1 - c u), c u < 1e-12 here.

So, with the + 3 taken on every stage (one formula for both kinds):

    c = sum_k (q_k + 3) + 2.

Block basis (gg_kron_block_matvec): block beta is the Kronecker product of
the half-order matrices S_k (beta_k = 0) or T_k (beta_k = 1), S = F[j][i] +
F[j][m-1-i], T = F[j][i] - F[j][m-1-i], h_k x h_k, formed on the host in
float64 (one rounding each).  mag_b = (|S or T|_0 (x) ...) |x_b| per block in
the layout of oracle.kron.block_fold; zero padding contributes exact zeros.
Each stage: h_k products (q_k = h_k) + 1 for the formed entry; the pair
launch keeps its intermediate in registers (no extra rounding).  The same
formula with q_k = h_k:

    c_b = sum_k (h_k + 3) + 2.

Neither constant is tuned: a case over its bound is a missing term in this
derivation or a bug in the kernel.
"""
import numpy as np

from oracle import kron as okron

LD = np.longdouble
U53 = 2.0 ** -53


# ------------------------------------------------------------ the references
def _chain(factors, x):
    """(F_0 (x) ... (x) F_{d-1}) x in the dtype of x: per factor one einsum
    that contracts the slowest remaining axis and appends the new one as the
    fastest (the axis rotation of oracle.kron_matvec)."""
    y = x.reshape(-1)
    for F in factors:
        p, q = F.shape
        y = np.einsum("ji,ib->bj", F, y.reshape(q, -1)).reshape(-1)
    return y


def applied_factors(factors, transpose=False):
    return [np.asarray(F, dtype=np.float64).T if transpose else np.asarray(F, dtype=np.float64)
            for F in factors]


def fold_mask(factors, transpose=False, fold_min=48):
    """The mask gg_kron_fold_mask reports at the default switches: bit k for a
    square factor of order fold_min..256 that is centrosymmetric within
    16 eps max|F| (gg_kron.hip pack_fold)."""
    mask = 0
    for k, F in enumerate(applied_factors(factors, transpose)):
        m = F.shape[0]
        if F.shape[0] != F.shape[1] or m < fold_min or m > 256:
            continue
        amax = np.max(np.abs(F))
        if amax > 0 and np.max(np.abs(F - F[::-1, ::-1])) <= 16 * 2.220446049250313e-16 * amax:
            mask |= 1 << k
    return mask


def matvec_ref(factors, x, transpose=False, shift=0.0, mask=0):
    """(ref, mag): ref = (F_0 (x) ... )^{T?} x + shift x in long double and
    mag = (G_0 (x) ... ) |x| (module docstring; bit k of mask = axis k split)."""
    Fs = applied_factors(factors, transpose)
    xl = np.asarray(x, dtype=LD).reshape(-1)
    ref = _chain([F.astype(LD) for F in Fs], xl)
    if shift != 0.0:
        ref = ref + LD(shift) * xl
    Gs = []
    for k, F in enumerate(Fs):
        G = np.abs(F).astype(LD)
        if (mask >> k) & 1:
            G = G + G[:, ::-1]
        Gs.append(G)
    return ref, _chain(Gs, np.abs(xl))


def matvec_c(factors, transpose=False):
    """c = sum_k (q_k + 3) + 2 (module docstring)."""
    return sum(F.shape[1] + 3 for F in applied_factors(factors, transpose)) + 2


def matvec_bound(factors, x, mag, transpose=False, shift=0.0):
    xa = np.abs(np.asarray(x, dtype=LD).reshape(-1))
    b = matvec_c(factors, transpose) * U53 * np.asarray(mag, dtype=LD)
    return b + 2 * U53 * abs(shift) * xa if shift != 0.0 else b


def block_perm(ms, pad):
    """pos[i] = the block-layout position of element i of the C-order
    (2^d, e_0, .., e_{d-1}) array: oracle.kron.slab_tile applied to the
    positions themselves (the layout is the oracle's, not restated here)."""
    es = okron.block_extents(ms, pad)
    n = (1 << len(ms)) * int(np.prod(es))
    tiled = okron.slab_tile(np.arange(n, dtype=np.float64), es)   # tiled[pos[i]] = i
    pos = np.empty(n, dtype=np.int64)
    pos[tiled.astype(np.int64)] = np.arange(n)
    return pos, es


def block_pad_mask(ms, pad=True):
    """Boolean over the block layout: True at the zero-padding positions."""
    pos, es = block_perm(ms, pad)
    d = len(ms)
    hs = [int(m) // 2 for m in ms]
    real = np.zeros((1 << d,) + tuple(es), dtype=bool)
    real[(slice(None),) + tuple(slice(0, h) for h in hs)] = True
    out = np.empty(pos.size, dtype=bool)
    out[pos] = ~real.reshape(-1)
    return out


def block_matvec_ref(factors, xb, shift=0.0, pad=True, blk0=0, nblk=None):
    """(ref, mag) of (P K P^T + shift I) x_b in the block layout of
    oracle.kron.block_fold (pad: the device layout), long double; blocks
    [blk0, blk0 + nblk) only when nblk is given (xb holds just them)."""
    ms = [np.shape(F)[0] for F in factors]
    d = len(ms)
    hs = [m // 2 for m in ms]
    pos, es = block_perm(ms, pad)
    nb = int(np.prod(es))
    if nblk is None:
        blk0, nblk = 0, 1 << d
    pos = pos[blk0 * nb:(blk0 + nblk) * nb] - blk0 * nb
    st = []
    for F, h, e in zip(factors, hs, es):
        Fl = np.asarray(F, dtype=LD)
        Fr = Fl[:h, ::-1][:, :h]
        S, T = np.zeros((e, e), dtype=LD), np.zeros((e, e), dtype=LD)
        S[:h, :h], T[:h, :h] = Fl[:h, :h] + Fr, Fl[:h, :h] - Fr
        st.append((S, T))
    xl = np.asarray(xb, dtype=LD).reshape(-1)
    xc = xl[pos]                                   # C order over (block, e_0 .. e_{d-1})
    ref, mag = np.empty_like(xc), np.empty_like(xc)
    for b in range(nblk):
        B = blk0 + b
        fs = [st[k][(B >> (d - 1 - k)) & 1] for k in range(d)]
        seg = xc[b * nb:(b + 1) * nb]
        ref[b * nb:(b + 1) * nb] = _chain(fs, seg)
        mag[b * nb:(b + 1) * nb] = _chain([np.abs(f) for f in fs], np.abs(seg))
    out, outm = np.empty_like(ref), np.empty_like(mag)
    out[pos], outm[pos] = ref, mag
    if shift != 0.0:
        out = out + LD(shift) * xl
    return out, outm


def block_c(factors):
    """c_b = sum_k (h_k + 3) + 2 (module docstring)."""
    return sum(np.shape(F)[0] // 2 + 3 for F in factors) + 2


def block_bound(factors, xb, mag, shift=0.0):
    b = block_c(factors) * U53 * np.asarray(mag, dtype=LD)
    if shift != 0.0:
        b = b + 2 * U53 * abs(shift) * np.abs(np.asarray(xb, dtype=LD).reshape(-1))
    return b


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0; NaN or a miss of a zero
    bound as inf)."""
    err = np.abs(np.asarray(got, dtype=LD).reshape(-1) - np.asarray(ref, dtype=LD).reshape(-1))
    bound = np.asarray(bound, dtype=LD).reshape(-1)
    if np.any(np.isnan(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------ shared operators
_cache = {}


def _frozen(key, make):
    if key not in _cache:
        vals = make()
        for v in vals:
            for a in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key] = vals
    return _cache[key]


def centro(A):
    """(A + J A J) / 2: centrosymmetric to the bit (the sum is commutative,
    the halving exact)."""
    A = np.asarray(A, dtype=np.float64)
    return 0.5 * (A + A[::-1, ::-1])


# name -> (shapes, kind): "dense" random factors; "centro_sym" symmetric and
# centrosymmetric; "centro" centrosymmetric, not symmetric
MATVEC_CASES = {
    "1x1": ([(1, 1)], "dense"),
    "5x3": ([(5, 3)], "dense"),
    "1x7_7x1": ([(1, 7), (7, 1)], "dense"),
    "growing": ([(17, 3), (9, 2)], "dense"),
    "shrinking": ([(3, 17), (2, 9)], "dense"),
    "mixed3": ([(13, 17), (5, 3), (33, 31)], "dense"),
    "2x2_12": ([(2, 2)] * 12, "dense"),
    "two_launch": ([(257, 255), (6, 2)], "dense"),
    "t4_tail": ([(200, 200), (3, 3)], "dense"),
    "centro_48_7_49": ([(48, 48), (7, 7), (49, 49)], "centro_sym"),
    "centro_nonsym": ([(50, 50), (3, 3), (49, 49)], "centro"),
}
# the mask gg_kron_fold_mask must report (both orientations), default switches
MATVEC_MASKS = {"centro_48_7_49": 0b101, "centro_nonsym": 0b101}


def matvec_case(name):
    """(factors, x_forward, x_transposed) of a named case, seeded."""
    shapes, kind = MATVEC_CASES[name]

    def make():
        rng = np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(name)))
        fs = []
        for p, q in shapes:
            A = rng.standard_normal((p, q))
            if kind == "centro_sym":
                A = centro(A + A.T)
            elif kind == "centro":
                A = centro(A)
            fs.append(np.ascontiguousarray(A / np.sqrt(q)))
        n_in = int(np.prod([q for _, q in shapes]))
        n_out = int(np.prod([p for p, _ in shapes]))
        return fs, rng.standard_normal(n_in), rng.standard_normal(n_out)
    return _frozen(("mv", name), make)


def toeplitz_factors(ms, rho0=0.3):
    """Symmetric Toeplitz factors rho_k^|i - j| (rho_k = rho0 + 0.03 k): SPD,
    eigenvalues inside [(1 - rho) / (1 + rho), (1 + rho) / (1 - rho)], and
    centrosymmetric to the bit (a function of |i - j| alone)."""
    def make():
        out = []
        for k, m in enumerate(ms):
            i = np.arange(int(m))
            out.append(np.ascontiguousarray(
                np.power(rho0 + 0.03 * k, np.abs(i[:, None] - i[None, :]).astype(np.float64))))
        return (out,)
    return _frozen(("toep", tuple(int(m) for m in ms), rho0), make)[0]


BLOCK_OPS = [(40, 40), (4, 40, 40), (2, 6, 40, 40), (4, 64, 64)]


def vector(n, seed):
    return _frozen(("vec", int(n), int(seed)),
                   lambda: (np.random.default_rng(seed).standard_normal(int(n)),))[0]
