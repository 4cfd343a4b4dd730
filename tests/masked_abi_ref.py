"""Plain np.longdouble restatement of the masked CG / masked Lanczos section of
the C ABI (gg_cgm_*, gg_lanczos_probe_masked, _noise): test infrastructure
only, NumPy only.  The float64 restatements (masked_ref.masked_cg,
noise_ref.weighted_cg, masked_lanczos_ref.masked_lanczos,
noise_ref.weighted_lanczos) have long-double twins here -- the same
recurrences and the same stopping rule, the Kronecker product through
kron_abi_ref's long-double chain -- so a device iterate can be compared with
something that is not itself a float64 computation.

The first iterate and its bound (u = 2^-53).  With W = diag(mask), bt = W b,
A = W K W + s I (or W K W + D, D = diag(noise) on the observed set), the first
CG step from x0 = 0 is

    p = r0 = bt,  t = K p (+ s p),  rho = bt.bt,
    pq = p.t                      (scalar shift)
    pq = p.(K p) + sum_i d_i p_i^2  (noise),
    alpha = rho / pq,  x1 = alpha bt,  r1 = bt - alpha W (t + d o p).

What the device may differ by, term by term:

  * rho, and the noise sum S = sum d_i p_i^2, are sums of n non-negative
    terms.  Summed in any order, with or without fma, a term passes through at
    most n roundings (S: n + 1, the product d_i p_i is rounded first), so the
    computed value is within a relative g(n) = n u / (1 - n u) of the exact
    one (g(n + 1) for S).
  * the matvec is kron_abi_ref's: |t^_i - t_i| <= E_i = c u mag_i +
    2 u |s| |p_i|, c = sum_k (q_k + 3) + 2, mag = (|F_0| (x) ...) |p|, with the
    fold of a centrosymmetric factor in mag where gg_kron_fold_mask reports
    it.  Its dot epilogue sums the products p_i t^_i in any order:
        |pq^ - pq| <= e_pq = sum_i |p_i| E_i + g(n) sum_i |p_i| (|t_i| + E_i)
    (for the noise variant s = 0 there, S carries g(n + 1) S, and the one
    addition p.Kp + S adds u times their computed sum).
  * alpha^ = rho^ / pq^ is one more rounding: alpha^ lies in
        [rho (1 - g)(1 - u) / (pq + e_pq),  rho (1 + g)(1 + u) / (pq - e_pq)],
    d_alpha = the larger distance from alpha to an end (pq - e_pq > 0 is
    asserted).
  * x1_i = fma(alpha^, p_i, 0): one rounding.
        |x1^_i - x1_i| <= d_alpha |p_i| + u (alpha + d_alpha) |p_i|
  * r1_i = fma(-alpha^, t'_i, bt_i) at an observed point, t' = t^ (shift) or
    fma(d_i, p_i, t^_i) (noise: one more rounding, E'_i = E_i + u (|t_i| + E_i
    + d_i |p_i|)); one rounding of the result.  With a_hi = alpha + d_alpha,
        B_i = d_alpha |t'_i| + a_hi E'_i
        |r1^_i - r1_i| <= B_i + u (|r1_i| + B_i)
  * one more u |x1_i| and u (|bt_i| + alpha |t'_i|) covers the long-double
    reference's own rounding (its sums are pairwise: a few 2^-64) as the
    spare unit of kron_abi_ref's constant does for the matvec.

At a missing point x1 and r1 are exactly 0 and the bound is 0.  Nothing here
is tuned: a case over its bound is a missing term above or a bug in a kernel.
tests/test_masked_abi_ref.py shows float64 NumPy inside the bound at every
case tests/test_gpu_masked_abi.py uses.

The wrap cases.  vec_blocks(n) caps the grid of every streaming kernel of the
masked family at 2048 blocks of 256 lanes, each lane a pair of doubles on the
16-byte path: elements at flat index 2^20 and above belong to the second
grid-stride trip.  wrap_case puts at least a quarter of the observed points
there; wrap_figures measures what float64 NumPy itself loses against the long
double twins after 3 iterations / steps, the unit of the device tolerances.
"""
import numpy as np

import kron_abi_ref as R
import masked_lanczos_ref as ml
import masked_ref as mr
import noise_ref as nr
from oracle import cg as ocg

LD = np.longdouble
U53 = 2.0 ** -53
WRAP = 1 << 20                      # first flat index of the second trip
WRAP_SHAPES = [(103, 101, 101), (104, 101, 100)]
WRAP_ITERS = 3


def norm(v):
    return np.sqrt(np.sum(np.asarray(v, dtype=LD) ** 2))


def rel(a, b):
    """|a - b| / |b| in long double."""
    a = np.asarray(a, dtype=LD).reshape(-1)
    b = np.asarray(b, dtype=LD).reshape(-1)
    return float(norm(a - b) / max(norm(b), LD(1e-300)))


def max_rel(a, b):
    """max_j |a_j - b_j| / |b_j| (0 / 0 counts as 0)."""
    a = np.asarray(a, dtype=LD).reshape(-1)
    b = np.asarray(b, dtype=LD).reshape(-1)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, LD(0), d / np.abs(b))
    return float(np.max(r)) if r.size else 0.0


# ------------------------------------------------------------ the CG twins
def cg_ld(F, b, mask, shift=None, noise=None, rtol=1e-5, atol=0.0, maxiter=None, precond=None,
          pshift=None, dtype=LD):
    """(x, info, iters, |r|) of CG on (W K W + shift I) x = W b (noise None:
    masked_ref.masked_cg) or (W K W + D) x = W b (noise given:
    noise_ref.weighted_cg with its split p.Kp + sum d p^2), x0 = 0, in
    `dtype` arithmetic.  precond None or 'kron': z = W Q diag(1 / (lam +
    pshift)) Q^T r with the float64 eigenpairs of the factors taken as exact
    data (pshift: shift, or the geometric mean of the observed noise).  The
    stopping test is on the true |r|, seen after each update."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    FL = [np.asarray(f, dtype=np.float64).astype(dtype) for f in F]
    bt = np.where(mask, np.asarray(b, dtype=np.float64).reshape(-1), 0.0).astype(dtype)
    n = bt.size
    d = None
    if noise is not None:
        d = np.where(mask, np.asarray(noise, dtype=np.float64).reshape(-1), 0.0).astype(dtype)
    else:
        shift = dtype(shift)
    if maxiter is None:
        maxiter = 10 * n
    bnorm = norm(bt).astype(dtype)
    tol = max(dtype(atol), dtype(rtol) * bnorm)
    x = np.zeros(n, dtype=dtype)
    if bnorm == 0:
        return x, 0, 0, dtype(0)
    if precond == 'kron':
        if pshift is None:
            pshift = nr.geometric_mean(mask, noise) if noise is not None else float(shift)
        Q, lam = mr.factor_eigh(F)
        QL = [q.astype(dtype) for q in Q]
        QTL = [q.T.astype(dtype) for q in Q]
        t = np.ones(1, dtype=dtype)
        for l in lam:
            t = np.kron(t, l.astype(dtype))
        dinv = 1 / (t + dtype(pshift))

        def M(r):
            return np.where(mask, R._chain(QL, dinv * R._chain(QTL, r)), dtype(0))
    elif precond is None:
        def M(r):
            return r
    else:
        raise ValueError("precond must be None or 'kron'")
    r = bt.copy()
    z = M(r)
    rho = np.sum(r * z)
    p = z.copy()
    info, its = maxiter, maxiter
    for it in range(maxiter):
        if norm(r) < tol:
            info, its = 0, it
            break
        t = R._chain(FL, p)
        if d is None:
            t = t + shift * p
            pq = np.sum(p * t)
        else:
            pq = np.sum(p * t) + np.sum(d * p * p)
            t = t + d * p
        alpha = rho / pq
        x = x + alpha * p
        r = r - alpha * np.where(mask, t, dtype(0))
        z = M(r)
        rho_new = np.sum(r * z)
        p = z + (rho_new / rho) * p
        rho = rho_new
    else:
        if norm(r) < tol:
            info = 0
    return x, info, its, norm(r)


# ------------------------------------------------------- the Lanczos twins
def lanczos_ld(F, mask, shift=None, noise=None, seed=0, probe=0, steps=1, dtype=LD):
    """(alphas, betas, steps_done) of three-term Lanczos on v -> W K v + shift v
    (noise None: masked_lanczos_ref.masked_lanczos) or W K v + d o v (noise
    given: noise_ref.weighted_lanczos) from where(mask, probe_signs, 0) /
    sqrt(n_obs) in `dtype` arithmetic -- oracle.lanczos_tridiag's recurrence
    and breakdown rule.  betas has steps_done entries: betas[j] = |w_j|, the
    last one included (the device writes it too; T_k uses betas[:k - 1])."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    FL = [np.asarray(f, dtype=np.float64).astype(dtype) for f in F]
    z = np.where(mask, ocg.probe_signs(seed, probe, mask.size), 0.0).astype(dtype)
    if noise is not None:
        d = np.where(mask, np.asarray(noise, dtype=np.float64).reshape(-1), 0.0).astype(dtype)
    else:
        d = dtype(shift)
    v = z / norm(z).astype(dtype)
    v_prev = np.zeros_like(v)
    beta = dtype(0)
    alphas, betas = [], []
    for _ in range(steps):
        w = np.where(mask, R._chain(FL, v), dtype(0)) + d * v - beta * v_prev
        a = np.sum(w * v)
        w = w - a * v
        beta = norm(w).astype(dtype)
        alphas.append(a)
        betas.append(beta)
        if beta <= 1e-300:
            break
        v_prev, v = v, w / beta
    return np.array(alphas, dtype=dtype), np.array(betas, dtype=dtype), len(alphas)


def quadrature(alphas, betas, steps_done):
    """sum_j U[0][j]^2 log theta_j of the leading steps_done x steps_done
    tridiagonal (float64 eigh): times n_obs, one probe's estimate of
    log det."""
    k = int(steps_done)
    a = np.asarray(alphas, dtype=np.float64)[:k]
    b = np.asarray(betas, dtype=np.float64)[:k - 1]
    T = np.diag(a) + np.diag(b, 1) + np.diag(b, -1)
    theta, Uv = np.linalg.eigh(T)
    assert np.all(theta > 0), theta
    return float(np.sum(Uv[0, :] ** 2 * np.log(theta)))


# --------------------------------------------------------- the first iterate
def first_iterate(F, b, mask, shift=None, noise=None, fold=0, kp=None):
    """dict(alpha, x, r, bx, br): alpha_0, x_1 = alpha_0 W b and r_1 = W b -
    alpha_0 W (K + D) W b in long double, and the elementwise bounds of the
    module docstring (fold: gg_kron_fold_mask's bits).  Exactly one of shift
    and noise is given.  kp: kron_abi_ref.matvec_ref(F, W b, False, 0.0, fold)
    where the caller has it already (both variants share it)."""
    assert (shift is None) != (noise is None)
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    bt = np.where(mask, np.asarray(b, dtype=np.float64).reshape(-1), 0.0)
    n = bt.size
    p = bt.astype(LD)
    pa = np.abs(p)
    s = 0.0 if shift is None else float(shift)
    t, mag = R.matvec_ref(F, bt, False, 0.0, fold) if kp is None else kp
    if s != 0.0:
        t = t + LD(s) * p
    E = R.matvec_bound(F, bt, mag, False, s)
    u = LD(U53)
    g = n * u / (1 - n * u)
    rho = np.sum(p * p)
    pk = np.sum(p * t)
    e_pq = np.sum(pa * E) + g * np.sum(pa * (np.abs(t) + E))
    if noise is None:
        pq, tp, Ep = pk, t, E
    else:
        d = np.where(mask, np.asarray(noise, dtype=np.float64).reshape(-1), 0.0).astype(LD)
        S = np.sum(d * p * p)
        g1 = (n + 1) * u / (1 - (n + 1) * u)
        e_pq = e_pq + g1 * S
        e_pq = e_pq + u * (np.abs(pk) + S + e_pq)
        pq = pk + S
        tp = t + d * p
        Ep = E + u * (np.abs(t) + E + d * pa)
    assert pq - e_pq > 0
    alpha = rho / pq
    hi = rho * (1 + g) * (1 + u) / (pq - e_pq)
    lo = rho * (1 - g) * (1 - u) / (pq + e_pq)
    da = max(hi - alpha, alpha - lo)
    a_hi = alpha + da
    x = alpha * p
    bx = da * pa + u * a_hi * pa + u * np.abs(x)
    tpm = np.where(mask, tp, LD(0))
    r = p - alpha * tpm
    B = np.where(mask, da * np.abs(tpm) + a_hi * Ep, LD(0))
    br = B + u * (np.abs(r) + B) + u * (pa + alpha * np.abs(tpm))
    return dict(alpha=alpha, x=x, r=r, bx=bx, br=br)


def first_iterate_f64(F, b, mask, shift=None, noise=None):
    """(x_1, r_1) by float64 NumPy (oracle.kron_matvec, np.dot)."""
    import oracle
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    p = np.where(mask, np.asarray(b, dtype=np.float64).reshape(-1), 0.0)
    t = oracle.kron_matvec(F, p)
    if noise is None:
        t = t + shift * p
        pq = float(p.dot(t))
    else:
        d = np.where(mask, np.asarray(noise, dtype=np.float64).reshape(-1), 0.0)
        pq = float(p.dot(t)) + float(np.sum(d * p * p))
        t = t + d * p
    alpha = float(p.dot(p)) / pq
    return alpha * p, p - alpha * np.where(mask, t, 0.0)


# ------------------------------------------------------------ shared cases
_cache = {}


def _frozen(key, make):
    if key not in _cache:
        val = make()
        for a in val.values():
            for e in (a if isinstance(a, list) else [a]):
                if isinstance(e, np.ndarray):
                    e.setflags(write=False)
        _cache[key] = val
    return _cache[key]


def small_case(ms, frac=0.2):
    """dict(F, mask, b, noise, n) at a small shape: rbf_factors, make_mask (the
    two end points missing), b from default_rng(1), noise = NOISE_VAR *
    noise_scale."""
    def make():
        n = int(np.prod(ms))
        mask = mr.make_mask(n, frac)
        return dict(F=mr.rbf_factors(ms), mask=mask, n=n,
                    b=np.random.default_rng(1).standard_normal(n),
                    noise=nr.NOISE_VAR * nr.noise_scale(n))
    return _frozen(("small", tuple(ms), frac), make)


def wrap_case(ms, kind):
    """dict(F, mask, b, noise, n) at a shape past the grid-stride wrap, kind
    'cg' or 'lanczos' (another mask seed; b is the CG's right-hand side, the
    Lanczos probes need none).  Observed: 9 of 10 of the flat indices >= 2^20
    (a default_rng choice, so some pairs there are split) with n - 1 forced in,
    and 4096 of the indices below 2^20 (a default_rng choice) with 0 forced
    out: at least a quarter of the observed points belong to the second trip."""
    assert kind in ("cg", "lanczos")

    def make():
        n = int(np.prod(ms))
        assert n >= WRAP + 2
        rng = np.random.default_rng(11 if kind == "cg" else 13)
        mask = np.zeros(n, dtype=bool)
        mask[rng.choice(WRAP, size=4096, replace=False)] = True
        tail = n - WRAP
        mask[WRAP + rng.choice(tail, size=(9 * tail) // 10, replace=False)] = True
        mask[0] = False
        mask[n - 1] = True
        return dict(F=mr.rbf_factors(ms), mask=mask, n=n, b=rng.standard_normal(n),
                    noise=nr.NOISE_VAR * nr.noise_scale(n))
    return _frozen(("wrap", tuple(ms), kind), make)


SHIFT = 0.01
WRAP_SHIFT = SHIFT
WRAP_SEED, WRAP_PROBE = 5, 1
# odd n; two blocks of pairs; a folded factor; d = 1 and 2; a factor of order 1
SMALL_SHAPES = [(7, 5, 3), (12, 10, 8), (48, 6, 5), (9,), (6, 4), (5, 1, 4)]
# six observed points of the (4, 3, 2) grid: steps above n_obs
SIX_SHAPE, SIX_POINTS = (4, 3, 2), [1, 4, 8, 15, 18, 23]


def cg_case(ms):
    return wrap_case(ms, "cg") if tuple(ms) in WRAP_SHAPES else small_case(ms)


def first_case(ms, variant):
    """first_iterate of cg_case(ms), variant 'shift' (SHIFT) or 'noise', with
    the fold mask the library reports for these factors (kron_abi_ref.fold_mask;
    the device test asserts gg_kron_fold_mask agrees)."""
    def make():
        c = cg_case(ms)
        fold = R.fold_mask(c["F"])
        kp = _frozen(("kp", tuple(ms)), lambda: dict(zip("tm", R.matvec_ref(
            c["F"], np.where(c["mask"], c["b"], 0.0), False, 0.0, fold))))
        kw = dict(shift=SHIFT) if variant == "shift" else dict(noise=c["noise"])
        return first_iterate(c["F"], c["b"], c["mask"], fold=fold, kp=(kp["t"], kp["m"]), **kw)
    return _frozen(("first", tuple(ms), variant), make)


def dense_quadratic_log(F, mask, shift, seed, probe):
    """z_o^T log(K_oo + shift I) z_o, z the Rademacher probe (seed, probe): what
    n_obs sum U[0]^2 log theta equals once the Krylov space is exhausted."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    o = np.nonzero(mask)[0]
    lam, Q = np.linalg.eigh(mr.dense_K(F)[np.ix_(o, o)] + shift * np.eye(o.size))
    z = ocg.probe_signs(seed, probe, mask.size)[o]
    return float(np.sum(Q.T.dot(z) ** 2 * np.log(lam)))


def _variant_kw(c, variant):
    return dict(shift=SHIFT) if variant == "shift" else dict(noise=c["noise"])


def cg_twin(ms, variant, precond, iters):
    """dict(x, rn, fig_x, fig_rn): the long-double twin of cg_case(ms) after
    `iters` iterations at rtol = 0 (variant 'shift' or 'noise', precond None
    or 'kron'), and float64 NumPy's distance from it -- fig_x the norm-wise
    relative error of masked_ref.masked_cg / noise_ref.weighted_cg's x, fig_rn
    that of |r| from the same recurrence run in float64."""
    def make():
        c = cg_case(ms)
        kw = _variant_kw(c, variant)
        if variant == "shift":
            x64 = mr.masked_cg(c["F"], c["b"], c["mask"], SHIFT, rtol=0.0, maxiter=iters,
                               precond=precond)[0]
        else:
            x64 = nr.weighted_cg(c["F"], c["b"], c["mask"], c["noise"], rtol=0.0, maxiter=iters,
                                 precond=precond)[0]
        x, _, its, rn = cg_ld(c["F"], c["b"], c["mask"], rtol=0.0, maxiter=iters, precond=precond,
                              **kw)
        assert its == iters
        rn64 = cg_ld(c["F"], c["b"], c["mask"], rtol=0.0, maxiter=iters, precond=precond,
                     dtype=np.float64, **kw)[3]
        return dict(x=x, rn=rn, fig_x=rel(x64, x), fig_rn=float(abs(LD(rn64) - rn) / rn))
    return _frozen(("cgtwin", tuple(ms), variant, precond, iters), make)


CONVERGED_RTOL = 1e-11


def converged_twin(ms, variant, precond):
    """dict(iters, dense): the twin's iteration count at rtol = CONVERGED_RTOL
    and the dense K_oo solve of small_case(ms)."""
    def make():
        c = small_case(ms)
        x, info, its, _ = cg_ld(c["F"], c["b"], c["mask"], rtol=CONVERGED_RTOL, precond=precond,
                                **_variant_kw(c, variant))
        assert info == 0
        dense = (mr.dense_solve(c["F"], c["b"], c["mask"], SHIFT) if variant == "shift"
                 else nr.dense_solve(c["F"], c["b"], c["mask"], c["noise"]))
        assert rel(x, dense) < 1e-9
        return dict(iters=its, dense=dense)
    return _frozen(("conv", tuple(ms), variant, precond), make)


def wrap_twin(ms, family):
    """The long-double twin at a wrap shape after WRAP_ITERS iterations /
    steps, and float64 NumPy's distance from it.  family 'cg', 'cg_noise':
    cg_twin's dict.  family 'lz', 'lz_noise': dict(alphas, betas, fig_a,
    fig_b) -- the largest relative error over the WRAP_ITERS alphas / betas of
    masked_lanczos_ref.masked_lanczos / noise_ref.weighted_lanczos (run one
    step further: they drop the last beta)."""
    k = WRAP_ITERS
    if family in ("cg", "cg_noise"):
        return cg_twin(ms, "shift" if family == "cg" else "noise", None, k)

    def make():
        c = wrap_case(ms, "lanczos")
        if family == "lz":
            kw = dict(shift=WRAP_SHIFT)
            a64, b64 = ml.masked_lanczos(c["F"], c["mask"], WRAP_SHIFT, WRAP_SEED, WRAP_PROBE,
                                         k + 1)
        else:
            assert family == "lz_noise"
            kw = dict(noise=c["noise"])
            a64, b64 = nr.weighted_lanczos(c["F"], c["mask"], c["noise"], WRAP_SEED, WRAP_PROBE,
                                           k + 1)
        a, b, done = lanczos_ld(c["F"], c["mask"], seed=WRAP_SEED, probe=WRAP_PROBE, steps=k, **kw)
        assert done == k and len(a64) == k + 1
        return dict(alphas=a, betas=b, fig_a=max_rel(a64[:k], a), fig_b=max_rel(b64[:k], b))
    return _frozen(("twin", tuple(ms), family), make)


def tolerance(fig):
    """The device tolerance of a wrap comparison: 100 x float64 NumPy's own
    distance from the long-double twin, floored at 1e-13.  The margin covers
    the device's 2048-block partial sums against NumPy's pairwise sums in
    alpha and beta; the recurrence amplifies those differences exactly as it
    amplifies NumPy's own."""
    return max(100.0 * float(fig), 1e-13)
