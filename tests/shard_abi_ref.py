"""Plain np.longdouble restatement of the sharded section of the C ABI
(gg_kron_dist_*, gg_cgs_*, gg_parity_fold, gg_shard0_fold): test
infrastructure only, NumPy only.  tests/kron_abi_ref.py is its single-GPU
sibling and supplies the matvec bound; dist_helpers.NumpyEngine is the float64
restatement to read alongside (tests/test_shard_abi_ref.py holds the two
together on the host).

Layouts are written from the header text with reshape / transpose, never from
the kernels' address arithmetic:

  * local vector of rank g: (m_1, .., m_{d-1}, a), a = i_0 - g s0 fastest,
    s0 = m_0 / G;
  * phase 1 send buffer: all mode products 1..d-1 applied, then chunk h = the
    rows j_1 in [h m_1 / G, (h + 1) m_1 / G), each chunk in
    (a, j_1', j_2, .., j_{d-1}) order;
  * exchange: chunk h of rank g's send becomes chunk g of rank h's recv
    (all-to-all), so recv is (m_0, R / G) row-major, R = N / m_0;
  * phase 2: factor 0 applied to recv's rows, then chunk g' = the rows j_0 in
    [g' s0, (g' + 1) s0), each chunk in (c, a) order; after the second
    exchange every rank holds its part of K x in the local layout.

Bounds (u = 2^-53), derived, not tuned:

  * matvec phases: kron_abi_ref.matvec_bound over the stages the call runs
    (factors 1..d-1 for phase 1, factor 0 for phase 2), with the bits of
    gg_kron_dist_fold_mask -- the sharded path runs the same kernels.
  * dots: chain u sum |x_i y_i|, chain = the longest chain of additions
    between one product and the result (dot_chain below).  An fma adds one
    product with one rounding, so a thread that takes t products has a chain
    of t; the block stage adds 6 wave shuffles and at most 4 wave partials;
    the one-block reduction reads ceil(blocks / 1024) partials per thread,
    then 6 shuffles and 16 wave partials.
  * elementwise updates x + a p with a = rho / pq formed on the device in
    float64: a carries one rounding (u |a p|), the product at most one
    (u |a p|, none when contracted to an fma), the sum one
    (u |x + a p| <= u (|x| + |a p|)); second-order terms and the long double
    reference's own rounding are below one more u:  4 u (|x| + |a p|)
    (AXPY_C), whether or not the compiler contracts.  The fused recurrence's
    r - a (q + s p) forms q + s p first (at most two more roundings, relative
    to |q| + |s p|):  6 u (|r| + |a| (|q| + |s p|))  (FUSED_R_C).
  * parity fold: every output is scale times a sum of 2^K corner values
    (2^K - 1 additions, one multiply, the float64 scale's own rounding):
    (2^K + 1) u scale sum |corner values|.
"""
import itertools

import numpy as np

import kron_abi_ref as R

LD = np.longdouble
U53 = 2.0 ** -53
AXPY_C = 4
FUSED_R_C = 6
K_VEC_THREADS = 256    # gg_internal.h kVecThreads
K_VEC_BLOCKS = 2048    # gg_internal.h kVecBlocks
CANCEL_TOL = 1e-6      # the fused recurrence's repair threshold


def ld(a):
    return np.asarray(a, dtype=LD)


# ------------------------------------------------------------------ layouts
def dims(m, world):
    m = [int(v) for v in m]
    return m, m[0] // int(world), int(np.prod(m)) // int(world)


def scatter(x, m, world, rank):
    """Rank's part of the grid vector x (C order over m) in the local layout."""
    m, s0, _ = dims(m, world)
    X = np.asarray(x).reshape(m)[rank * s0:(rank + 1) * s0]
    return np.ascontiguousarray(np.moveaxis(X, 0, -1)).reshape(-1)


def gather(locals_, m):
    m, s0, _ = dims(m, len(locals_))
    parts = [np.moveaxis(np.asarray(v).reshape(m[1:] + [s0]), -1, 0) for v in locals_]
    return np.concatenate(parts, axis=0).reshape(-1)


def _stage(F, X, axis):
    return np.moveaxis(np.tensordot(F, X, axes=([1], [axis])), 0, axis)


def _abs_factor(F, split):
    G = np.abs(ld(F))
    return G + G[:, ::-1] if split else G


def phase1_ref(factors, world, x_local, mask=0):
    """(send, mag) of gg_kron_dist_phase1 on one rank's x_local."""
    m, s0, _ = dims([np.shape(F)[0] for F in factors], world)
    d = len(m)
    X = ld(x_local).reshape(m[1:] + [s0])
    A = np.abs(X)
    for k in range(1, d):
        X = _stage(ld(factors[k]), X, k - 1)
        A = _stage(_abs_factor(factors[k], (mask >> k) & 1), A, k - 1)
    out = []
    for Y in (X, A):
        Y = np.moveaxis(Y, -1, 0).reshape(s0, world, m[1] // world, -1)
        out.append(np.ascontiguousarray(Y.transpose(1, 0, 2, 3)).reshape(-1))
    return out[0], out[1]


def phase1_bound(factors, x_local, mag):
    return R.matvec_bound(list(factors[1:]), x_local, mag)


def exchange(sends):
    """The all-to-all as a host permutation: recv[g] chunk h = send[h] chunk g."""
    G = len(sends)
    c = np.asarray(sends[0]).size // G
    return [np.concatenate([np.asarray(sends[h]).reshape(-1)[g * c:(g + 1) * c]
                            for h in range(G)]) if c else np.asarray(sends[g]).reshape(-1)[:0]
            for g in range(G)]


def phase2_ref(factors, world, recv, mask=0):
    """(send, mag) of gg_kron_dist_phase2 on one rank's recv."""
    m, s0, _ = dims([np.shape(F)[0] for F in factors], world)
    Xr = ld(recv).reshape(m[0], -1)
    C = Xr.shape[1]
    out = []
    for F, X in ((ld(factors[0]), Xr), (_abs_factor(factors[0], mask & 1), np.abs(Xr))):
        Z = np.einsum("ji,ic->jc", F, X)
        out.append(np.ascontiguousarray(Z.T.reshape(C, world, s0).transpose(1, 0, 2)).reshape(-1))
    return out[0], out[1]


def phase2_bound(factors, recv, mag):
    return R.matvec_bound([factors[0]], recv, mag)


def matvec_ref(factors, world, locals_, mask=0):
    """Every rank's part of K x in the local layout, long double, through the
    two phases and the two exchanges."""
    s1 = [phase1_ref(factors, world, v, mask)[0] for v in locals_]
    s2 = [phase2_ref(factors, world, v, mask)[0] for v in exchange(s1)]
    return exchange(s2)


# ------------------------------------------------------------------- gates
def fold_mask(factors, fold_min=48, enabled=True):
    """pack_fold's condition per factor: fold_min <= m <= 256 and
    centrosymmetric within 16 eps max |F|."""
    return R.fold_mask(factors, False, fold_min) if enabled else 0


def ceil_div(a, b):
    return -(-int(a) // int(b))


def lean_ok(m_k, M):
    """dist_phase1_fused's lean_ok for a folded factor of order m_k applied to
    M rows: both k-step unrollings (3 and 2) of its fKS = ceil(ceil(m / 2) / 4)
    k-steps fit the factor's own order, and 32 M fits 32 bits."""
    fks = ceil_div(m_k - m_k // 2, 4)
    return (4 * 3 * ceil_div(fks, 3) <= m_k and 4 * 2 * ceil_div(fks, 2) <= m_k
            and 32 * int(M) < (1 << 32))


def lean_flags(m, world):
    """lean_ok of factors 1..d-1 of the sharded operator."""
    m, _, nl = dims(m, world)
    return [lean_ok(m[k], nl // m[k]) for k in range(1, len(m))]


# -------------------------------------------------------------------- dots
def vec_blocks(n):
    return min(K_VEC_BLOCKS, max(ceil_div(max(int(n) // 2, 1), K_VEC_THREADS), 1))


def dot_chain(n, lane):
    """The longest chain of additions of a vector kernel's dot product over n
    elements, lane = 2 (16-byte lanes, the odd tail on thread 0) or 1."""
    nb = vec_blocks(n)
    per_thread = lane * ceil_div(int(n) // lane, nb * K_VEC_THREADS)
    if lane == 2 and int(n) & 1:
        per_thread += 1
    return per_thread + 6 + 4 + ceil_div(nb, 1024) + 6 + 16


def dot_ref(x, y):
    """(value, sum |x_i y_i|) in long double."""
    t = ld(x).reshape(-1) * ld(y).reshape(-1)
    return t.sum(), np.abs(t).sum()


def dot_bound(n, lane, mag, extra=0):
    return (dot_chain(n, lane) + extra) * U53 * mag


# ------------------------------------------------------------ CG scalar calls
def new_state():
    return dict(rho=0.0, rho_prev=0.0, pq=0.0, alpha=LD(0), beta=LD(0), tol=0.0, bnorm=0.0,
                iters=0, done=False, first=True, pending=False, repair=False, cancels=0,
                xh=2, xs=False, xsc=LD(0), xsp=None, xc=[LD(0), LD(0)], xp=[None, None])


def init_ref(sc, rr, rtol, atol):
    """gg_cgs_init from the global r.r (a float64, as the device reads it)."""
    s = float(rr)
    sc = dict(new_state(), rho=s)
    with np.errstate(invalid="ignore"):
        sc["bnorm"] = float(np.sqrt(s))
        sc["tol"] = float(np.fmax(atol, rtol * sc["bnorm"]))
        sc["done"] = bool(s == 0.0 or not np.sqrt(s) >= sc["tol"])
    return sc


def prologue_ref(sc, p, r):
    """Phase 1's CG prologue, p in place: (p_new, |r| + |beta p|)."""
    p, r = ld(p), ld(r)
    if sc["done"]:
        return p, np.abs(p)
    if sc["first"]:
        return r.copy(), np.abs(r)
    return r + sc["beta"] * p, np.abs(r) + np.abs(sc["beta"] * p)


def shift_dot_ref(sc, q, p, shift):
    """(q_new, |q| + |shift p|); the local p.q is taken on the device's q_new."""
    q, p = ld(q), ld(p)
    if sc["done"]:
        return q, np.abs(q)
    return q + LD(shift) * p, np.abs(q) + np.abs(LD(shift) * p)


def alpha_ref(sc, pq):
    sc = dict(sc)
    if not sc["done"]:
        sc["pq"] = float(pq)
        with np.errstate(divide="ignore", invalid="ignore"):
            sc["alpha"] = LD(sc["rho"]) / LD(float(pq))
    return sc


def update_ref(sc, x, r, p, q):
    """(x_new, r_new, mag_x, mag_r)."""
    x, r, p, q = ld(x), ld(r), ld(p), ld(q)
    if sc["done"]:
        return x, r, np.abs(x), np.abs(r)
    a = sc["alpha"]
    return x + a * p, r - a * q, np.abs(x) + np.abs(a * p), np.abs(r) + np.abs(a * q)


def rho_ref(sc, rr):
    sc = dict(sc)
    if sc["done"]:
        return sc
    s = float(rr)
    sc.update(rho_prev=sc["rho"], rho=s, iters=sc["iters"] + 1, first=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc["beta"] = LD(s) / LD(sc["rho_prev"])
        sc["beta_err"] = U53 * abs(sc["beta"])
        if not np.sqrt(s) >= sc["tol"]:
            sc["done"] = True
    return sc


# ---- the fused recurrence
def half(n):
    return min(2 * ceil_div(n, 4), int(n))


def fused_prologue_ref(sc, p_old, r, q_old, x, shift, vecs):
    """The prologue and the side job of gg_kron_dist_phase1_fused: dict(r,
    p_new, x, qe = q_old + s p_old, and the elementwise bounds b_r, b_p, b_x).
    vecs maps the direction ids the state holds (xp) to their vectors.
    b_p: p_new = r + beta p_old on the device's r (b_r) with the device's
    beta (beta_err, fused_scalars_ref); b_x: two axpy steps in one pass."""
    p_old, r, q_old, x = ld(p_old), ld(r), ld(q_old), ld(x)
    if sc["done"]:
        return None
    qe = q_old + LD(shift) * p_old
    mag_r = np.abs(r)
    if sc["pending"]:
        mag_r = mag_r + np.abs(sc["alpha"]) * (np.abs(q_old) + np.abs(LD(shift) * p_old))
        r = r - sc["alpha"] * qe
    pn = r + sc["beta"] * p_old
    mag_p = np.abs(r) + np.abs(sc["beta"] * p_old)
    mag_x = np.abs(x)
    if sc["xh"] < 2:
        H = half(x.size)
        lo, hi = (0, H) if sc["xh"] == 0 else (H, x.size)
        t0 = sc["xc"][0] * ld(vecs[sc["xp"][0]])[lo:hi]
        t1 = sc["xc"][1] * ld(vecs[sc["xp"][1]])[lo:hi]
        x = x.copy()
        mag_x = mag_x.copy()
        x[lo:hi] += t0 + t1
        mag_x[lo:hi] += np.abs(t0) + np.abs(t1)
    b_r = FUSED_R_C * U53 * mag_r
    b_p = AXPY_C * U53 * mag_p + b_r + sc.get("beta_err", LD(0)) * np.abs(p_old)
    return dict(r=r, p_new=pn, x=x, qe=qe, b_r=b_r, b_p=b_p, b_x=2 * AXPY_C * U53 * mag_x)


def fused_post_ref(q, p, shift):
    """red[2], red[4] and their magnitudes from q = K p (unshifted)."""
    qv = ld(q) + LD(shift) * ld(p)
    pq, mpq = dot_ref(p, qv)
    qq, mqq = dot_ref(qv, qv)
    return pq, qq, mpq, mqq, qv


def fused_scalars_ref(sc, red, p_new_id):
    """gg_cgs_fused_scalars from the all-reduced red (five float64)."""
    sc = dict(sc, xc=list(sc["xc"]), xp=list(sc["xp"]))
    if sc["done"]:
        return sc
    rr, pqo, pq, _, qq = [float(v) for v in red]
    if sc["pending"]:
        sc.update(rho_prev=sc["rho"], rho=rr, iters=sc["iters"] + 1)
        if not np.sqrt(rr) >= sc["tol"]:
            sc.update(done=True, pending=False)
            if sc["xh"] < 2:
                sc["xh"] += 1
            return sc
    rho = LD(sc["rho"])
    alpha = rho / LD(pq)
    rq = LD(pq) - sc["beta"] * LD(pqo)
    rt = rho - 2 * alpha * rq + alpha * alpha * LD(qq)
    repair = bool(rt < LD(CANCEL_TOL) * rho)
    # the float64 beta = rt / rho: rt is a difference of three terms of size
    # ~rho (the reason for the repair threshold), so its error is absolute in
    # T = rho + 2 |alpha rq| + alpha^2 qq.  rq = pq - beta pqo: u (|pq| +
    # 2 |beta pqo|) + beta_err |pqo|; 2 alpha rq: three roundings, alpha^2 qq:
    # four, the two sums: one each, relative to at most T -> 6 u T in all
    erq = U53 * (abs(LD(pq)) + 2 * abs(sc["beta"] * LD(pqo))) + \
        sc.get("beta_err", LD(0)) * abs(LD(pqo))
    T = rho + 2 * abs(alpha * rq) + alpha * alpha * LD(qq)
    err_rt = 2 * abs(alpha) * erq + 6 * U53 * T
    sc["beta_err"] = LD(0) if repair else err_rt / rho + U53 * abs(rt / rho)
    sc.update(pq=pq, alpha=alpha, beta=LD(0) if repair else rt / rho, first=False, pending=True,
              repair=repair, cancels=sc["cancels"] + int(repair), rt=rt)
    if sc["xh"] < 2:
        sc["xh"] += 1
    if not sc["xs"]:
        sc.update(xs=True, xsc=alpha, xsp=p_new_id)
    else:
        sc.update(xc=[sc["xsc"], alpha], xp=[sc["xsp"], p_new_id], xh=0, xs=False)
    return sc


def fused_close_ref(sc, x, r, q, p, shift, vecs):
    """(sc, x, r, b_x, b_r): the deferred x steps (applied even when the
    latch is set; at most three axpy steps in one pass) and the pending r
    update, with their elementwise bounds."""
    sc = dict(sc)
    x, r = ld(x).copy(), ld(r)
    mag_x, mag_r = np.abs(x), np.abs(r)
    if sc["xs"]:
        t = sc["xsc"] * ld(vecs[sc["xsp"]])
        x += t
        mag_x += np.abs(t)
    if sc["xh"] < 2:
        lo = 0 if sc["xh"] == 0 else half(x.size)
        t0 = sc["xc"][0] * ld(vecs[sc["xp"][0]])[lo:]
        t1 = sc["xc"][1] * ld(vecs[sc["xp"][1]])[lo:]
        x[lo:] += t0 + t1
        mag_x[lo:] += np.abs(t0) + np.abs(t1)
    sc.update(xh=2, xs=False)
    if not sc["done"] and sc["pending"]:
        r = r - sc["alpha"] * (ld(q) + LD(shift) * ld(p))
        mag_r = mag_r + np.abs(sc["alpha"]) * (np.abs(ld(q)) + np.abs(LD(shift) * ld(p)))
    return sc, x, r, 3 * AXPY_C * U53 * mag_x, FUSED_R_C * U53 * mag_r


def fused_close_rho_ref(sc, rr):
    sc = dict(sc)
    if sc["done"] or not sc["pending"]:
        return sc
    s = float(rr)
    sc.update(rho_prev=sc["rho"], rho=s, iters=sc["iters"] + 1, first=False, pending=False,
              repair=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc["beta"] = LD(s) / LD(sc["rho_prev"])
        sc["beta_err"] = U53 * abs(sc["beta"])
        if not np.sqrt(s) >= sc["tol"]:
            sc["done"] = True
    return sc


# ------------------------------------------------------------------- folds
def _parity_geom(m, world):
    m = [int(v) for v in m]
    K = int(world).bit_length() - 1
    return m, K, [m[k] // 2 for k in range(K)]


def _corner_view(X, K, hs, corner):
    """The view of the d-dimensional X that holds corner `corner` of every
    local element: axis k < K reversed where the corner bit is set, cut to
    its first half."""
    sl = tuple((slice(None, None, -1) if corner[k] else slice(None)) for k in range(K))
    V = X[sl]
    return V[tuple(slice(0, h) for h in hs)]


def _sign(K, rank, corner):
    s = 1
    for k in range(K):
        if corner[k] and (rank >> (K - 1 - k)) & 1:
            s = -s
    return s


def parity_scale(K):
    """2^(-K / 2) as the library forms it: exact for even K, the float64
    sqrt(1/2) times a power of two for odd K."""
    return float(np.ldexp(1.0, -(K // 2)) * (np.sqrt(0.5) if K & 1 else 1.0))


def parity_fold_ref(x, m, world, rank):
    """(local block, bound): rank's block of the grid vector x in the even /
    odd basis of axes 0..K-1, C order over (m_K .. m_{d-1}, h_0 .. h_{K-1});
    the even (rank bit clear) half adds the mirrored element, the odd
    subtracts it, each sharded axis scaled by 2^(-1/2)."""
    m, K, hs = _parity_geom(m, world)
    d = len(m)
    X = ld(x).reshape(m)
    acc, mag = LD(0), LD(0)
    for corner in itertools.product((0, 1), repeat=K):
        V = _corner_view(X, K, hs, corner)
        acc = acc + _sign(K, rank, corner) * V
        mag = mag + np.abs(V)
    sc = LD(parity_scale(K))
    axes = list(range(K, d)) + list(range(K))
    out = np.ascontiguousarray(np.transpose(acc * sc, axes)).reshape(-1)
    mg = np.ascontiguousarray(np.transpose(mag * sc, axes)).reshape(-1)
    return out, ((1 << K) + 1) * U53 * mg


def parity_unfold_ref(local, m, world, rank):
    """(contribution, bound): P^T of rank's block, written to every grid
    element (the ranks' contributions sum to the grid vector)."""
    m, K, hs = _parity_geom(m, world)
    d = len(m)
    axes = list(range(K, d)) + list(range(K))
    lshape = [hs[a] if a < K else m[a] for a in axes]
    L = np.transpose(ld(local).reshape(lshape), np.argsort(axes))   # (h_0.., m_K..)
    sc = LD(parity_scale(K))
    out = np.full(m, np.nan, dtype=LD)
    for corner in itertools.product((0, 1), repeat=K):
        _corner_view(out, K, hs, corner)[...] = _sign(K, rank, corner) * sc * L
    out = out.reshape(-1)
    return out, 2 * U53 * np.abs(out)


def shard0_ref(x, m, world, rank):
    """gg_shard0_fold forward: exact (a gather)."""
    return scatter(x, m, world, rank)


def shard0_positions(m, world, rank):
    """Grid index of every local element, from the layout alone."""
    n = int(np.prod([int(v) for v in m]))
    return scatter(np.arange(n), m, world, rank)


# ------------------------------------------------------------- case lists
# (m, world, folded?, fold_min or None for the default, expected mask)
def _mask_all(m):
    return (1 << len(m)) - 1


MATVEC_SHAPES = [
    ((2, 2), 1), ((2, 2), 2), ((5, 7, 3), 1), ((6, 9, 5), 3), ((4, 8, 17, 3), 4),
    ((4, 4, 1, 5), 2), ((4, 4, 1, 5), 4), ((12, 20), 4), ((256, 8), 8), ((8, 256), 8),
]
# folded: (m, world, GG_KRON_FOLD_MIN or None, mask)
FOLDED_SHAPES = [
    ((2, 100), 2, 8, 0b10), ((100, 2), 2, 8, 0b01), ((9, 9, 11), 3, 8, 0b111),
    ((4, 8, 9, 48), 4, None, 0b1000),
]
PROLOGUE_SHAPES = [((12, 20), 4, None), ((6, 9, 5), 3, None), ((9, 9, 11), 3, 8)]
TEXTBOOK_SHAPES = [((6, 9, 5), 3), ((4, 8, 17, 3), 4)]
FUSED_SHAPES = [((4, 8, 10, 12), 2), ((4, 12, 16, 8), 4), ((2, 8, 8, 12, 8), 2),
                ((4, 8, 9, 11), 4)]
# lean_ok of factors 1..d-1 each fused case was written for
FUSED_LEAN = {
    (4, 8, 10, 12): [False, False, True],
    (4, 12, 16, 8): [True, True, False],
    (2, 8, 8, 12, 8): [False, False, True, False],
    (4, 8, 9, 11): [False, False, False],
}


def matvec_cases():
    """(id, m, world, fold_env, mask): fold_env = ("GG_KRON_FOLD", "0") for
    the dense cases, ("GG_KRON_FOLD_MIN", "8") or None (the default switches)
    for the folded ones."""
    out = []
    for m, G in MATVEC_SHAPES:
        out.append(("x".join(map(str, m)) + "_w%d_dense" % G, m, G, ("GG_KRON_FOLD", "0"), 0))
    for m, G, fmin, mask in FOLDED_SHAPES:
        env = ("GG_KRON_FOLD_MIN", str(fmin)) if fmin else None
        out.append(("x".join(map(str, m)) + "_w%d_folded" % G, m, G, env, mask))
    return out


def case_factors(m, mask, seed=0):
    """Random nonsymmetric factors scaled by 1 / sqrt(m_k); the factors in
    mask are centrosymmetric (and still nonsymmetric: their order is above 2)."""
    def make():
        rng = np.random.default_rng(1000 + seed + sum((i + 1) * int(v) for i, v in enumerate(m)))
        fs = []
        for k, mk in enumerate(m):
            A = rng.standard_normal((int(mk), int(mk)))
            if (mask >> k) & 1:
                A = R.centro(A)
            fs.append(np.ascontiguousarray(A / np.sqrt(mk)))
        return (fs,)
    return R._frozen(("shard", tuple(m), int(mask), seed), make)[0]
