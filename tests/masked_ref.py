"""NumPy restatement of the masked grid-GP algebra (test infrastructure only).

The grid GP with missing observations: W = diag(mask), A = W K W + s I,
A x = W y.  masked_cg is the (optionally preconditioned) CG the device runs
(gg_cgm_*), with oracle.cg_solve's stopping rule and iteration count; the two
log-determinant formulas are the ones GPGridModel(mask=...) uses.  Dense
K_oo algebra (dense_*) is the ground truth the tests compare both against.
"""
import numpy as np

import oracle


def rbf_factors(ms):
    """RBF factors on linspace(0, 1, m), l_i = 0.1 (1 + 0.05 i), jitter 1e-12."""
    F = []
    for i, m in enumerate(ms):
        g = np.linspace(0, 1, m)
        F.append(oracle.cov_1d("RBF", g, g, 1.0, 0.1 * (1 + 0.05 * i)) + 1e-12 * np.eye(m))
    return F


def make_mask(n, frac, seed=0):
    """Boolean mask (True = observed): round(frac n) points from
    default_rng(seed).choice missing, the first and last grid points forced
    missing."""
    miss = np.random.default_rng(seed).choice(n, size=int(round(frac * n)), replace=False)
    mask = np.ones(n, dtype=bool)
    mask[miss] = False
    mask[0] = mask[-1] = False
    return mask


def factor_eigh(F):
    lam, Q = [], []
    for f in F:
        w, q = np.linalg.eigh(f)
        lam.append(w)
        Q.append(q)
    return Q, lam


def kron_eigs(lam):
    t = np.ones(1)
    for l in lam:
        t = np.kron(t, l)
    return t


def masked_cg(F, b, mask, shift, rtol=1e-5, atol=0.0, maxiter=None, precond=None):
    """(x, info, iters) of CG on (W K W + shift I) x = W b, x0 = 0.

    precond None or 'kron': z = W Q diag(1 / (lam + shift)) Q^T r.  The
    stopping test is on the true |r| either way, seen after each update (the
    same count as oracle.cg_solve: iterations completed when |r| < tol)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
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
        Q, lam = factor_eigh(F)
        QT = [q.T for q in Q]
        dinv = 1.0 / (kron_eigs(lam) + shift)

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
        t = oracle.kron_matvec(F, p) + shift * p
        alpha = rho / float(p.dot(t))
        x += alpha * p
        r -= alpha * np.where(mask, t, 0.0)
        z = M(r)
        rho_new = float(r.dot(z))
        p = z + (rho_new / rho) * p
        rho = rho_new
    if np.linalg.norm(r) < tol:
        return x, 0, maxiter
    return x, maxiter, maxiter


def dense_K(F):
    K = np.ones((1, 1))
    for f in F:
        K = np.kron(K, f)
    return K


def dense_solve(F, b, mask, shift):
    """x with x_o = (K_oo + shift I)^-1 b_o and 0 at the missing points."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    K = dense_K(F)
    o = np.nonzero(mask)[0]
    x = np.zeros(mask.size)
    x[o] = np.linalg.solve(K[np.ix_(o, o)] + shift * np.eye(o.size),
                           np.asarray(b, dtype=np.float64).reshape(-1)[o])
    return x


def dense_logdet(F, mask, shift):
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    K = dense_K(F)
    o = np.nonzero(mask)[0]
    return float(np.linalg.slogdet(K[np.ix_(o, o)] + shift * np.eye(o.size))[1])


def schur_logdet(F, mask, shift):
    """log det(K_oo + s I) = sum_N log(lam_g + s) + log det[((K + s I)^-1)_mm]:
    the m x m block from m exact solves of unit vectors (Q^T e_j is a
    Kronecker product of rows of the Q_f)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    Q, lam = factor_eigh(F)
    QT = [q.T for q in Q]
    t = kron_eigs(lam)
    full = float(np.sum(np.log(t + shift)))
    miss = np.nonzero(~mask)[0]
    if miss.size == 0:
        return full
    B = np.empty((miss.size, miss.size))
    for k, g in enumerate(miss):
        e = np.zeros(mask.size)
        e[g] = 1.0
        B[:, k] = oracle.kron_matvec(Q, oracle.kron_matvec(QT, e) / (t + shift))[miss]
    B = 0.5 * (B + B.T)
    return full + float(np.linalg.slogdet(B)[1])


def scaled_eigs_logdet(F, mask, shift):
    """Wilson's scaled eigenvalues: sum_{i <= n} log((n / N) lam_(i) + s) over the
    n largest Kronecker eigenvalues."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    _, lam = factor_eigh(F)
    t = np.sort(kron_eigs(lam))[::-1]
    n, N = int(mask.sum()), mask.size
    return float(np.sum(np.log(t[:n] * (float(n) / float(N)) + shift)))
