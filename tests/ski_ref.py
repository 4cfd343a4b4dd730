"""NumPy restatement of structured kernel interpolation (test infrastructure
only): the per-axis stencils of gg_ski_stencils, a dense W, the dense
W K W^T, the CG on the points with its coefficients recorded (gg_skicg_*), the
Lanczos tridiagonal rebuilt from them with its quadrature, and a dense LML.

The grid has evenly spaced axes, input dimension 0 fastest: the node index is
sum_f j_f prod_{e<f} m_e.  With u = (x - lo) / h on an axis of m nodes:
  cubic   1 <= u <= m - 2;  j = min(max(floor u, 1), m - 3), t = u - j, nodes
          j - 1 .. j + 2, Keys' cubic convolution weights
  linear  0 <= u <= m - 1;  j = min(max(floor u, 0), m - 2), nodes j, j + 1
u within EDGE_TOL of a domain edge counts as on it (the rounding of the
division); anything further out is outside.
"""
import numpy as np

import oracle
from oracle.cg import probe_signs, quadrature_logdet  # noqa: F401

EDGE_TOL = 1e-10


def axis_params(g):
    a = np.asarray(g, dtype=np.float64).reshape(-1)
    return float(a[0]), float((a[-1] - a[0]) / (a.size - 1)), int(a.size)


def domain_points(xg, n, order, seed=0):
    """n uniform points inside the interpolation domain of xg, (n, d)."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, len(xg)))
    for f, g in enumerate(xg):
        lo, h, m = axis_params(g)
        pad = h if order == 4 else 0.0
        X[:, f] = rng.uniform(lo + pad, lo + (m - 1) * h - pad, n)
    return X


def stencil_1d(x, lo, h, m, order):
    """(first node (int64), weights (n, order), outside (bool)) of one axis."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    u = (x - lo) / h
    ulo = 1.0 if order == 4 else 0.0
    uhi = (m - 1) - ulo
    outside = ~((u >= ulo - EDGE_TOL) & (u <= uhi + EDGE_TOL))
    u = np.minimum(np.maximum(u, ulo), uhi)
    j = np.clip(np.floor(u), ulo, m - (3 if order == 4 else 2))
    t = u - j
    if order == 4:
        w = 0.5 * np.stack([((-t + 2.0) * t - 1.0) * t,
                            (3.0 * t - 5.0) * t * t + 2.0,
                            ((-3.0 * t + 4.0) * t + 1.0) * t,
                            (t - 1.0) * t * t], axis=1)
        first = j.astype(np.int64) - 1
    else:
        w = np.stack([1.0 - t, t], axis=1)
        first = j.astype(np.int64)
    return first, w, outside


def stencils(xg, X, order):
    """first (n, d) int64, weights (n, d, order), number of points outside."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    first = np.empty((n, d), dtype=np.int64)
    w = np.empty((n, d, order))
    out = np.zeros(n, dtype=bool)
    for f in range(d):
        lo, h, m = axis_params(xg[f])
        first[:, f], w[:, f, :], o = stencil_1d(X[:, f], lo, h, m, order)
        out |= o
    return first, w, int(out.sum())


def dense_W(xg, X, order):
    """The n x N interpolation matrix (rows: points; columns: nodes, dimension
    0 fastest).  Raises ValueError if a point is outside the domain."""
    first, w, nout = stencils(xg, X, order)
    if nout:
        raise ValueError("%d point(s) outside the interpolation domain" % nout)
    n, d = first.shape
    ms = [axis_params(g)[2] for g in xg]
    N = int(np.prod(ms))
    W = np.zeros((n, N))
    strides = np.concatenate(([1], np.cumprod(ms)[:-1])).astype(np.int64)
    for c in np.ndindex(*([order] * d)):
        node = np.zeros(n, dtype=np.int64)
        wp = np.ones(n)
        for f in range(d):
            node += (first[:, f] + c[f]) * strides[f]
            wp = wp * w[:, f, c[f]]
        np.add.at(W, (np.arange(n), node), wp)
    return W


def rbf_factors(xg, ls, var=1.0, jitter=1e-12):
    """Per-axis RBF factors on the grid axes (the whole variance on axis 0)."""
    F = []
    for f, g in enumerate(xg):
        a = np.asarray(g, dtype=np.float64).reshape(-1)
        l = ls[f] if np.ndim(ls) else ls
        F.append(oracle.cov_1d("RBF", a, a, var if f == 0 else 1.0, l)
                 + jitter * np.eye(a.size))
    return F


def dense_K(F):
    """The dense Kronecker matrix in the grid layout (dimension 0 fastest)."""
    K = np.ones((1, 1))
    for f in F:
        K = np.kron(f, K)
    return K


def dense_wkw(W, F):
    return W @ dense_K(F) @ W.T


def cg_coeffs(matvec, b, rtol=1e-5, atol=0.0, maxiter=None):
    """oracle.cg_solve's recurrence with (alpha_j, beta_j) recorded:
    (x, info, iters, alphas, betas); beta_j = rho_{j+1} / rho_j follows update
    j.  rtol = atol = 0 runs maxiter iterations (or to rho = 0)."""
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    bnorm = np.linalg.norm(b)
    tol = max(float(atol), float(rtol) * float(bnorm))
    x = np.zeros_like(b)
    if maxiter is None:
        maxiter = 10 * b.size
    r = b.copy()
    p = r.copy()
    rho = float(r @ r)
    al, be = [], []
    for it in range(maxiter):
        if rho == 0.0 or np.sqrt(rho) < tol:
            return x, 0, it, np.array(al), np.array(be)
        q = matvec(p)
        alpha = rho / float(p @ q)
        x += alpha * p
        r -= alpha * q
        rho_new = float(r @ r)
        beta = rho_new / rho
        al.append(alpha)
        be.append(beta)
        p = r + beta * p
        rho = rho_new
    conv = rho == 0.0 or np.sqrt(rho) < tol
    return x, 0 if conv else maxiter, maxiter, np.array(al), np.array(be)


def tridiag_from_cg(alphas, betas):
    """(diagonal, off-diagonal) of the Lanczos T of the CG's Krylov space."""
    a = np.asarray(alphas, dtype=np.float64)
    b = np.asarray(betas, dtype=np.float64)
    k = a.size
    diag = 1.0 / a
    diag[1:] += b[:k - 1] / a[:k - 1]
    return diag, np.sqrt(b[:k - 1]) / a[:k - 1]


def slq_probe(A, z, steps):
    """|z|^2 e_1^T log(T) e_1 with T from `steps` CG iterations on A z-start."""
    _, _, _, al, be = cg_coeffs(lambda v: A @ v, z, rtol=0.0, atol=0.0, maxiter=steps)
    diag, off = tridiag_from_cg(al, be)
    return quadrature_logdet(diag, off, float(z @ z))


def dense_lml(A, y):
    """(LML, alpha, log det) of y ~ N(0, A)."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    L = np.linalg.cholesky(A)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, y))
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    return -0.5 * (float(y @ alpha) + logdet + y.size * np.log(2 * np.pi)), alpha, logdet
