"""The NumPy reference of structured kernel interpolation (tests/ski_ref.py)
pinned on the CPU: partition of unity, polynomial reproduction, selection rows
on the nodes, the convergence order of W K W^T, and the Lanczos tridiagonal
from CG coefficients."""
import numpy as np
import pytest

import oracle
from oracle.cg import probe_signs, quadrature_logdet  # noqa: F401
import ski_ref as sr

ORDERS = {"cubic": 4, "linear": 2}


def _grid(ms, lo=-0.3, hi=1.2):
    return [np.linspace(lo + 0.05 * f, hi + 0.1 * f, m) for f, m in enumerate(ms)]


def _points(xg, n, order, seed=0):
    """n uniform points in the interpolation domain of xg."""
    rng = np.random.default_rng(seed)
    X = np.empty((n, len(xg)))
    for f, g in enumerate(xg):
        lo, h, m = sr.axis_params(g)
        pad = h if order == 4 else 0.0
        X[:, f] = rng.uniform(lo + pad, lo + (m - 1) * h - pad, n)
    return X


@pytest.mark.parametrize("kind", ["cubic", "linear"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_rows_sum_to_one_and_reproduce_polynomials(kind, d):
    order = ORDERS[kind]
    xg = _grid([7, 5, 6, 4][:d])
    X = _points(xg, 40, order, seed=d)
    W = sr.dense_W(xg, X, order)
    assert np.max(np.abs(W.sum(axis=1) - 1.0)) < 1e-13
    # nodes in the grid layout: dimension 0 fastest
    mesh = np.meshgrid(*[np.asarray(g) for g in xg], indexing="ij")
    nodes = np.stack([a.reshape(-1, order="F") for a in mesh], axis=1)
    rng = np.random.default_rng(10 + d)
    c0, c1 = rng.standard_normal(), rng.standard_normal(d)
    C2 = rng.standard_normal((d, d)) if order == 4 else np.zeros((d, d))

    def poly(P):
        # cubic reproduces a quadratic (products of per-axis quadratics would
        # be of higher total degree: keep each axis's own square and the
        # bilinear cross terms), linear an affine function
        return c0 + P @ c1 + np.einsum("ni,ij,nj->n", P, C2, P)
    err = np.max(np.abs(W @ poly(nodes) - poly(X)))
    assert err < 1e-13, err


@pytest.mark.parametrize("kind", ["cubic", "linear"])
def test_points_on_nodes_give_selection_rows(kind):
    order = ORDERS[kind]
    # spacings that are exact in binary, so (x - lo) / h is an integer
    xg = [np.arange(6) * 0.5 - 1.0, np.arange(5) * 0.25]
    pad = 1 if order == 4 else 0
    idx = [(i, j) for i in range(pad, 6 - pad) for j in range(pad, 5 - pad)]
    X = np.array([[xg[0][i], xg[1][j]] for i, j in idx])
    W = sr.dense_W(xg, X, order)
    want = np.zeros_like(W)
    for r, (i, j) in enumerate(idx):
        want[r, i + 6 * j] = 1.0
    # the right domain edge (i = 6 - pad - 1, j = 5 - pad - 1) is among them
    assert np.array_equal(W, want)


def test_outside_is_counted_not_clamped():
    xg = [np.linspace(0, 1, 9)]
    h = 1.0 / 8
    X = np.array([[h - 1e-9 * h], [0.5], [1 - h + 1e-9 * h], [1 - h]])
    assert sr.stencils(xg, X, 4)[2] == 2
    with pytest.raises(ValueError):
        sr.dense_W(xg, X, 4)
    assert sr.stencils(xg, X, 2)[2] == 0


def test_gram_error_order():
    """W K W^T against the exact RBF Gram matrix (l = 0.3, 100 points on
    [0.1, 0.9], m nodes on [0, 1]): the error falls by more than 6x (cubic) and
    more than 3x (linear) per halving of h."""
    x = np.random.default_rng(0).uniform(0.1, 0.9, 100)
    exact = oracle.cov_1d("RBF", x, x, 1.0, 0.3)
    errs = {4: [], 2: []}
    for m in (12, 23, 45, 89):
        g = np.linspace(0, 1, m)
        Kg = oracle.cov_1d("RBF", g, g, 1.0, 0.3)
        for order in (4, 2):
            W = sr.dense_W([g], x[:, None], order)
            errs[order].append(np.max(np.abs(W @ Kg @ W.T - exact)))
    for order, ratio in ((4, 6.0), (2, 3.0)):
        e = errs[order]
        for a, b in zip(e[:-1], e[1:]):
            assert a / b > ratio, (order, e)
    assert errs[4][-1] < 1e-5 and errs[2][-1] < 1e-3


def test_tridiagonal_from_cg_equals_lanczos():
    rng = np.random.default_rng(3)
    n = 60
    B = rng.standard_normal((n, n))
    A = B @ B.T / n + 0.5 * np.eye(n)
    z = probe_signs(0, 0, n)
    steps = 20
    _, _, it, al, be = sr.cg_coeffs(lambda v: A @ v, z, rtol=0.0, atol=0.0, maxiter=steps)
    assert it == steps and al.size == steps
    diag, off = sr.tridiag_from_cg(al, be)
    la, lb = oracle.lanczos_tridiag(lambda v: A @ v, z, steps)
    assert np.max(np.abs(diag - la)) < 1e-10
    assert np.max(np.abs(off - lb)) < 1e-10
    q1 = quadrature_logdet(diag, off, float(n))
    q2 = quadrature_logdet(la, lb, float(n))
    assert abs(q1 - q2) < 1e-10 * abs(q2)
    assert abs(sr.slq_probe(A, z, steps) - q1) == 0.0


def test_cg_coeffs_is_the_oracle_cg():
    rng = np.random.default_rng(4)
    n = 40
    B = rng.standard_normal((n, n))
    A = B @ B.T / n + 0.1 * np.eye(n)
    b = rng.standard_normal(n)
    x0, info0, it0 = oracle.cg_solve(lambda v: A @ v, b, rtol=1e-9)
    x1, info1, it1, al, be = sr.cg_coeffs(lambda v: A @ v, b, rtol=1e-9)
    assert (info0, it0) == (info1, it1) and al.size == it1
    assert np.max(np.abs(x0 - x1)) < 1e-12 * np.max(np.abs(x0))


def test_dense_lml_matches_slogdet():
    xg = [np.linspace(0, 1, 8), np.linspace(0, 1, 7)]
    X = _points(xg, 30, 4, seed=5)
    W = sr.dense_W(xg, X, 4)
    A = sr.dense_wkw(W, sr.rbf_factors(xg, [0.3, 0.25])) + 0.1 * np.eye(30)
    y = np.random.default_rng(6).standard_normal(30)
    lml, alpha, logdet = sr.dense_lml(A, y)
    assert abs(logdet - np.linalg.slogdet(A)[1]) < 1e-10
    assert np.max(np.abs(A @ alpha - y)) < 1e-10
    assert abs(lml + 0.5 * (y @ alpha + logdet + 30 * np.log(2 * np.pi))) < 1e-12
