"""The batched symmetric eigensolver (gg_sym_eig_batched and the tridiagonal
subset path) on the spectra a random dense matrix never shows it: zero
Householder columns (diagonal, block-diagonal and already tridiagonal input),
exactly repeated eigenvalues, close pairs, ill-conditioned RBF factors, extreme
scaling, every size around the LDS / HBM switch, and launches whose factors
differ in size.

Bars are the project's own.  Full path (test_device_eigensolver): eigenvalues,
Q^T Q - I and Q diag(lam) Q^T - A within 1e-12 * max(1, m / 10) (times
scale = max|lambda| where the quantity carries the matrix's scale).  Subset
path (test_eig_subset_vs_full): eigenvalues within 1e-13 * scale * m, selected
rows orthonormal to 1e-12, eigen-residual within 1e-12 * scale.  Eigenvectors
are never compared entrywise (repeated eigenvalues leave them non-unique).
The reference is LAPACK's eigvalsh, or the closed form where there is one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tens(gpu):
    from gp_grief_amd import tensors
    return tensors


# ------------------------------------------------------------------ matrices
def _rand_sym(m, seed):
    A = np.random.default_rng(seed).standard_normal((m, m))
    return A + A.T


def _rbf(m, ls):
    g = np.linspace(0, 1, m)
    return np.exp(-0.5 * (g[:, None] - g[None, :]) ** 2 / ls ** 2) + 1e-12 * np.eye(m)


def _toeplitz(m):
    return 2.0 * np.eye(m) - np.eye(m, k=1) - np.eye(m, k=-1)


def _toeplitz_eigs(m):
    return np.sort(2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1)))


def _block_diag(m, seed):
    """Two random dense symmetric blocks of unequal size: the tridiagonal form
    has a zero off-diagonal where they meet."""
    m1 = max(1, m // 3)
    A = np.zeros((m, m))
    A[:m1, :m1] = _rand_sym(m1, seed)
    A[m1:, m1:] = _rand_sym(m - m1, seed + 1)
    return A


def _wilkinson(m=21):
    h = (m - 1) // 2
    return np.diag(np.abs(np.arange(-h, h + 1)).astype(np.float64)) + np.eye(m, k=1) + \
        np.eye(m, k=-1)


def _glued_wilkinson(coupling=1e-8):
    W = _wilkinson(21)
    A = np.zeros((42, 42))
    A[:21, :21] = W
    A[21:, 21:] = W
    A[20, 21] = A[21, 20] = coupling
    return A


def kinds(m):
    """name -> (matrix, reference eigenvalues ascending, well separated?)"""
    rng = np.random.default_rng(1000 + m)
    out = {}
    out["cI"] = (2.5 * np.eye(m), np.full(m, 2.5), False)
    out["zero"] = (np.zeros((m, m)), np.zeros(m), False)
    d = rng.permutation(np.arange(1, m + 1) * 0.75 - 0.3 * m)
    out["diag_distinct"] = (np.diag(d), np.sort(d), True)
    dr = d.copy()
    dr[m // 4:m // 4 + max(2, m // 3)] = 1.25           # a repeated block
    out["diag_repeated"] = (np.diag(dr), np.sort(dr), False)
    out["toeplitz"] = (_toeplitz(m), _toeplitz_eigs(m), True)
    B = _block_diag(m, 2000 + m)
    out["block_diag"] = (B, np.linalg.eigvalsh(B), True)
    v = rng.standard_normal(m)
    vv = float(v.dot(v))
    out["rank_one"] = (np.outer(v, v), np.concatenate([np.zeros(m - 1), [vv]]), False)
    out["eye_plus_rank_one"] = (np.eye(m) + np.outer(v, v),
                                np.concatenate([np.ones(m - 1), [1.0 + vv]]), False)
    for name, ls in (("rbf_1e-4", 1e-4), ("rbf_1", 1.0)):
        R = _rbf(m, ls)
        out[name] = (R, np.linalg.eigvalsh(R), False)
    S = _rand_sym(m, 3000 + m)
    w = np.linalg.eigvalsh(S)
    out["rand"] = (S, w, True)
    out["rand_2^200"] = (S * 2.0 ** 200, w * 2.0 ** 200, True)
    out["rand_2^-200"] = (S * 2.0 ** -200, w * 2.0 ** -200, True)
    return out


# ------------------------------------------------------------------ checks
def check_full(name, A, w, q, lam):
    m = A.shape[0]
    scale = np.abs(w).max()
    bar = 1e-12 * max(1, m / 10)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(q)), name
    assert np.all(np.diff(lam) >= 0), name
    if scale == 0.0:
        assert np.all(lam == 0.0), name
    assert np.max(np.abs(lam - w)) <= bar * scale, (name, np.max(np.abs(lam - w)) / max(scale, 1e-300))
    assert np.max(np.abs(q.T.dot(q) - np.eye(m))) < bar, name
    # scaled before the product so 2^+-200 neither overflows nor underflows
    s = scale if scale > 0 else 1.0
    assert np.max(np.abs((q * (lam / s)).dot(q.T) - A / s)) <= bar, name


def check_eigenvalues_subset(name, w, lam):
    m = w.size
    scale = np.abs(w).max()
    assert np.all(np.isfinite(lam)), name
    assert np.all(np.diff(lam) >= 0), name
    if scale == 0.0:
        assert np.all(lam == 0.0), name
    assert np.abs(lam - w).max() <= 1e-13 * scale * m, (name, np.abs(lam - w).max() / max(scale, 1e-300))


def separated(w, sel, tol=1e-6):
    """Every selected eigenvalue at least tol * scale from its neighbours: the
    precondition of the subset vectors (the header: the caller guarantees
    separation; the models use 1e-10)."""
    w = np.asarray(w)
    gaps = np.diff(w)
    t = tol * np.abs(w).max()
    return all((k == 0 or gaps[k - 1] >= t) and (k == w.size - 1 or gaps[k] >= t) for k in sel)


def check_vectors_subset(name, A, w, lam, sel, V):
    m = A.shape[0]
    sel = np.asarray(sel, dtype=np.int64)
    assert V.shape == (sel.size, m), name
    if sel.size == 0:
        return
    assert separated(w, sel), name
    scale = np.abs(w).max()
    assert np.all(np.isfinite(V)), name
    assert np.abs(V.dot(V.T) - np.eye(sel.size)).max() < 1e-12, name
    s = scale if scale > 0 else 1.0
    assert np.abs(V.dot(A / s) - (lam[sel] / s)[:, None] * V).max() < 1e-12, name


def run_full(tens, cases):
    names = list(cases)
    Q, lam = tens.device_sym_eig([cases[k][0] for k in names])
    for k, q, l in zip(names, Q, lam):
        check_full(k, cases[k][0], cases[k][1], np.asarray(q), l)


def run_subset(tens, cases, selections):
    names = list(cases)
    lam, h = tens.device_sym_eig_tridiag([cases[k][0] for k in names])
    for k, l in zip(names, lam):
        check_eigenvalues_subset(k, cases[k][1], l)
    V = tens.device_sym_eig_tridiag_vectors(h, [selections[k] for k in names])
    for k, l, v in zip(names, lam, V):
        check_vectors_subset(k, cases[k][0], cases[k][1], l, selections[k], v.cpu().numpy())


def spread_selection(m):
    """Index 0, index m - 1 and a few between."""
    return sorted(set([0, m - 1, m // 2, m // 3, min(m - 1, 1)]))


# ------------------------------------------------------------------ matrix kinds
@pytest.mark.parametrize("m", [3, 4, 33, 128, 129])
def test_kinds_full(tens, m):
    run_full(tens, kinds(m))


@pytest.mark.parametrize("m", [3, 4, 33, 128, 129])
def test_kinds_subset(tens, m):
    """Bisection eigenvalues for every kind; inverse-iteration vectors for the
    well-separated ones only."""
    cases = kinds(m)
    sels = {k: (spread_selection(m) if c[2] else []) for k, c in cases.items()}
    sels["toeplitz"] = list(range(m))          # a full selection
    run_subset(tens, cases, sels)


def test_wilkinson(tens):
    """W21+ (its largest eigenvalues agree to ~1e-14) and two copies glued with
    coupling 1e-8 (every eigenvalue doubled to ~1e-8 or closer)."""
    W, G = _wilkinson(21), _glued_wilkinson()
    cases = {"wilkinson21": (W, np.linalg.eigvalsh(W), False),
             "glued_wilkinson": (G, np.linalg.eigvalsh(G), False)}
    run_full(tens, cases)
    # W21+'s lower eigenvalues are well separated; the top pairs are not
    w = cases["wilkinson21"][1]
    low = [k for k in range(8) if separated(w, [k])]
    assert 0 in low
    run_subset(tens, cases, {"wilkinson21": low, "glued_wilkinson": []})


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("m", [1, 2, 3, 4, 127, 128, 129, 255, 256, 257, 512, 1024])
def test_sizes(tens, m):
    """Around the LDS / HBM switch (kLdsMaxM = 128) and up: a random symmetric
    matrix and an RBF factor, full and subset paths."""
    S, R = _rand_sym(m, m), _rbf(m, 0.15)
    cases = {"rand": (S, np.linalg.eigvalsh(S), True), "rbf": (R, np.linalg.eigvalsh(R), False)}
    run_full(tens, cases)
    top = [k for k in range(max(0, m - 6), m) if separated(cases["rbf"][1], [k])]
    run_subset(tens, cases, {"rand": spread_selection(m), "rbf": top})


def test_ceiling_2048_subset(tens):
    """m = 2048, the contract's ceiling, on the subset path (1.2 s measured on
    an MI355X).  The full QL path takes 13 s there -- one workgroup per matrix
    -- so 1024 stays its largest size in this file."""
    m = 2048
    S = _rand_sym(m, m)
    run_subset(tens, {"rand": (S, np.linalg.eigvalsh(S), True)}, {"rand": spread_selection(m)})


def test_size_limit_rejected(tens):
    """m = 2049 is past the contract's ceiling: GG_ERR_VALUE from both paths."""
    A = np.eye(2049)
    with pytest.raises(ValueError):
        tens.device_sym_eig([A])
    with pytest.raises(ValueError):
        tens.device_sym_eig_tridiag([A])


# ------------------------------------------------------------------ mixed batches
def _mixed(sizes, names):
    out = {}
    for m, name in zip(sizes, names):
        out["%s_%d" % (name, m)] = kinds(m)[name]
    return out


LDS_SIZES = [5, 128, 33, 1, 64]
HBM_SIZES = [3, 200, 64, 129, 1]


@pytest.mark.parametrize("sizes,names", [
    (LDS_SIZES, ["rank_one", "rand", "diag_repeated", "rand", "rbf_1"]),
    (HBM_SIZES, ["cI", "rbf_1", "toeplitz", "block_diag", "diag_distinct"]),
], ids=["lds", "hbm"])
def test_mixed_batch_full(tens, sizes, names):
    """Factors of different size and kind in one launch: the per-factor offset
    tables, LDS sized from the largest, one kernel variant for the batch."""
    run_full(tens, _mixed(sizes, names))


@pytest.mark.parametrize("sizes,names", [
    (LDS_SIZES, ["toeplitz", "rand", "diag_distinct", "rand", "block_diag"]),
    (HBM_SIZES, ["toeplitz", "rand", "diag_distinct", "block_diag", "rand"]),
], ids=["lds", "hbm"])
def test_mixed_batch_subset(tens, sizes, names):
    cases = _mixed(sizes, names)
    keys = list(cases)
    sels = {}
    for i, (k, m) in enumerate(zip(keys, sizes)):
        sels[k] = spread_selection(m)
    sels[keys[0]] = list(range(sizes[0]))      # full selection (well separated)
    sels[keys[2]] = []                         # an empty selection inside the batch
    run_subset(tens, cases, sels)


def test_mixed_batch_jacobi(tens, monkeypatch):
    """GG_EIG=jacobi is kept as the A/B reference: it stays right on a mixed
    batch too."""
    from gp_grief_amd import native
    monkeypatch.setenv("GG_EIG", "jacobi")
    native.knobs_reload()
    try:
        run_full(tens, _mixed(LDS_SIZES, ["rank_one", "rand", "diag_repeated", "rand", "rbf_1"]))
    finally:
        monkeypatch.delenv("GG_EIG")
        native.knobs_reload()
