"""Pins tests/masked_abi_ref.py (the long-double twins of the masked CG and
masked Lanczos, the first iterate's bound and the cases past the grid-stride
wrap) against dense K_oo algebra, and measures on the host what
tests/test_gpu_masked_abi.py scales its tolerances with: float64 NumPy's own
distance from the long-double twins, and its share of the first iterate's
bound.  No GPU."""
import numpy as np
import pytest

import masked_abi_ref as M
import masked_lanczos_ref as ml
import masked_ref as mr
import noise_ref as nr
from oracle import cg as ocg

LD = np.longdouble
VARIANTS = ["shift", "noise"]


def ids(ms):
    return "x".join(map(str, ms)) if isinstance(ms, tuple) else str(ms)


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2.0 ** -60


# ------------------------------------------------------------ the twins
@pytest.mark.parametrize("ms", [(7, 5, 3), (4, 3, 2)], ids=ids)
@pytest.mark.parametrize("precond", [None, "kron"])
def test_cg_twins_against_dense(ms, precond):
    """Converged, the long-double twins are the dense solves; their iteration
    counts are those of the float64 restatements they twin."""
    c = M.small_case(ms)
    F, b, mask, noise = c["F"], c["b"], c["mask"], c["noise"]
    x, info, it, rn = M.cg_ld(F, b, mask, shift=M.SHIFT, rtol=1e-12, precond=precond)
    want = mr.dense_solve(F, b, mask, M.SHIFT)
    _, info64, it64 = mr.masked_cg(F, b, mask, M.SHIFT, rtol=1e-12, precond=precond)
    print("cg_ld shift %s %s: %d iters (float64 %d), err vs dense %.2e"
          % (ms, precond, it, it64, M.rel(x, want)))
    assert info == 0 and info64 == 0 and M.rel(x, want) < 1e-10
    assert np.all(x[~mask] == 0) and abs(it - it64) <= max(1, 0.05 * it64)
    assert rn < 1e-12 * M.norm(np.where(mask, b, 0.0))
    x, info, it, rn = M.cg_ld(F, b, mask, noise=noise, rtol=1e-12, precond=precond)
    want = nr.dense_solve(F, b, mask, noise)
    _, info64, it64 = nr.weighted_cg(F, b, mask, noise, rtol=1e-12, precond=precond)
    print("cg_ld noise %s %s: %d iters (float64 %d), err vs dense %.2e"
          % (ms, precond, it, it64, M.rel(x, want)))
    assert info == 0 and info64 == 0 and M.rel(x, want) < 1e-10
    assert np.all(x[~mask] == 0) and abs(it - it64) <= max(1, 0.05 * it64)


def test_cg_twin_in_float64_is_the_restatement():
    """dtype=float64 runs the recurrence of masked_ref.masked_cg /
    noise_ref.weighted_cg: the same iterates to rounding."""
    c = M.small_case((12, 10, 8))
    F, b, mask, noise = c["F"], c["b"], c["mask"], c["noise"]
    x = M.cg_ld(F, b, mask, shift=M.SHIFT, rtol=0.0, maxiter=10, dtype=np.float64)[0]
    assert x.dtype == np.float64
    assert M.rel(x, mr.masked_cg(F, b, mask, M.SHIFT, rtol=0.0, maxiter=10)[0]) < 1e-12
    x = M.cg_ld(F, b, mask, noise=noise, rtol=0.0, maxiter=10, dtype=np.float64)[0]
    assert M.rel(x, nr.weighted_cg(F, b, mask, noise, rtol=0.0, maxiter=10)[0]) < 1e-12


@pytest.mark.parametrize("ms,steps", [((7, 5, 3), 8), ((4, 3, 2), 6)], ids=ids)
def test_lanczos_twins_against_dense(ms, steps):
    """The tridiagonal of the compressed dense matrix from the compressed
    probe, at the feature tests' 1e-8 (alphas) and 1e-7 (betas)."""
    c = M.small_case(ms)
    F, mask, noise = c["F"], c["mask"], c["noise"]
    a, b, done = M.lanczos_ld(F, mask, shift=M.SHIFT, seed=3, probe=2, steps=steps)
    da, db = ml.dense_masked_lanczos(F, mask, M.SHIFT, 3, 2, steps)
    assert done == steps and a.dtype == LD and len(b) == steps
    sc = float(np.max(np.abs(da)))
    assert np.max(np.abs(a - da)) <= 1e-8 * sc and np.max(np.abs(b[:steps - 1] - db)) <= 1e-7 * sc
    a, b, done = M.lanczos_ld(F, mask, noise=noise, seed=3, probe=2, steps=steps)
    A, o = nr.dense_A(F, mask, noise)
    da, db = ocg.lanczos_tridiag(A.dot, ocg.probe_signs(3, 2, mask.size)[o], steps)
    sc = float(np.max(np.abs(da)))
    assert done == steps
    assert np.max(np.abs(a - da)) <= 1e-8 * sc and np.max(np.abs(b[:steps - 1] - db)) <= 1e-7 * sc
    # the last beta, which the float64 restatements drop: |w| of the last step
    a64, b64 = nr.weighted_lanczos(F, mask, noise, 3, 2, steps + 1)
    assert abs(float(b[steps - 1]) - b64[steps - 1]) <= 1e-7 * sc


# ------------------------------------------------------- the first iterate
@pytest.mark.parametrize("ms", M.SMALL_SHAPES + M.WRAP_SHAPES, ids=ids)
def test_numpy_meets_first_iterate_bound(ms):
    """Float64 NumPy's first CG step inside the elementwise bound at every
    case of the device test; x and r exactly zero off the mask, where the
    bound is zero too."""
    c = M.cg_case(ms)
    for variant in VARIANTS:
        fi = M.first_case(ms, variant)
        kw = dict(shift=M.SHIFT) if variant == "shift" else dict(noise=c["noise"])
        x, r = M.first_iterate_f64(c["F"], c["b"], c["mask"], **kw)
        miss = ~c["mask"]
        assert np.all(fi["bx"][miss] == 0) and np.all(fi["br"][miss] == 0)
        assert np.all(fi["x"][miss] == 0) and np.all(fi["r"][miss] == 0)
        assert np.all(fi["bx"][c["mask"]] > 0) and np.all(fi["br"][c["mask"]] > 0)
        rx = M.R.worst_ratio(x, fi["x"], fi["bx"])
        rr = M.R.worst_ratio(r, fi["r"], fi["br"])
        print("numpy / bound, first iterate %s %s: x %.4f r %.4f (alpha_0 %.6g)"
              % (ms, variant, rx, rr, float(fi["alpha"])))
        assert rx <= 1.0 and rr <= 1.0, (ms, variant, rx, rr)
        if c["n"] < M.WRAP:      # the twin's first iteration is this iterate
            xt, _, it, rn = M.cg_ld(c["F"], c["b"], c["mask"], rtol=0.0, maxiter=1, **kw)
            assert it == 1 and M.rel(xt, fi["x"]) < 1e-17
            assert abs(rn - M.norm(fi["r"])) <= 1e-17 * rn


# ---------------------------------------------------------- the wrap cases
@pytest.mark.parametrize("ms", M.WRAP_SHAPES, ids=ids)
def test_wrap_masks(ms):
    n = int(np.prod(ms))
    assert n >= M.WRAP + 2 and (n % 2 == 1) == (ms == (103, 101, 101))
    for kind in ("cg", "lanczos"):
        c = M.wrap_case(ms, kind)
        mask = c["mask"]
        past = int(mask[M.WRAP:].sum())
        assert mask.size == n and not mask[0] and mask[n - 1]
        assert 4 * past >= int(mask.sum()), (past, int(mask.sum()))
        # split pairs in the second trip: one lane observed, its partner missing
        tail = mask[M.WRAP:M.WRAP + 2 * ((n - M.WRAP) // 2)].reshape(-1, 2)
        assert np.any(tail[:, 0] != tail[:, 1])
        assert c["noise"].shape == (n,) and np.all(c["noise"] > 0)
    assert not np.array_equal(M.wrap_case(ms, "cg")["mask"], M.wrap_case(ms, "lanczos")["mask"])


@pytest.mark.parametrize("ms", M.WRAP_SHAPES, ids=ids)
@pytest.mark.parametrize("family", ["cg", "cg_noise", "lz", "lz_noise"])
def test_wrap_figures(ms, family):
    """Float64 NumPy against the long-double twin after 3 iterations / steps:
    the unit of the device tolerances (100 x, floored at 1e-13).  Three steps
    of a recurrence whose first residual is |b| cannot lose six digits: a
    figure above 1e-11 (a device tolerance above 1e-9) would be a defect of
    the references, not a measurement."""
    t = M.wrap_twin(ms, family)
    if family.startswith("cg"):
        figs = (t["fig_x"], t["fig_rn"])
        print("float64 vs long double, %s %s, 3 iterations: x %.3e |r| %.3e"
              % (family, ms, figs[0], figs[1]))
        assert np.all(np.isfinite(np.asarray(t["x"], dtype=np.float64)))
        assert np.all(t["x"][~M.wrap_case(ms, "cg")["mask"]] == 0)
    else:
        figs = (t["fig_a"], t["fig_b"])
        print("float64 vs long double, %s %s, 3 steps: alphas %.3e betas %.3e"
              % (family, ms, figs[0], figs[1]))
        assert len(t["alphas"]) == len(t["betas"]) == M.WRAP_ITERS
        assert np.all(t["betas"] > 0)
    for f in figs:
        assert 0.0 <= f < 1e-11, figs
        assert 1e-13 <= M.tolerance(f) <= 1e-9


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precond", [None, "kron"])
def test_fixed_30_figures(variant, precond):
    """The same figure for the 30 unconverged iterations at (12, 10, 8), all
    four variants.  The preconditioned |r| is not monotone and carries the
    recurrence's rounding growth in full: its figure is the largest.  Every
    device tolerance (100 x) stays below the feature tests' 1e-3 for
    unconverged Krylov steps."""
    t = M.cg_twin((12, 10, 8), variant, precond, 30)
    print("float64 vs long double, (12, 10, 8) %s precond=%s, 30 iterations: x %.3e |r| %.3e"
          % (variant, precond, t["fig_x"], t["fig_rn"]))
    assert M.tolerance(t["fig_x"]) <= 1e-3 and M.tolerance(t["fig_rn"]) <= 1e-3


# ----------------------------------------------------- breakdown references
@pytest.mark.parametrize("where", ["last", "first"])
def test_one_observed_point(where):
    """One observed point i: v_0 = +-e_i, alpha_0 = K_ii + shift (or + noise_i),
    w_0 = A v_0 - alpha_0 v_0 is an exact zero, so one step is done."""
    ms = (7, 5, 3)
    c = M.small_case(ms)
    n = c["n"]
    i = n - 1 if where == "last" else 0
    mask = np.zeros(n, dtype=bool)
    mask[i] = True
    kii = np.prod([LD(f[j, j]) for f, j in zip(c["F"], np.unravel_index(i, ms))])
    for kw, add in ((dict(shift=M.SHIFT), LD(M.SHIFT)), (dict(noise=c["noise"]),
                                                         LD(c["noise"][i]))):
        for dtype in (LD, np.float64):
            a, b, done = M.lanczos_ld(c["F"], mask, seed=3, probe=2, steps=4, dtype=dtype, **kw)
            assert done == 1 and len(a) == 1 and len(b) == 1
            assert b[0] == 0.0
            assert abs(a[0] - (kii + add)) <= 8 * np.finfo(dtype).eps * (kii + add)


def test_steps_above_n_obs():
    """Six observed points, 12 steps: every entry finite, and n_obs times the
    quadrature is z_o^T log(K_oo + s I) z_o (the Krylov space is exhausted
    after at most six steps; what follows restarts from rounding noise with
    weights of the order of that beta squared)."""
    F = mr.rbf_factors(M.SIX_SHAPE)
    mask = np.zeros(int(np.prod(M.SIX_SHAPE)), dtype=bool)
    mask[M.SIX_POINTS] = True
    want = M.dense_quadratic_log(F, mask, M.SHIFT, 3, 2)
    for dtype in (LD, np.float64):
        a, b, done = M.lanczos_ld(F, mask, shift=M.SHIFT, seed=3, probe=2, steps=12, dtype=dtype)
        assert np.all(np.isfinite(a.astype(np.float64))) and np.all(np.isfinite(b.astype(np.float64)))
        got = 6 * M.quadrature(a, b, done)
        print("six points, 12 steps, %s: done %d, min beta %.2e, quadrature %.15g dense %.15g "
              "rel diff %.2e" % (dtype.__name__, done, float(np.min(b)), got, want,
                                 abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-9 * abs(want)
