"""The NumPy restatement of the Laplace approximation (laplace_ref.py) against
dense Newton on the CPU: the ground under test_gpu_laplace.py.

Six cases (laplace_ref.CASES x Poisson / binomial), newton_tol 1e-8 and the
CG to 1e-11: the inner tolerance bounds the mode's accuracy, so the CG-based
mode is held to 1e-8 of the dense one.
"""
import numpy as np
import pytest

import oracle
import laplace_ref as lr
import noise_ref as nr

ALL = [(ms, frac, amp, lik) for (ms, frac, amp) in lr.CASES for lik in lr.LIKELIHOODS]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_cg_newton_matches_dense_newton(ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    R = lr.mode(ms, frac, amp, lik, solve="cg", cg_rtol=1e-11)
    print(lik, ms, frac, "newton", R["iters"], "dense", D["iters"], "cg", R["cg_iters"],
          "halvings", R["halvings"], "a err", rel(R["a"], D["a"]), "f err", rel(R["f"], D["f"]),
          "ymax", C["y"].max(), "noise", R["noise"][C["mask"]].min(),
          R["noise"][C["mask"]].max())
    assert D["converged"] and R["converged"]
    assert rel(R["a"], D["a"]) < 1e-8
    assert rel(R["f"], D["f"]) < 1e-8
    assert np.all(R["a"][~C["mask"]] == 0)
    # psi rises over the accepted steps; the converging one is accepted on the
    # stop rule and may move psi by the rounding of its sums
    for X in (R, D):
        P = np.array(X["psis"])
        scale = abs(X["sums"][0]) + abs(X["const"]) + 0.5 * abs(X["sums"][1])
        assert np.all(np.diff(P[:-1]) > 0)
        assert P[-1] - P[-2] > -1e-13 * scale


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_mode_satisfies_a_equals_g(ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    m = C["mask"]
    _, g, _, _, _ = lr.point(C["kind"], C["y"][m], C["aux"][m], D["f"][m])
    assert np.linalg.norm(g - D["a"][m]) <= 1e-8 * max(1.0, np.linalg.norm(g))
    # a warm start from the mode takes no step
    W = lr.newton(C["F"], C["kind"], C["y"], C["aux"], m, solve="dense", a0=D["a"])
    assert W["converged"] and W["iters"] == 0


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_pseudo_target_identity(ms, frac, amp, lik):
    """The Gaussian posterior mean of the pseudo-targets b^ under noise 1 / w^
    is f^: K (K_oo + W^-1)^-1 b^ = K a^.  Away from the exact mode the two
    differ by K (K_oo + W^-1)^-1 W^-1 (g - a), linear in the stop rule's
    residual, so the identity is checked at a mode run to newton_tol 1e-10
    (where psi's resolution may end the run first: stalled counts)."""
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense", newton_tol=1e-10)
    assert D["converged"] or D["stalled"]
    alpha = nr.dense_solve(C["F"], D["b"], C["mask"], D["noise"])
    assert rel(oracle.kron_matvec(C["F"], alpha), D["f"]) < 1e-8


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_pass_selects_missing_points_away(lik):
    rng = np.random.default_rng(0)
    n = 105
    kind = lr.KINDS[lik]
    mask = nr.make_mask(n, 0.2)
    f, a = rng.uniform(-6, 6, n), rng.standard_normal(n)
    aux = rng.integers(1, 6, n).astype(np.float64)
    y = np.floor(rng.uniform(0, 1, n) * (aux + 1))
    ref = lr.newton_pass(kind, y, aux, f, a, mask)
    nan = lr.newton_pass(kind, np.where(mask, y, np.nan), np.where(mask, aux, np.nan), f, a, mask)
    for r, q in zip(ref, nan):
        assert np.array_equal(r, q)
    assert np.all(ref[0][~mask] == 1) and np.all(ref[1][~mask] == 0)
    # long double element outputs agree with the double ones to a few ulp
    pre = lr.newton_pass(kind, y, aux, f, a, mask, precise=True)
    assert np.allclose(pre[0], ref[0], rtol=1e-14, atol=0)
    _, _, w, _, _ = lr.point(kind, y, aux, f)
    assert np.all(np.abs(pre[1] - ref[1]) <= 1e-13 * (np.abs(f) + (np.abs(y) + w) / w))


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_slq_logdet_within_its_standard_error(ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    dense = nr.dense_logdet(C["F"], C["mask"], D["noise"])
    mean, ests = nr.weighted_slq(C["F"], C["mask"], D["noise"], probes=8, steps=50, seed=0)
    se = ests.std(ddof=1) / np.sqrt(ests.size)
    print(lik, ms, frac, "dense", dense, "slq", mean, "se", se, "z", (mean - dense) / se)
    assert abs(mean - dense) <= 4 * se
    lml_d = lr.laplace_lml(D["psi"], dense, D["sums"][2])
    assert np.isfinite(lml_d)
