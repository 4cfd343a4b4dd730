"""laplace_abi_ref.py held to itself on the CPU: the ground under
test_gpu_laplace_abi.py.

The double-precision restatement (laplace_ref.point / newton_pass) is compared
with the long-double evaluation at the edge rows to the tolerances the device
is held to (noise 1e-14 relative; b 1e-14 (|f| + (|y| + w) / w); sums 1e-12 of
the sum of the absolute terms), so the reference alone stays inside them,
denormal corners included.  Measured: noise 2.1e-16 for both kinds; b 0.017 of
its bound for the Poisson and 0.034 for the binomial over the rows where the
bound is at least half the spacing of the doubles at b.  The 32 binomial rows
with y = 0 and f >= 36 are below that (b = f - 1 - exp(f), bound 1e-14 (f + 1)):
there plain double arithmetic is 1 ulp of b from the long-double value (at f =
36, 1.35e12 times the stated bound), and the restatement is held to
laplace_abi_ref.B_ULPS on those rows; the device, which forms exp(f) to 2^-64
there, is held to the stated bound on every row.

The driver cases of test_gpu_laplace_abi.py are conditioned here, so that the
device tests cannot pass vacuously.
"""
import numpy as np
import pytest

import laplace_ref as lr
import laplace_abi_ref as ar

KINDS = [lr.POISSON, lr.BINOMIAL]
TINY = np.finfo(np.float64).tiny


def double_pass(kind, E, rows):
    """The double-precision restatement over some rows of edge_points."""
    y, e, f, a = (E[k][rows] for k in ("y", "e", "f", "a"))
    return (y, e, f, a) + tuple(lr.newton_pass(kind, y, e, f, a)[:3])


@pytest.mark.parametrize("kind", KINDS)
def test_edge_points_cover_the_branches(kind):
    E = ar.edge_points(kind)
    f, e, y = E["f"], E["e"], E["y"]
    for v in ar.EDGE_F:
        assert np.any(f == v) and np.any(f == -v)
    assert np.any((f == 0) & np.signbit(f)) and np.any((f == 0) & ~np.signbit(f))
    assert np.any(f == np.nextafter(700.0, np.inf)) and np.any(f == np.nextafter(-700.0, -np.inf))
    assert np.any(~E["given"]) and np.all(e[~E["given"]] == 1.0)
    for v in (1e-4, 1.0, 1e4):
        assert np.any(E["given"] & (e == v))
    assert np.any(y == 0) and np.any(y == e) and np.any((y > 0) & (y != e))
    if kind == lr.BINOMIAL:
        assert np.all(y <= e) and not E["designated"].any()
    # the long-double b rounds to a finite double everywhere but at the
    # designated row, where it is +inf while the noise is still finite
    R = ar.pass_ref(kind, y, e, f, E["a"])
    assert np.array_equal(~np.isfinite(R["b"]), E["designated"])
    if kind == lr.POISSON:
        d = E["designated"]
        assert d.sum() == 1 and R["b"][d][0] == np.inf and np.isfinite(R["noise"][d][0])
        assert abs(f[d][0]) <= ar.CLAMP and 1e-4 <= e[d][0] <= 1e4


@pytest.mark.parametrize("kind", KINDS)
def test_noise_is_finite_and_positive_in_the_documented_range(kind):
    E = ar.edge_points(kind)
    R = ar.pass_ref(kind, E["y"], E["e"], E["f"], E["a"])
    inr = (np.abs(E["f"]) <= ar.CLAMP) & (E["e"] >= 1e-4) & (E["e"] <= 1e4)
    noise = R["noise"][inr]
    print("kind", kind, "noise in", noise.min(), noise.max(), "normal from", TINY)
    assert np.all(np.isfinite(noise)) and np.all(noise > 0)
    # beyond the clamp the noise is that of +-700, so the same holds there
    assert np.all(np.isfinite(R["noise"])) and np.all(R["noise"] > 0)
    Rc = ar.pass_ref(kind, E["y"], E["e"], ar.clamped(E["f"]), E["a"])
    assert np.array_equal(R["noise"], Rc["noise"])
    if kind == lr.POISSON:
        # by a hair: both corners of the range are denormal on one side
        assert noise.max() > 1e308 and noise.min() < TINY


@pytest.mark.parametrize("kind", KINDS)
def test_double_restatement_within_the_device_tolerances(kind):
    E = ar.edge_points(kind)
    worst = dict(noise=0.0, b_reach=0.0, b_ulps=0.0, b=0.0)
    for v in ar.EDGE_F:
        for sign in (False, True):
            rows = (np.abs(E["f"]) == v) & (np.signbit(E["f"]) == sign)
            y, e, f, a, noise, b, sums = double_pass(kind, E, rows)
            R = ar.pass_ref(kind, y, e, f, a)
            err = ar.pass_errors(R, noise, b, sums)
            for k in worst:
                worst[k] = max(worst[k], err[k])
            assert not err["nan"] and err["classes"], (v, sign)
            assert err["noise"] <= ar.NOISE_RTOL
            assert err["b_reach"] <= 1.0
            assert err["b_ulps"] <= ar.B_ULPS
            assert np.all(err["sums"] <= ar.SUM_TOL), (v, sign, err["sums"])
    print("kind", kind, worst)
    if kind == lr.POISSON:
        assert worst["b"] <= 1.0     # no row below the spacing of b


def test_binomial_sums_are_finite_for_every_finite_f():
    E = ar.edge_points(lr.BINOMIAL)
    huge = np.array([1e4, 1e300, np.finfo(np.float64).max])
    f = np.concatenate([E["f"], huge, -huge])
    e = np.concatenate([E["e"], np.ones(6)])
    y = np.concatenate([E["y"], np.array([0.0, 1.0, 0.5, 0.0, 1.0, 0.5])])
    a = np.zeros(f.size)
    for i in range(f.size):
        for sums in (lr.newton_pass(lr.BINOMIAL, y[i:i + 1], e[i:i + 1], f[i:i + 1], a[i:i + 1])[2],
                     ar.pass_ref(lr.BINOMIAL, y[i:i + 1], e[i:i + 1], f[i:i + 1],
                                 a[i:i + 1])["sums"]):
            assert np.all(np.isfinite(sums)), (y[i], e[i], f[i], sums)


def test_poisson_overflow_lands_in_three_sums():
    E = ar.edge_points(lr.POISSON)
    over = E["f"] > ar.EXP_OVERFLOW
    assert over.sum() >= 3 * 12
    for i in np.nonzero(over)[0]:
        s = slice(i, i + 1)
        for sums in (lr.newton_pass(lr.POISSON, E["y"][s], E["e"][s], E["f"][s], E["a"][s])[2],
                     ar.pass_ref(lr.POISSON, E["y"][s], E["e"][s], E["f"][s], E["a"][s])["sums"]):
            assert sums[0] == -np.inf and sums[3] == np.inf and sums[4] == np.inf
            assert np.isfinite(sums[1]) and np.isfinite(sums[2])
    # up to the overflow of exp the rate is finite: sums[0] is, and the squares
    # of g overflow on their own
    i = int(np.nonzero(E["f"] == np.nextafter(700.0, np.inf))[0][0])
    sums = ar.pass_ref(lr.POISSON, E["y"][i:i + 1], E["e"][i:i + 1], E["f"][i:i + 1],
                       E["a"][i:i + 1])["sums"]
    assert np.isfinite(sums[0]) and sums[0] < -1e300 and sums[4] == np.inf


@pytest.mark.parametrize("kind", KINDS)
def test_response_ref(kind):
    n = 8
    F, W = ar.response_values(kind, n)
    mean, m2, same = ar.response_ref(kind, F, W)
    r = ar.response(kind, F + W, dtype=np.float64)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(m2)) and np.all(m2 >= 0)
    # against the two-pass moments of the double responses
    two = np.sum((r - r.mean(axis=0)) ** 2, axis=0)
    assert np.allclose(mean, r.mean(axis=0), rtol=1e-14, atol=5e-324)
    assert np.allclose(m2[~same], two[~same], rtol=1e-13, atol=0)
    assert np.all(two[same] == 0)
    # +0 and -0, and the saturated columns, are flagged equal
    assert same[0] and same[1] and mean[0] == (1.0 if kind == lr.POISSON else 0.5)
    if kind == lr.BINOMIAL:
        assert same[2] and mean[2] == 1.0 and same[4] and mean[4] == 1.0
        assert not same[3] and 0 < mean[3] < 1e-17 and m2[3] > 0
        assert same[5] and mean[5] == 0.0
    else:
        assert same[2] and np.isfinite(mean[2]) and mean[2] > 1e303
        assert not same[3] and same[4] and 0 < mean[4] < TINY
    assert not same[6:].any()


# ------------------------------------------------------------ the driver cases
def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def test_halving_case():
    D, R = ar.driver_run("halving", solve="dense"), ar.driver_run("halving")
    print("halvings dense", D["halvings"], "cg", R["halvings"])
    assert D["converged"] and R["converged"]
    assert max(R["halvings"]) >= 1 and R["halvings"] == D["halvings"]
    assert rel(R["a"], D["a"]) < 1e-8


def test_overflow_case():
    D, R = ar.driver_run("overflow", solve="dense"), ar.driver_run("overflow")
    trial = ar.first_trial_sums("overflow")
    print("halvings dense", D["halvings"], "cg", R["halvings"], "first trial", trial)
    assert not np.all(np.isfinite(trial)) and not np.isnan(trial).any()
    assert trial[0] == -np.inf and np.isfinite(trial[1])
    assert D["converged"] and R["converged"]
    assert R["halvings"][0] == D["halvings"][0] >= 1
    # margin under max_halvings = 20: the reference alone never exhausts it
    assert max(R["halvings"]) <= 18 and max(D["halvings"]) <= 18
    assert rel(R["a"], D["a"]) < 1e-8


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_stall_case(lik):
    case = ((7, 5, 3), 0.2, 1.0, lik)
    D = lr.mode(*case, solve="dense")
    S = lr.mode(*case, solve="cg", cg_rtol=1e-11, newton_tol=1e-14)
    print(lik, "iters", S["iters"], "halvings", S["halvings"])
    assert S["stalled"] and not S["converged"] and S["iters"] < 50
    assert rel(S["a"], D["a"]) < 1e-6


def test_cut_off_cases():
    C = ar.driver_case("halving")
    D = ar.driver_run("halving", solve="dense")
    M = ar.driver_run("halving", max_newton=2)
    assert M["iters"] == 2 and len(M["cg_iters"]) == 2
    assert not M["converged"] and not M["stalled"]
    W = lr.newton(C["F"], C["kind"], C["y"], C["aux"], C["mask"], cg_rtol=1e-11, a0=M["a"])
    assert W["converged"] and rel(W["a"], D["a"]) < 1e-6
    H = ar.driver_run("halving", max_halvings=0)
    assert H["stalled"] and not H["converged"] and H["iters"] == 0 and H["halvings"] == []
    assert np.all(H["a"] == 0)


def test_warm_start_is_zeroed_at_missing_points():
    C = ar.driver_case("halving")
    M = ar.driver_run("halving", max_newton=2)
    m = C["mask"]
    runs = []
    for fill in (0.0, np.nan, 7.0):
        R = lr.newton(C["F"], C["kind"], C["y"], C["aux"], m, cg_rtol=1e-11,
                      a0=np.where(m, M["a"], fill))
        assert np.all(R["a"][~m] == 0)
        runs.append(R["a"])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_kron_preconditioned_case(lik):
    case = ((7, 5, 3), 0.2, 1.0, lik)
    D = lr.mode(*case, solve="dense")
    P = lr.mode(*case, solve="cg", cg_rtol=1e-11, precond="kron")
    assert P["converged"] and rel(P["a"], D["a"]) < 1e-8
