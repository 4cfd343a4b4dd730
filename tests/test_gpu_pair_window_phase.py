"""The x window of the block-basis CG applied in streaming phases
(blk_pair_lds_kernel, GG_CG_XWIN_PHASE = R).

With R >= 2 a workgroup of the pair launch applies the window only in every
R-th of its units, all of its waves streaming R units' shares of the armed
region in one pipelined loop; R = 1 keeps one visit per unit and wave.  The
schedule moves no element's arithmetic: x + sum_t c_t p_t[e] is formed in
the same order for every element, so every R gives x bitwise equal to R = 1.

Innermost order 72 (h = 36) is the smallest with the LDS pair launch; on 256
CUs its grid is at most 512 workgroups of 2 slabs.  (16, 40, 72, 72) has 1280
units, 2-3 per workgroup; (6, 12, 72, 72) 144, at most one per workgroup;
(2, 72, 72) 8 single-slab units on 8 workgroups.  Phases so fall on a full
group of units, on a leftover group in the last unit, and on a workgroup's
only unit.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


def grid_factor(m, ell, kind):
    g = np.linspace(0.0, 1.0, m)
    return oracle.cov_1d(kind, g, g, 1.0, ell) + 1e-12 * np.eye(m)


def factors(ms, seed=0):
    kinds = ["RBF", "Matern52", "RBF", "Matern32"]
    return [grid_factor(m, 0.1 + 0.03 * k + 0.01 * seed, kinds[k % len(kinds)])
            for k, m in enumerate(ms)]


def dev(gg, x):
    return gg.device.to_device(np.ascontiguousarray(x, dtype=np.float64).reshape(-1))


def host(gg, xd):
    return gg.device.to_host(xd).reshape(-1)


def oracle_cg(F, b, shift, rtol, maxiter):
    return oracle.cg_solve(lambda v: oracle.kron_matvec(F, v) + shift * v, b, rtol=rtol,
                           maxiter=maxiter)


def solver(gg, monkeypatch, F, shift, K, R):
    """A fresh operator and CG handle under window K and phase length R (the
    handles latch the knobs when they are made)."""
    monkeypatch.setenv("GG_CG_XWIN", str(K))
    if R is None:
        monkeypatch.delenv("GG_CG_XWIN_PHASE", raising=False)
    else:
        monkeypatch.setenv("GG_CG_XWIN_PHASE", str(R))
    s = gg.linalg.KronCG(gg.tensors.KronMatrix(F, sym=True), shift)
    assert s.basis == "block" and s.xwin == K
    return s


@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("ms", [(16, 40, 72, 72), (6, 12, 72, 72), (2, 72, 72)])
def test_phases_bitwise_equal_per_unit_schedule(gg, monkeypatch, ms, K):
    """37 iterations in one call: x of R = 2, 3, 8 equals R = 1's bitwise and
    the status (iterations, flag, residual, tolerance) is identical."""
    shift = 0.05
    F = factors(ms, 2)
    bd = dev(gg, np.random.default_rng(6).standard_normal(int(np.prod(ms))))
    runs = {}
    for R in (1, 2, 3, 8):
        s = solver(gg, monkeypatch, F, shift, K, R)
        s.start(bd, rtol=1e-14)
        s.iterate(37)
        runs[R] = (host(gg, s.x), s.status())
    x1, st1 = runs[1]
    assert st1[0] == 37
    assert np.all(np.isfinite(x1)) and np.linalg.norm(x1) > 0
    for R in (2, 3, 8):
        xr, st = runs[R]
        assert np.array_equal(xr, x1), (R, rel(xr, x1))
        assert st == st1, (R, st, st1)


def test_phases_open_chain_bitwise(gg, monkeypatch):
    """Open calls chain into one closed call bitwise at R = 3 (the armed
    region carries across calls whatever the phase schedule)."""
    ms, shift = (6, 12, 72, 72), 0.05
    F = factors(ms, 2)
    bd = dev(gg, np.random.default_rng(6).standard_normal(int(np.prod(ms))))
    a = solver(gg, monkeypatch, F, shift, 8, 3)
    a.start(bd, rtol=1e-14)
    a.iterate(37)
    xa = host(gg, a.x)
    c = solver(gg, monkeypatch, F, shift, 8, 3)
    c.start(bd, rtol=1e-14)
    for k in (5, 11, 1, 20):
        c.iterate(k, close=False)
    c.close()
    assert np.array_equal(host(gg, c.x), xa)
    assert a.status() == c.status() and a.status()[0] == 37


@pytest.mark.parametrize("R", [None, 3])
def test_phases_converge_inside_first_window(gg, monkeypatch, R):
    """A solve that converges in fewer iterations than the window (the ring of
    directions never fills: every phase takes fewer than K directions)."""
    ms, shift = (4, 8, 72, 72), 1e7   # (K + s I) ~ s I: a few iterations
    F = factors(ms, 5)
    b = np.random.default_rng(8).standard_normal(int(np.prod(ms)))
    s = solver(gg, monkeypatch, F, shift, 8, R)
    s.start(dev(gg, b), rtol=1e-8)
    s.iterate(8)
    it, conv, res, tol = s.status()
    xs, _, its = oracle_cg(F, b, shift, 1e-8, 1000)
    assert its < 8, its
    assert conv and it < 8 and abs(it - its) <= 1
    assert rel(host(gg, s.x), xs) < 1e-9


@pytest.mark.parametrize("R", [None, 3])
def test_phases_close_inside_first_window(gg, monkeypatch, R):
    """Three iterations and a close under window 8: the closing flush applies
    what the phases have not; x is the oracle CG's third iterate."""
    ms, shift = (4, 8, 72, 72), 0.2
    F = factors(ms, 5)
    b = np.random.default_rng(9).standard_normal(int(np.prod(ms)))
    s = solver(gg, monkeypatch, F, shift, 8, R)
    s.start(dev(gg, b), rtol=1e-14)
    s.iterate(3)
    assert s.status()[0] == 3
    xs, _, its = oracle_cg(F, b, shift, 1e-14, 3)
    assert its == 3
    assert rel(host(gg, s.x), xs) < 1e-9


@pytest.mark.parametrize("R", [None, 3])
@pytest.mark.parametrize("K", [3, 7])
def test_phases_region_edges(gg, monkeypatch, K, R):
    """(6, 10, 72, 72): the block layout holds 311040 doubles in 240
    single-slab units.  K = 3: regions of 103680, 432 per unit, no remainder.
    K = 7: 311040 is no multiple of 16 K; the regions of 44436 start off the
    128-byte lines, the last one is 12 short, and the units' shares of 192
    overshoot the region, so the last units' shares are clamped or empty.  x
    against the oracle CG to 1e-8 and the true residual at the tolerance."""
    ms, shift = (6, 10, 72, 72), 0.2
    F = factors(ms, 4)
    n = int(np.prod(ms))
    b = np.random.default_rng(11).standard_normal(n)
    s = solver(gg, monkeypatch, F, shift, K, R)
    s.start(dev(gg, b), rtol=1e-10)
    for _ in range(100):
        s.iterate(50)
        it, conv, res, tol = s.status()
        if conv:
            break
    assert conv
    x = host(gg, s.x)
    xs, info, its = oracle_cg(F, b, shift, 1e-10, 20000)
    assert info == 0
    assert abs(it - its) <= max(2, 0.02 * its), (it, its)
    assert rel(x, xs) < 1e-8
    r = oracle.kron_matvec(F, x) + shift * x - b
    assert np.linalg.norm(r) <= 1.5e-10 * np.linalg.norm(b)


def test_phases_block_sharded_range(gg, monkeypatch):
    """Two virtual ranks, 8 of the 16 blocks each (nblk < 2^d: a range's pair
    launch has its own unit count and region length), with the window in
    phases: the gathered solution equals the single-range solve's."""
    from dist_helpers import ThreadExchange, run_threads
    from gp_grief_amd.distributed import solve
    ms, shift = (6, 12, 72, 72), 0.2
    F = factors(ms, 3)
    n = int(np.prod(ms))
    b = np.random.default_rng(12).standard_normal(n)
    monkeypatch.setenv("GG_CG_XWIN", "8")
    monkeypatch.setenv("GG_CG_XWIN_PHASE", "3")
    K = gg.tensors.KronMatrix(F, sym=True)
    one = gg.linalg.KronCG(K, shift)
    assert one.basis == "block" and one.xwin == 8
    x1, info1 = gg.linalg.cg(K, b.reshape(-1, 1), shift=shift, rtol=1e-10, maxiter=20000)
    it1 = gg.linalg.cg.last.iters
    assert info1 == 0
    ex = ThreadExchange(2)

    def body(g):
        ex.bind(g)
        x, info, k, how = solve(K, b, shift, ex, rtol=1e-10, maxiter=20000, check_every=10,
                                decomposition="block")
        assert info == 0 and how == "block"
        return k, gg.device.to_host(x)

    k2, x2 = run_threads(2, body)[0]
    assert abs(k2 - it1) <= max(10, 0.02 * it1), (k2, it1)
    assert rel(x2, x1) < 1e-8
