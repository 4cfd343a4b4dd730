"""blk_mode_fast_kernel with two column strips per wave (GG_BLK_MODE_STRIPS).

The switch is a mask read when the operator is created: bit 0 the plain mode
launches, bit 1 the CG prologues (stored and derived r); 0 runs one strip per
wave everywhere (the Lanczos prologue always does).  A wave that owns two strips
issues, per output element, the k-steps of the one-strip kernel in the same
order from the same fragments, so everything a launch writes to a vector is
bitwise what mask 0 writes; only the r.r / p.q_old partials group over
another grid.  Shapes: the smallest that reach each path -- odd and even strip
counts per row (the odd ones end every row in a half window), TF = 1, 2 and
the bench's TF = 6, a block range that starts inside the vector.
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


def grid_factor(m, ell=0.15, kind="RBF"):
    g = np.linspace(0.0, 1.0, m)
    return oracle.cov_1d(kind, g, g, 1.0, ell) + 1e-12 * np.eye(m)


def factors(ms, seed=0):
    kinds = ["RBF", "Matern52", "RBF", "Matern32", "RBF", "Exponential"]
    return [grid_factor(m, 0.1 + 0.03 * k + 0.01 * seed, kinds[k % len(kinds)])
            for k, m in enumerate(ms)]


def dev(gg, x):
    return gg.device.to_device(np.ascontiguousarray(x, dtype=np.float64).reshape(-1))


def host(gg, xd):
    return gg.device.to_host(xd).reshape(-1)


def operator(gg, monkeypatch, F, mask):
    monkeypatch.setenv("GG_BLK_MODE_STRIPS", str(mask))
    return gg.tensors.KronMatrix(F, sym=True)


# strips per row (inner / 16) of the mode launches:
#   (40,) * 3     axis 0: 25, odd
#   (40,) * 4     axis 0: 500, even; axis 1: 25, odd
#   (72,) * 4     TF 2; axis 0: 2916, even; axis 1: 81, odd
#   (200,) * 3    TF 6, the bench's instantiation; axis 0: 625, odd
SHAPES = [(40, 40, 40), (40, 40, 40, 40), (72, 72, 72, 72), (200, 200, 200)]


@pytest.mark.parametrize("ms", SHAPES)
def test_plain_two_strips_bitwise_and_oracle(gg, monkeypatch, ms):
    """The block matvec with bit 0 on is the mask-0 matvec bitwise, and the
    oracle's to test_gpu_block.py's 1e-13."""
    F = factors(ms)
    n = int(np.prod(ms))
    xb = oracle.kron.block_fold(np.random.default_rng(2).standard_normal(n), ms)
    y = {}
    for mask in (0, 1):
        K = operator(gg, monkeypatch, F, mask)
        y[mask] = host(gg, K._device().block_matvec(dev(gg, xb), shift=0.05))
    assert np.array_equal(y[0], y[1])
    assert rel(y[1], oracle.kron.block_matvec(F, xb) + 0.05 * xb) < 1e-13


def test_plain_two_strips_block_range(gg, monkeypatch):
    """Blocks [3, 6) of 8 (the block-sharded engine's range): the range starts
    inside the vector, crosses axis 0's parity bit between blocks 3 and 4, and
    a block's 13 windows are no multiple of the workgroup's 8, so every block
    ends in spare windows; the last window of every row is half valid."""
    ms = (40, 40, 40)
    F = factors(ms, 1)
    n = int(np.prod(ms))
    nb = n >> 3
    xb = oracle.kron.block_fold(np.random.default_rng(3).standard_normal(n), ms)
    ref = oracle.kron.block_matvec(F, xb) + 0.02 * xb
    y = {}
    for mask in (0, 1):
        dk = operator(gg, monkeypatch, F, mask)._device()
        y[mask] = host(gg, dk.block_matvec_range(dev(gg, xb[3 * nb:6 * nb]), 3, 3, shift=0.02))
    assert np.array_equal(y[0], y[1])
    assert rel(y[1], ref[3 * nb:6 * nb]) < 1e-13


def test_cg_plain_bit_bitwise_history(gg, monkeypatch):
    """The plain launch carries no dot products: a fused CG with only bit 0
    on has bitwise the x and the residual history of mask 0 (30 iterations,
    rtol 0, the residual read after every chunk)."""
    ms, shift = (40, 40, 40, 40), 0.5
    F = factors(ms)
    b = np.random.default_rng(4).standard_normal(int(np.prod(ms)))
    out = {}
    for mask in (0, 1):
        s = gg.linalg.KronCG(operator(gg, monkeypatch, F, mask), shift)
        assert s.basis == "block"
        s.start(dev(gg, b), rtol=0.0)
        hist = []
        for k in (1, 2, 3, 5, 8, 11):
            s.iterate(k)
            hist.append(s.status())
        out[mask] = (host(gg, s.x), hist)
    assert out[0][1] == out[1][1] and out[1][1][-1][0] == 30
    assert np.array_equal(out[0][0], out[1][0])


# derived r comes with the x window, which the LDS pair launch carries: pair
# order >= 72.  Axis 0's strips per row: 25 (odd) at pair order 40, 81 (odd)
# at (., 72, 72), 486 (even) at (., 6, 72, 72); (200, 72, 72) is TF = 6.
@pytest.mark.parametrize("ms,rderive", [((40, 40, 40), "0"), ((40, 40, 40, 40), "0"),
                                        ((40, 72, 72), "0"), ((40, 72, 72), "1"),
                                        ((40, 6, 72, 72), "1"), ((200, 72, 72), "1")])
def test_cg_prologue_two_strips_first_launch_bitwise(gg, monkeypatch, ms, rderive):
    """One open iteration from the same start.  The first prologue's scalars
    are the start's, the same in both runs, so everything the iteration writes
    (p, the prologue's Y -- at d = 3 the chain buffer keeps it -- and q) is
    bitwise mask 0's: the whole workspace is compared."""
    monkeypatch.setenv("GG_CG_RDERIVE", rderive)
    shift = 0.3
    F = factors(ms, 2)
    b = np.random.default_rng(5).standard_normal(int(np.prod(ms)))
    out = {}
    for mask in (0, 2):
        s = gg.linalg.KronCG(operator(gg, monkeypatch, F, mask), shift)
        assert s.basis == "block" and s.rderive == (rderive == "1")
        s.work.zero_()
        s.start(dev(gg, b), rtol=0.0)
        s.iterate(1, close=False)
        out[mask] = host(gg, s.work).copy()
        s.close()
    assert np.array_equal(out[0], out[2])


@pytest.mark.parametrize("ms,rderive", [((40, 40, 40), False), ((40, 72, 72), True),
                                        ((200, 72, 72), True)])
def test_cg_prologue_two_strips_totals_and_second_launch(gg, monkeypatch, ms, rderive):
    """The prologue's own sums, read where a block-sharded rank reads them
    (gg_cg_iterate_partial's red[5] = [r.r, p.q_old, p.q, r.q, q.q]), on the
    rank that owns blocks 4..7 of 8 (blk0 != 0).  Iteration 1: the prologue
    sums nothing yet and the pair launch's sums come from bitwise equal
    vectors, so red and the workspace are bitwise mask 0's -- and with them the
    scalars iterate_finish hands to iteration 2.  Iteration 2 therefore runs
    its prologue on real alpha and beta that are the same in both runs: the
    workspace (p, Y, q) is bitwise equal again, the pair launch's three sums
    too, and r.r and p.q_old, summed over another grid of workgroups with the
    half windows' and spare windows' lanes masked out, agree to 1e-13
    relative.  For r.r, a sum of squares, that is relative to the sum.
    p.q_old = p_j . K p_{j-1} is zero in exact arithmetic (the directions are
    conjugate): what the kernels return is the rounding residue of terms of
    size |p_j| |q_{j-1}| (measured: 2.4e-9 from terms of 1e10, and another
    residue from the one-strip kernel on another grid), so a bound relative
    to the residue itself asks nothing of either kernel.  The bound is
    relative to the sum's terms, through a scale that is no larger than
    theirs: |q_{j-1}| = sqrt(q.q) of the iteration before, and |p_j| >=
    sqrt(r.r), p_j = r + beta p_{j-1} with r orthogonal to p_{j-1}.
    Iteration 3 the same sums once more, now from scalars that may differ in
    the last bits: 1e-12, p.q_old on its scale again."""
    from gp_grief_amd.distributed import BlockHipEngine
    shift = 0.3
    F = factors(ms, 2)
    b = np.random.default_rng(5).standard_normal(int(np.prod(ms)))
    out = {}
    for mask in (0, 2):
        e = BlockHipEngine(operator(gg, monkeypatch, F, mask), 2, 1, shift)
        assert e.blk0 == 4 and e.nblk == 4 and e.rderive == rderive
        e.work.zero_()
        bl = e.fold(dev(gg, b))
        x = e.zeros()
        e.start_partial(bl, x)
        e.start_finish(0.0, 0.0)
        steps = []
        for _ in range(3):
            red = host(gg, e.iterate_partial()).copy()
            steps.append((red, host(gg, e.work).copy()))
            e.iterate_finish()
        out[mask] = steps
    (r1, w1), (r2, w2), (r3, _) = out[0]
    (s1, v1), (s2, v2), (s3, _) = out[2]
    print("iteration 2 red, mask 0:", r2.tolist(), "mask 2:", s2.tolist())
    print("iteration 3 red, mask 0:", r3.tolist(), "mask 2:", s3.tolist())
    assert np.array_equal(r1, s1) and np.array_equal(w1, v1)
    assert np.array_equal(w2, v2) and np.array_equal(r2[2:], s2[2:])
    assert r2[0] > 0.0
    assert abs(s2[0] - r2[0]) <= 1e-13 * abs(r2[0])
    assert abs(s2[1] - r2[1]) <= 1e-13 * np.sqrt(r2[0] * r1[4])
    for k in (0, 2, 3, 4):
        assert abs(s3[k] - r3[k]) <= 1e-12 * abs(r3[k])
    assert abs(s3[1] - r3[1]) <= 1e-12 * np.sqrt(r3[0] * r2[4])


def oracle_cg(F, b, shift, rtol, maxiter):
    return oracle.cg_solve(lambda v: oracle.kron_matvec(F, v) + shift * v, b, rtol=rtol,
                           maxiter=maxiter)


@pytest.mark.parametrize("rderive", ["1", "0"])
@pytest.mark.parametrize("ms,shift", [((40, 2, 72, 72), 0.2), ((40, 72, 72), 0.2)])
def test_cg_two_strips_vs_oracle(gg, monkeypatch, ms, shift, rderive):
    """Full solves with both bits on and the x window (the default, 8) against
    the oracle CG at test_gpu_block.py's tolerances: iterations within 2 %, x
    to 1e-8, the true residual at the tolerance; stored and derived r."""
    monkeypatch.setenv("GG_CG_RDERIVE", rderive)
    F = factors(ms, 9)
    n = int(np.prod(ms))
    b = np.random.default_rng(14).standard_normal((n, 1))
    K = operator(gg, monkeypatch, F, 3)
    s = gg.linalg.KronCG(K, shift)
    assert s.basis == "block" and s.rderive == (rderive == "1") and s.xwin == 8
    x, info = gg.linalg.cg(K, b, shift=shift, rtol=1e-10, maxiter=20000)
    it = gg.linalg.cg.last.iters
    xs, _, its = oracle_cg(F, b[:, 0], shift, 1e-10, 20000)
    assert info == 0
    assert abs(it - its) <= max(2, 0.02 * its), (it, its)
    assert rel(x, xs) < 1e-8
    r = oracle.kron_matvec(F, x[:, 0]) + shift * x[:, 0] - b[:, 0]
    assert np.linalg.norm(r) <= 1.5e-10 * np.linalg.norm(b)


def test_cg_two_strips_rderive_repairs(gg, monkeypatch):
    """Forced cancellations (GG_CG_CANCEL_TOL = 0.3), as
    test_block_cg_rderive_repairs: the repair materialises r from the
    directions the two-strip prologue wrote, and the solve lands on the
    oracle's x."""
    monkeypatch.setenv("GG_CG_CANCEL_TOL", "0.3")
    ms, shift = (40, 72, 72), 0.05
    F = factors(ms, 10)
    s = gg.linalg.KronCG(operator(gg, monkeypatch, F, 3), shift)
    assert s.rderive
    b = np.random.default_rng(15).standard_normal(int(np.prod(ms)))
    s.start(dev(gg, b), rtol=1e-10)
    s.iterate(20000, check_every=25)
    it, conv, res, tol = s.status()
    assert conv and s.cancels() > 0
    xs, _, its = oracle_cg(F, b, shift, 1e-10, 20000)
    assert rel(host(gg, s.x), xs) < 1e-8



def test_lanczos_plain_bit_bitwise(gg, monkeypatch):
    """The Lanczos step's prologue stays at one strip per wave (its two-strip
    form did not clear the measurement's margin and was removed); its plain
    launch on axis 1 follows bit 0 and carries no sums: alpha, beta are
    bitwise mask 0's, and the oracle's tridiagonal as
    test_block_lanczos_matches_grid_and_oracle."""
    ms, s = (40, 40, 40, 40), 0.03
    F = factors(ms, 6)
    n = int(np.prod(ms))
    out = {}
    for mask in (0, 3):
        K = operator(gg, monkeypatch, F, mask)
        assert gg.linalg.lanczos_info(K) == (True, 3)
        out[mask] = gg.linalg.lanczos_tridiag(K, s, 20, seed=7, probe=2)
    (a0, b0), (a3, b3) = out[0], out[3]
    assert np.array_equal(a0, a3) and np.array_equal(b0, b3)
    k = min(a3.size, 12)
    assert k == 12
    zp = oracle.cg.probe_signs(7, 2, n)
    ao, bo = oracle.lanczos_tridiag(lambda v: oracle.kron_matvec(F, v) + s * v, zp, 20)
    np.testing.assert_allclose(a3[:k], ao[:k], rtol=1e-8)
    np.testing.assert_allclose(b3[:k - 1], bo[:k - 1], rtol=1e-7)
