"""The Kronecker / CG / Lanczos section of include/gp_grief_amd.h at its edges,
called through ctypes exactly as a C caller would (gg_kron_*, the parity-block
basis, gg_cg_*, gg_lanczos_probe, the decoded diagonal).

Guarded buffers: every device operand is a payload of exactly the documented
size with 64 NaN doubles on either side; outputs and scratch are pre-filled
with NaN, so an overrun of one double lands in a guard and a read of
uninitialised scratch reaches the result.  Guards, and every input, are
compared bit for bit after each call; a refused call must leave everything
untouched.

Elementwise bound of the matvecs (derived in tests/kron_abi_ref.py, not
tuned; tests/test_kron_abi_ref.py shows float64 NumPy inside it):
    |got - ref| <= c u mag + 2 u |shift| |x|,   u = 2^-53,
c = sum_k (q_k + 3) + 2 over the stages (q_k = h_k in the block basis),
against a long-double reference.

Alignment of x, y and work in gg_kron_matvec: every load and store of the
mode-product kernels on these operands is a single double (the 16-byte forms --
the ring kernel, the staged folded epilogue -- are selected at run time only
when the pointers are 16-byte aligned), so each case also runs with all three
one double into their allocation.

Measured on MI355X (worst err / bound per case, printed by the tests): grid
matvec 0.0005 .. 0.165 (the folded 48 x 7 x 49 operators below 0.001, the
short chains highest), block matvec and its ranges 0.07 .. 0.10; the Lanczos
quadratures past the Krylov space within 5e-15 relative of the oracle's."""
import contextlib
import ctypes

import numpy as np
import pytest

import kron_abi_ref as R
import oracle
from oracle import cg as ocg
from oracle import kron as okron

from abi_guard import Guard, bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GG_OK, GG_ERR_VALUE = 0, -1


def rel(a, b):
    a = np.asarray(a, dtype=LD).reshape(-1)
    b = np.asarray(b, dtype=LD).reshape(-1)
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b ** 2)), LD(1e-300)))


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


def null_or(g):
    return g.ptr if g is not None else None


@contextlib.contextmanager
def kron(nat, factors):
    """A gg_kron handle made the way a C caller makes it."""
    fs = [np.ascontiguousarray(F, dtype=np.float64) for F in factors]
    d = len(fs)
    ptrs = (ctypes.c_void_p * d)(*[F.ctypes.data for F in fs])
    out = ctypes.c_void_p()
    nat.check(nat.lib().gg_kron_create(d, nat.i64_array([F.shape[0] for F in fs]),
                                       nat.i64_array([F.shape[1] for F in fs]), ptrs,
                                       ctypes.byref(out)), "gg_kron_create")
    try:
        yield out
    finally:
        import torch
        torch.cuda.synchronize()
        assert nat.lib().gg_kron_destroy(out) == GG_OK


def kron_shape(nat, K, tr):
    a, b, c = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    nat.check(nat.lib().gg_kron_shape(K, tr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def matvec(nat, K, tr, xg, yg, shift, wg):
    return nat.lib().gg_kron_matvec(K, tr, xg.ptr, yg.ptr, shift, null_or(wg), nat.stream_ptr())


# ============================================================ A. operator handle
@pytest.mark.parametrize("name", sorted(R.MATVEC_CASES))
def test_matvec_exact_scratch(nat, name):
    """Forward and transposed, shift 0 and (square) 0.37, work_dev of exactly
    gg_kron_shape's work_elems, operands 16-byte aligned and one double off:
    the elementwise bound, guards, x bitwise, a second call, the timed entry
    and a side stream bit for bit."""
    import torch
    L = nat.lib()
    fs, xf, xt = R.matvec_case(name)
    d = len(fs)
    square = xf.size == xt.size
    side = torch.cuda.Stream()
    with kron(nat, fs) as K:
        for tr in (0, 1):
            x = xt if tr else xf
            n_out, n_in, we = kron_shape(nat, K, tr)
            assert n_in == x.size and n_out == (xf.size if tr else xt.size) and we >= 0
            mask = ctypes.c_int64(-1)
            nat.check(L.gg_kron_fold_mask(K, tr, ctypes.byref(mask)))
            assert mask.value == R.MATVEC_MASKS.get(name, 0) == R.fold_mask(fs, bool(tr))
            for shift in (0.0, 0.37) if square else (0.0,):
                ref, mag = R.matvec_ref(fs, x, bool(tr), shift, mask.value)
                bound = R.matvec_bound(fs, x, mag, bool(tr), shift)
                for off in (0, 1):
                    xg, yg, wg = Guard(n_in, x, off), Guard(n_out, None, off), Guard(we, None, off)
                    nat.check(matvec(nat, K, tr, xg, yg, shift, wg), "gg_kron_matvec")
                    y = yg.read()
                    xg.unchanged()
                    wg.read()
                    r = R.worst_ratio(y, ref, bound)
                    print("kron matvec %s transpose=%d shift=%g off=%d c=%d: err/bound %.4f"
                          % (name, tr, shift, off, R.matvec_c(fs, bool(tr)), r))
                    assert r <= 1.0, (name, tr, shift, off, r)
                    # again, from NaN output and scratch: the same bits
                    yg.reset()
                    wg.reset()
                    nat.check(matvec(nat, K, tr, xg, yg, shift, wg), "gg_kron_matvec")
                    assert np.array_equal(bits(yg.read()), bits(y))
                    if off:
                        continue
                    # the timed entry: same bits, d positive times
                    yg.reset()
                    wg.reset()
                    ms, tot = (ctypes.c_double * d)(*([-1.0] * d)), ctypes.c_double(-1.0)
                    nat.check(L.gg_kron_matvec_timed(K, tr, xg.ptr, yg.ptr, shift, wg.ptr, 2, ms,
                                                     ctypes.byref(tot), nat.stream_ptr()),
                              "gg_kron_matvec_timed")
                    assert np.array_equal(bits(yg.read()), bits(y))
                    assert all(ms[k] > 0.0 for k in range(d)) and tot.value > 0.0, list(ms)
                    wg.read()
                    # a side stream: same bits
                    yg.reset()
                    wg.reset()
                    with torch.cuda.stream(side):
                        assert nat.stream_ptr().value == side.cuda_stream
                        nat.check(matvec(nat, K, tr, xg, yg, shift, wg), "gg_kron_matvec")
                    side.synchronize()
                    assert np.array_equal(bits(yg.read()), bits(y))
                    xg.unchanged()
                    wg.read()


def test_two_handles_and_destroy_null(nat):
    """Two live handles used alternately do not disturb each other."""
    L = nat.lib()
    assert L.gg_kron_destroy(None) == GG_OK
    f1, x1, _ = R.matvec_case("mixed3")
    f2, x2, _ = R.matvec_case("centro_48_7_49")
    with kron(nat, f1) as K1, kron(nat, f2) as K2:
        outs = []
        for rnd in range(2):
            for K, fs, x in ((K1, f1, x1), (K2, f2, x2)):
                n_out, n_in, we = kron_shape(nat, K, 0)
                xg, yg, wg = Guard(n_in, x), Guard(n_out), Guard(we)
                nat.check(matvec(nat, K, 0, xg, yg, 0.0, wg))
                outs.append(yg.read())
                wg.read()
        assert np.array_equal(bits(outs[0]), bits(outs[2]))
        assert np.array_equal(bits(outs[1]), bits(outs[3]))
        for y, fs, x, name in ((outs[0], f1, x1, "mixed3"), (outs[1], f2, x2, "centro_48_7_49")):
            ref, mag = R.matvec_ref(fs, x, False, 0.0, R.MATVEC_MASKS.get(name, 0))
            assert R.worst_ratio(y, ref, R.matvec_bound(fs, x, mag)) <= 1.0


def test_matvec_refusals(nat):
    """GG_ERR_VALUE before any launch: nothing is written."""
    L = nat.lib()
    fs = R.toeplitz_factors((8, 6))
    n = 48
    x = R.vector(n, 3)
    with kron(nat, fs) as K:
        _, _, we = kron_shape(nat, K, 0)
        xg, yg, wg = Guard(n, x), Guard(n), Guard(we)
        assert L.gg_kron_matvec(K, 0, xg.ptr, xg.ptr, 0.0, wg.ptr, nat.stream_ptr()) == GG_ERR_VALUE
        assert matvec(nat, K, 0, xg, yg, 0.0, None) == GG_ERR_VALUE      # d = 2: work required
        assert L.gg_kron_matvec(K, 0, None, yg.ptr, 0.0, wg.ptr, nat.stream_ptr()) == GG_ERR_VALUE
        assert L.gg_kron_matvec(None, 0, xg.ptr, yg.ptr, 0.0, wg.ptr,
                                nat.stream_ptr()) == GG_ERR_VALUE
        ms, tot = (ctypes.c_double * 2)(-1.0, -1.0), ctypes.c_double(-1.0)
        assert L.gg_kron_matvec_timed(K, 0, xg.ptr, yg.ptr, 0.0, wg.ptr, 0, ms, ctypes.byref(tot),
                                      nat.stream_ptr()) == GG_ERR_VALUE
        assert list(ms) == [-1.0, -1.0] and tot.value == -1.0
        for g in (xg, yg, wg):
            g.unchanged()
    gf, gx, _ = R.matvec_case("growing")
    with kron(nat, gf) as K:
        n_out, n_in, we = kron_shape(nat, K, 0)
        assert n_out != n_in
        xg, yg, wg = Guard(n_in, gx), Guard(n_out), Guard(we)
        assert matvec(nat, K, 0, xg, yg, 0.37, wg) == GG_ERR_VALUE     # shift, non-square
        for g in (xg, yg, wg):
            g.unchanged()
    # d = 1: no scratch, NULL work_dev is accepted
    f1, x1, _ = R.matvec_case("5x3")
    with kron(nat, f1) as K:
        xg, yg = Guard(3, x1), Guard(5)
        nat.check(matvec(nat, K, 0, xg, yg, 0.0, None), "gg_kron_matvec, d = 1, NULL work")
        ref, mag = R.matvec_ref(f1, x1)
        assert R.worst_ratio(yg.read(), ref, R.matvec_bound(f1, x1, mag)) <= 1.0
        xg.unchanged()


def test_create_refusals(nat):
    """gg_kron_create: bad shapes and every NULL pointer are GG_ERR_VALUE (the
    checks stand before the first dereference) and *out stays as it was."""
    L = nat.lib()
    F = np.ascontiguousarray(np.eye(3))
    one = (ctypes.c_void_p * 1)(F.ctypes.data)
    two = (ctypes.c_void_p * 2)(F.ctypes.data, None)
    i64 = nat.i64_array
    SENT = 0x5A5A5A5A

    def refused(d, rows, cols, ptrs, with_out=True):
        out = ctypes.c_void_p(SENT)
        st = L.gg_kron_create(d, rows, cols, ptrs, ctypes.byref(out) if with_out else None)
        assert st == GG_ERR_VALUE and out.value == SENT, (st, out.value)

    refused(0, i64([3]), i64([3]), one)                       # d = 0
    refused(-1, i64([3]), i64([3]), one)
    refused(1, i64([0]), i64([3]), one)                       # a 0-row factor
    refused(1, i64([3]), i64([0]), one)
    refused(1, i64([(1 << 20) + 1]), i64([1]), one)           # above 2^20 (never read)
    refused(1, i64([1]), i64([(1 << 20) + 1]), one)
    refused(1, i64([3]), i64([3]), one, with_out=False)       # NULL out
    refused(1, None, i64([3]), one)                           # NULL rows
    refused(1, i64([3]), None, one)                           # NULL cols
    refused(1, i64([3]), i64([3]), None)                      # NULL factors_host
    refused(2, i64([3, 3]), i64([3, 3]), two)                 # NULL factors_host[1]
    assert "NULL" in nat.last_error()
    # and the same arguments, complete, are accepted
    out = ctypes.c_void_p()
    nat.check(L.gg_kron_create(1, i64([3]), i64([3]), one, ctypes.byref(out)))
    assert L.gg_kron_destroy(out) == GG_OK


# ========================================================= B. parity-block basis
def block_info(nat, K):
    av, n, la = ctypes.c_int(-1), ctypes.c_int64(-1), ctypes.c_int(-1)
    nat.check(nat.lib().gg_kron_block_info(K, ctypes.byref(av), ctypes.byref(n), ctypes.byref(la)))
    return av.value, n.value, la.value


def block_problem(ms):
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    x = R.vector(n, 11)
    xb = okron.block_fold(x, ms, pad=True)
    return fs, n, x, xb


@pytest.mark.parametrize("ms", R.BLOCK_OPS, ids=lambda m: "x".join(map(str, m)))
def test_block_fold_and_matvec(nat, ms):
    """Fold / unfold 1e-15 normwise against oracle.kron.block_fold, the block
    matvec inside the elementwise bound (shift 0 and 0.05) with scratch of
    exactly the block layout's n; zero padding is zero after the fold and
    stays zero after the matvec."""
    L = nat.lib()
    fs, n, x, xb = block_problem(ms)
    d = len(ms)
    padm = R.block_pad_mask(ms)
    with kron(nat, fs) as K:
        av, N, la = block_info(nat, K)
        assert (av, N, la) == (1, xb.size, d - 1)
        assert (N > n) == (ms == (4, 64, 64))
        xg, bg = Guard(n, x), Guard(N)
        nat.check(L.gg_kron_block_fold(K, 0, xg.ptr, bg.ptr, nat.stream_ptr()))
        got = bg.read()
        xg.unchanged()
        assert rel(got, xb) < 1e-15
        assert np.all(bits(got[padm]) == 0), "padding must be +0.0 after the fold"
        ig, og = Guard(N, xb), Guard(n)
        nat.check(L.gg_kron_block_fold(K, 1, ig.ptr, og.ptr, nat.stream_ptr()))
        assert rel(og.read(), x) < 1e-15
        ig.unchanged()
        for shift in (0.0, 0.05):
            ref, mag = R.block_matvec_ref(fs, xb, shift)
            ig, yg = Guard(N, xb), Guard(N)
            wg = Guard(N) if d >= 3 else None
            nat.check(L.gg_kron_block_matvec(K, ig.ptr, yg.ptr, shift, null_or(wg),
                                             nat.stream_ptr()), "gg_kron_block_matvec")
            y = yg.read()
            ig.unchanged()
            if wg is not None:
                wg.read()
            r = R.worst_ratio(y, ref, R.block_bound(fs, xb, mag, shift))
            print("block matvec %s shift=%g c=%d: err/bound %.4f" % (ms, shift, R.block_c(fs), r))
            assert r <= 1.0, (ms, shift, r)
            assert np.all(y[padm] == 0), "padding must stay zero after the matvec"


@pytest.mark.parametrize("ms", R.BLOCK_OPS, ids=lambda m: "x".join(map(str, m)))
def test_block_ranges(nat, ms):
    """Every halving of the 2^d blocks down to single blocks, and one ragged
    range: the forward fold and the range matvec write exactly nblk n / 2^d
    doubles; the inverse folds of a partition sum to the full unfold."""
    L = nat.lib()
    fs, n, x, xb = block_problem(ms)
    d = len(ms)
    nblocks = 1 << d
    with kron(nat, fs) as K:
        N = block_info(nat, K)[1]
        nb = N // nblocks
        xg = Guard(n, x)
        ranges, nblk = [], nblocks
        while nblk >= 1:
            ranges += [(b0, nblk, True) for b0 in range(0, nblocks, nblk)]
            nblk //= 2
        ranges.append((1, 3, False))      # ragged: part of no partition below
        worst = 0.0
        sums = {}
        for blk0, nblk, in_partition in ranges:
            seg = slice(blk0 * nb, (blk0 + nblk) * nb)
            fg = Guard(nblk * nb)
            nat.check(L.gg_kron_block_fold_range(K, 0, xg.ptr, fg.ptr, blk0, nblk,
                                                 nat.stream_ptr()), "fold_range")
            assert rel(fg.read(), xb[seg]) < 1e-15, (blk0, nblk)
            for shift in (0.0, 0.05):
                ref, mag = R.block_matvec_ref(fs, xb[seg], shift, True, blk0, nblk)
                ig, yg = Guard(nblk * nb, xb[seg]), Guard(nblk * nb)
                wg = Guard(nblk * nb) if d >= 3 else None
                nat.check(L.gg_kron_block_matvec_range(K, ig.ptr, yg.ptr, shift, null_or(wg), blk0,
                                                       nblk, nat.stream_ptr()), "matvec_range")
                r = R.worst_ratio(yg.read(), ref, R.block_bound(fs, xb[seg], mag, shift))
                assert r <= 1.0, (ms, blk0, nblk, shift, r)
                worst = max(worst, r)
                ig.unchanged()
                if wg is not None:
                    wg.read()
            # this range's share of P^T x_b, into every grid element
            ig, og = Guard(nblk * nb, xb[seg]), Guard(n)
            nat.check(L.gg_kron_block_fold_range(K, 1, ig.ptr, og.ptr, blk0, nblk,
                                                 nat.stream_ptr()), "inverse fold_range")
            part = og.read().astype(LD)
            assert np.all(np.isfinite(part))
            if in_partition:
                sums[nblk] = sums.get(nblk, 0) + part
        xg.unchanged()
        print("block range matvec %s: worst err/bound %.4f over %d ranges"
              % (ms, worst, len(ranges)))
        assert sorted(sums) == [1 << k for k in range(d + 1)]
        for nblk, total in sums.items():
            assert rel(total, x) < 1e-15, (ms, nblk)


def test_block_refusals(nat):
    L = nat.lib()
    ms = (4, 40, 40)
    fs, n, x, xb = block_problem(ms)
    with kron(nat, fs) as K:
        N = block_info(nat, K)[1]
        nb = N // 8
        xg, bg, yg, wg = Guard(n, x), Guard(N, xb), Guard(N), Guard(N)
        s = nat.stream_ptr()
        for blk0, nblk in ((-1, 2), (7, 2), (0, 9), (0, 0), (8, 1)):
            assert L.gg_kron_block_fold_range(K, 0, xg.ptr, yg.ptr, blk0, nblk, s) == GG_ERR_VALUE
            assert L.gg_kron_block_fold_range(K, 1, bg.ptr, yg.ptr, blk0, nblk, s) == GG_ERR_VALUE
            assert L.gg_kron_block_matvec_range(K, bg.ptr, yg.ptr, 0.0, wg.ptr, blk0, nblk,
                                                s) == GG_ERR_VALUE
        assert L.gg_kron_block_fold(K, 0, bg.ptr, bg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_block_fold(K, 1, bg.ptr, bg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_block_fold_range(K, 0, bg.ptr, bg.ptr, 0, 1, s) == GG_ERR_VALUE
        assert L.gg_kron_block_matvec(K, bg.ptr, bg.ptr, 0.0, wg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_block_matvec(K, bg.ptr, yg.ptr, 0.0, None, s) == GG_ERR_VALUE   # d = 3
        for g in (xg, bg, yg, wg):
            g.unchanged()
        assert nb * 8 == N
    # an operator without the basis (an odd order)
    ms = (9, 40, 40)
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    with kron(nat, fs) as K:
        assert block_info(nat, K) == (0, 0, 0)
        xg, yg = Guard(n, R.vector(n, 5)), Guard(n)
        s = nat.stream_ptr()
        assert L.gg_kron_block_fold(K, 0, xg.ptr, yg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_block_fold_range(K, 0, xg.ptr, yg.ptr, 0, 1, s) == GG_ERR_VALUE
        assert L.gg_kron_block_matvec(K, xg.ptr, yg.ptr, 0.0, yg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_block_matvec_range(K, xg.ptr, yg.ptr, 0.0, yg.ptr, 0, 1,
                                            s) == GG_ERR_VALUE
        xg.unchanged()
        yg.unchanged()


# ================================================================= C. CG handle
_schur = {}


def schur_solve(ms, b, shift):
    key = tuple(ms)
    if key not in _schur:
        Q, lam = oracle.factor_eigh(R.toeplitz_factors(ms))
        _schur[key] = (Q, oracle.kron_expand(lam))
    Q, t = _schur[key]
    return oracle.solve_schur(Q, t, b, shift)


class Cg(object):
    """gg_cg_* on a guarded workspace of exactly gg_cg_work_elems doubles
    (sized now: after the caller's environment is set)."""

    def __init__(self, nat, K, shift, off=0):
        self.nat, self.L = nat, nat.lib()
        we = ctypes.c_int64(-1)
        nat.check(self.L.gg_cg_work_elems(K, ctypes.byref(we)), "gg_cg_work_elems")
        self.wg = Guard(we.value, None, off)
        self.h = ctypes.c_void_p()
        nat.check(self.L.gg_cg_create(K, shift, self.wg.ptr, ctypes.byref(self.h)), "gg_cg_create")

    def get(self, what):
        v = ctypes.c_int(-99)
        self.nat.check(getattr(self.L, "gg_cg_get_" + what)(self.h, ctypes.byref(v)))
        return v.value

    def start(self, bg, xg, rtol, atol=0.0):
        return self.L.gg_cg_start(self.h, bg.ptr, xg.ptr, rtol, atol, self.nat.stream_ptr())

    def iterate(self, max_iters, check_every):
        return self.L.gg_cg_iterate(self.h, max_iters, check_every, self.nat.stream_ptr())

    def status(self):
        it, cv = ctypes.c_int(-1), ctypes.c_int(-1)
        rn, tol = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        self.nat.check(self.L.gg_cg_status(self.h, ctypes.byref(it), ctypes.byref(cv),
                                           ctypes.byref(rn), ctypes.byref(tol),
                                           self.nat.stream_ptr()))
        return it.value, cv.value, rn.value, tol.value

    def close(self):
        import torch
        torch.cuda.synchronize()
        assert self.L.gg_cg_destroy(self.h) == GG_OK
        self.wg.read()


CG_SHIFT = 0.5
_WIN_ENVS = [{"GG_CG_XWIN": w, "GG_CG_RDERIVE": r} for w in "028" for r in "01"]
# (8, 6): d = 2, grid basis; (7, 5, 3): odd n, textbook; (6, 4, 2): odd d, the
# first-step scratch; (4, 40, 40): block basis (pair order 40: the register
# pair kernel, so GG_CG_XWIN is inert there); (4, 64, 64): the padded layout
# (block length > n) through gg_cg_set_basis(1), where the window runs;
# (40, 72, 72): unpadded with the LDS pair kernel and a first axis of half
# order 20 -- the window and the derived r both in effect
CG_ENVS = {
    (8, 6): [{}],
    (7, 5, 3): [{}],
    (6, 4, 2): [{}, {"GG_CG_VEC_PAD": "2"}],
    (4, 40, 40): _WIN_ENVS + [{"GG_CG_VEC_PAD": "2"}],
    (4, 64, 64): [{"GG_CG_XWIN": "0"}, {"GG_CG_XWIN": "2"},
                  {"GG_CG_XWIN": "8", "GG_CG_VEC_PAD": "2"}],
    (40, 72, 72): _WIN_ENVS + [{"GG_CG_VEC_PAD": "2"}],
}


def window_expected(ms, env):
    """(xwin, rderive) gg_cg_start picks in the block basis: the window where
    the LDS pair kernel carries the side job (pair extent 16 TF + 4, TF >= 2),
    the derived r with it where the first axis has half order 16 j + 4 >= 20."""
    if len(ms) < 3 or okron.block_pad(ms[-1] // 2) < 36:
        return 0, 0
    w = int(env.get("GG_CG_XWIN", "8"))
    w = 0 if w < 2 else w
    h0 = ms[0] // 2
    rd = int(w >= 2 and env.get("GG_CG_RDERIVE", "1") != "0" and h0 >= 20 and h0 % 16 == 4)
    return w, rd


@pytest.mark.parametrize("ms", sorted(CG_ENVS), ids=lambda m: "x".join(map(str, m)))
def test_cg_exact_workspace(nat, monkeypatch, ms):
    """Solve to rtol 1e-12 on a NaN-filled workspace of exactly
    gg_cg_work_elems doubles, its base 16-byte aligned and 8-byte aligned only
    (textbook recurrence there): x within 1e-9 of oracle.solve_schur, guards
    intact, b unchanged."""
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    b = R.vector(n, 23)
    want = schur_solve(ms, b, CG_SHIFT)
    for env in CG_ENVS[ms]:
        for k in ("GG_CG_XWIN", "GG_CG_RDERIVE", "GG_CG_VEC_PAD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with kron(nat, fs) as K:
            has_block = block_info(nat, K)[0] == 1
            for off in (0, 1):
                cg = Cg(nat, K, CG_SHIFT, off)
                if ms == (4, 64, 64):
                    assert cg.L.gg_cg_set_basis(cg.h, 1) == GG_OK
                fused = cg.get("recurrence")
                if off == 1 or n % 2 == 1 or len(ms) < 2:
                    assert fused == 0, "an 8-byte aligned base / odd n runs the textbook recurrence"
                else:
                    assert fused == 1
                block = int(bool(fused and has_block and len(ms) >= 3))
                win = window_expected(ms, env) if block else (0, 0)
                assert cg.get("basis") == block
                assert (cg.get("xwin"), cg.get("rderive")) == win
                bg, xg = Guard(n, b), Guard(n)
                assert cg.start(bg, xg, 1e-12) == GG_OK
                assert cg.get("basis") == block
                assert (cg.get("xwin"), cg.get("rderive")) == win
                assert cg.iterate(20 * n, 1) == GG_OK
                it, conv, rn, tol = cg.status()
                x = xg.read()
                bg.unchanged()
                e = rel(x, want)
                print("cg %s env=%s off=%d fused=%d: %d iters, rel err %.2e" % (ms, env, off, fused,
                                                                                 it, e))
                assert conv == 1 and 0 < it < 20 * n and rn < tol
                assert e < 1e-9, (ms, env, off, e)
                cg.close()


def test_cg_state_machine(nat):
    """The rules the header documents for the handle."""
    ms = (8, 6)
    fs = R.toeplitz_factors(ms)
    n = 48
    b = R.vector(n, 29)
    with kron(nat, fs) as K:
        cg = Cg(nat, K, CG_SHIFT)
        L, s = cg.L, nat.stream_ptr()
        bg, xg = Guard(n, b), Guard(n)
        # before start
        assert cg.iterate(5, 1) == GG_ERR_VALUE
        assert L.gg_cg_iterate_open(cg.h, 5, 1, s) == GG_ERR_VALUE
        assert L.gg_cg_close(cg.h, s) == GG_ERR_VALUE
        # out-of-range values
        before = [cg.get(w) for w in ("fusion", "xdefer", "rq", "basis", "recurrence")]
        assert L.gg_cg_set_fusion(cg.h, 3) == GG_ERR_VALUE
        assert L.gg_cg_set_fusion(cg.h, -1) == GG_ERR_VALUE
        assert L.gg_cg_set_xdefer(cg.h, 3) == GG_ERR_VALUE
        assert L.gg_cg_set_rq(cg.h, 2) == GG_ERR_VALUE
        assert L.gg_cg_set_basis(cg.h, 1) == GG_ERR_VALUE      # (8, 6) has no block basis
        assert [cg.get(w) for w in ("fusion", "xdefer", "rq", "basis", "recurrence")] == before
        # bad tolerances and pointers: refused, x untouched, still not started
        for rtol, atol in ((-1e-3, 0.0), (float("nan"), 0.0), (1e-6, float("nan")), (1e-6, -1.0)):
            assert cg.start(bg, xg, rtol, atol) == GG_ERR_VALUE
        assert L.gg_cg_start(cg.h, None, xg.ptr, 1e-6, 0.0, s) == GG_ERR_VALUE
        assert L.gg_cg_start(cg.h, bg.ptr, None, 1e-6, 0.0, s) == GG_ERR_VALUE
        # x one double off a 16-byte boundary (the update kernels move pairs)
        assert L.gg_cg_start(cg.h, bg.ptr, ctypes.c_void_p(xg.ptr.value + 8), 1e-6, 0.0,
                             s) == GG_ERR_VALUE
        xg.unchanged()
        assert cg.iterate(5, 1) == GG_ERR_VALUE
        # a legal setting before start sticks
        assert L.gg_cg_set_rq(cg.h, 0) == GG_OK and cg.get("rq") == 0
        assert L.gg_cg_set_rq(cg.h, 1) == GG_OK and cg.get("rq") == 1
        # start; tol = max(atol, rtol |b|), relative regime
        assert cg.start(bg, xg, 1e-6, 0.0) == GG_OK
        it, conv, rn, tol = cg.status()
        bn = float(np.sqrt(np.sum(b.astype(LD) ** 2)))
        assert (it, conv) == (0, 0)
        assert abs(tol - 1e-6 * bn) <= 1e-6 * bn * (n + 8) * U and abs(rn - bn) <= bn * (n + 8) * U
        # every setter is refused once started, the getters keep their values
        before = [cg.get(w) for w in ("fusion", "xdefer", "rq", "basis", "recurrence")]
        assert L.gg_cg_set_recurrence(cg.h, 0) == GG_ERR_VALUE
        assert L.gg_cg_set_recurrence(cg.h, 1) == GG_ERR_VALUE
        assert L.gg_cg_set_fusion(cg.h, 1) == GG_ERR_VALUE
        assert L.gg_cg_set_xdefer(cg.h, 0) == GG_ERR_VALUE
        assert L.gg_cg_set_rq(cg.h, 0) == GG_ERR_VALUE
        assert L.gg_cg_set_basis(cg.h, 0) == GG_ERR_VALUE
        assert [cg.get(w) for w in ("fusion", "xdefer", "rq", "basis", "recurrence")] == before
        # max_iters = 0: GG_OK, nothing moves
        assert cg.iterate(0, 1) == GG_OK and cg.iterate(0, 0) == GG_OK
        assert cg.status()[0] == 0
        assert np.all(bits(xg.read()) == 0)
        # the profile's length check
        la = ctypes.c_int(-1)
        nat.check(L.gg_cg_launches(cg.h, ctypes.byref(la)))
        assert la.value == 2
        nm, one = ctypes.c_int(-5), (ctypes.c_double * 1)(-1.0)
        assert L.gg_cg_profile_read(cg.h, ctypes.byref(nm), one, 1) == GG_ERR_VALUE
        assert nm.value == -5 and one[0] == -1.0
        assert L.gg_cg_profile_read(cg.h, None, one, 2) == GG_ERR_VALUE
        # the absolute regime: tol = atol exactly
        assert cg.start(bg, xg, 1e-6, 10.0) == GG_OK
        it, conv, rn, tol = cg.status()
        assert tol == 10.0 and it == 0
        assert cg.iterate(50, 1) == GG_OK
        it, conv, rn, tol = cg.status()
        assert (it, conv) == (0, 1) and np.all(bits(xg.read()) == 0)    # |b| < atol already
        # b = 0: converged, 0 iterations, x exactly 0
        zg = Guard(n, np.zeros(n))
        assert cg.start(zg, xg, 1e-10, 0.0) == GG_OK
        assert cg.iterate(50, 1) == GG_OK
        it, conv, rn, tol = cg.status()
        assert (it, conv, rn) == (0, 1, 0.0)
        assert np.all(bits(xg.read()) == 0)
        zg.unchanged()
        bg.unchanged()
        cg.close()


@pytest.mark.parametrize("ms", [(8, 6), (6, 4, 2), (4, 40, 40), (40, 72, 72)],
                         ids=lambda m: "x".join(map(str, m)))
def test_cg_done_flag_and_restart(nat, monkeypatch, ms):
    """check_every = 0 with max_iters far above need: the same iteration count
    and the same x, bit for bit, as polling every iteration (the device's done
    flag stops the recurrence exactly); a second gg_cg_start on a used handle
    with another b gives the bits of a fresh handle."""
    for k in ("GG_CG_XWIN", "GG_CG_RDERIVE", "GG_CG_VEC_PAD"):
        monkeypatch.delenv(k, raising=False)
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    b1, b2 = R.vector(n, 31), R.vector(n, 37)
    with kron(nat, fs) as K:
        def solve(cg, b, check_every, max_iters):
            bg, xg = Guard(n, b), Guard(n)
            assert cg.start(bg, xg, 1e-10) == GG_OK
            assert cg.iterate(max_iters, check_every) == GG_OK
            it, conv = cg.status()[:2]
            assert conv == 1
            bg.unchanged()
            return it, xg.read()

        cg = Cg(nat, K, CG_SHIFT)
        it1, x1 = solve(cg, b1, 1, 10 * n)
        cg.close()
        cg = Cg(nat, K, CG_SHIFT)
        it0, x0 = solve(cg, b1, 0, 10 * it1 + 7)
        assert it0 == it1 and np.array_equal(bits(x0), bits(x1))
        # the used handle, restarted with another b ...
        itr, xr = solve(cg, b2, 1, 10 * n)
        cg.close()
        # ... against a fresh one
        cg = Cg(nat, K, CG_SHIFT)
        itf, xf = solve(cg, b2, 1, 10 * n)
        cg.close()
        assert itr == itf and np.array_equal(bits(xr), bits(xf))
        assert rel(xf, schur_solve(ms, b2, CG_SHIFT)) < 1e-8


# ================================================================== D. Lanczos
SENT = -12345.0


def lanczos(nat, K, n, shift, steps, seed=0, probe=0, off=0):
    """(alphas, betas, steps_done) in full (steps entries each) on a guarded,
    NaN-filled workspace of exactly 4 n doubles."""
    wg = Guard(4 * n, None, off)
    a = (ctypes.c_double * steps)(*([SENT] * steps))
    b = (ctypes.c_double * steps)(*([SENT] * steps))
    done = ctypes.c_int(-7)
    nat.check(nat.lib().gg_lanczos_probe(K, shift, seed, probe, steps, wg.ptr, a, b,
                                         ctypes.byref(done), nat.stream_ptr()),
              "gg_lanczos_probe")
    wg.read()
    return np.array(a[:]), np.array(b[:]), done.value


def quadrature(a, b, k, n):
    """n sum_j U[0][j]^2 log theta_j of the leading k x k tridiagonal."""
    T = np.diag(a[:k]) + np.diag(b[:k - 1], 1) + np.diag(b[:k - 1], -1)
    theta, Uv = np.linalg.eigh(T)
    assert np.all(theta > 0), theta
    return float(n) * float(np.sum(Uv[0, :] ** 2 * np.log(theta)))


def test_lanczos_exact_breakdown(nat):
    """Identity factors (4, 4, 4), shift 0.5: A = 1.5 I and every quantity is
    exact in binary.  w_0 = 0: one step done, alpha_0 = 1.5, and the steps
    past the breakdown leave finite numbers."""
    fs = [np.eye(4)] * 3
    with kron(nat, fs) as K:
        a, b, done = lanczos(nat, K, 64, 0.5, 5)
        assert done == 1
        assert a[0] == 1.5 and b[0] == 0.0
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (a, b)


RANK1_CASES = [((6, 5, 4), (2.0, 2.0, 2.0)), ((3, 2, 2), (2.0, 2.0, 2.0)),
               ((6, 5, 4), (2.0, 1.0, 0.5)), ((3, 2, 2), (2.0, 1.0, 0.5))]


def rank1_factors(ms, cs):
    """I + c v v^T with unit v: eigenvalues 1 (m - 1 times) and 1 + c, so the
    operator has 2^d distinct eigenvalues at most (4 with every c = 2, 8 with
    distinct c) and the Krylov space of any probe is exhausted after as many
    steps."""
    rng = np.random.default_rng(41 + sum(ms))
    out = []
    for m, c in zip(ms, cs):
        v = rng.standard_normal(m)
        v /= np.linalg.norm(v)
        F = np.eye(m) + c * np.outer(v, v)
        out.append(0.5 * (F + F.T))
    return out


@pytest.mark.parametrize("ms,cs", RANK1_CASES,
                         ids=["x".join(map(str, m)) + "_c" + "_".join("%g" % c for c in cs)
                              for m, cs in RANK1_CASES])
def test_lanczos_near_breakdown_and_steps_above_n(nat, ms, cs):
    """Steps 8, 20, 40 on operators with at most 8 distinct eigenvalues (n = 120
    and n = 12: steps beyond the Krylov space and beyond n).  beta falls to
    rounding level at the exhaustion, never to 0, so every step runs; the
    per-probe quadrature n sum U[0]^2 log theta from the device tridiagonal is
    finite with every theta > 0 and equals the oracle's for the same probe and
    steps to 1e-9 relative."""
    fs = rank1_factors(ms, cs)
    n = int(np.prod(ms))
    shift = 0.3
    z = ocg.probe_signs(0, 0, n)

    def mv(v):
        return oracle.kron_matvec(fs, v) + shift * v

    with kron(nat, fs) as K:
        vals = []
        for steps in (8, 20, 40):
            a, b, done = lanczos(nat, K, n, shift, steps)
            assert 1 <= done <= steps
            assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), (steps, a, b)
            got = quadrature(a, b, done, n)
            oa, ob = ocg.lanczos_tridiag(mv, z, steps)
            want = ocg.quadrature_logdet(oa, ob, float(n))
            assert np.isfinite(got) and np.isfinite(want)
            print("lanczos %s c=%s steps=%d: done %d, min beta %.2e, device %.15g oracle %.15g "
                  "rel diff %.2e" % (ms, cs, steps, done, float(np.min(b[:done])), got, want,
                                     abs(got - want) / abs(want)))
            assert abs(got - want) <= 1e-9 * abs(want), (steps, got, want)
            vals.append(got)
        assert abs(vals[0] - vals[2]) <= 1e-9 * abs(vals[0])


@pytest.mark.parametrize("ms", [(8, 6), (6, 4, 2)], ids=lambda m: "x".join(map(str, m)))
def test_lanczos_one_step(nat, ms):
    """steps = 1: alpha_0 = v.A v and beta_0 = |A v - alpha_0 v| against the
    long-double reference.  With w computed to c u mag + 2 u |shift| |v| per
    element (the matvec's bound) and |v| = 1, alpha moves by at most the
    2-norm of that plus the reduction's roundings (tol); beta by that again
    plus alpha's own error (w = Y - alpha v): 2 tol."""
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    shift = 0.3
    v = ocg.probe_signs(3, 2, n) / np.sqrt(float(n))
    ref, mag = R.matvec_ref(fs, v, False, shift)
    vl = v.astype(LD)
    alpha = np.sum(vl * ref)
    beta = np.sqrt(np.sum((ref - alpha * vl) ** 2))
    eb = R.matvec_bound(fs, v, mag, False, shift)
    tol = float(np.sqrt(np.sum(eb ** 2))) + (n + 8) * U * float(np.sqrt(np.sum(ref ** 2)) + abs(alpha))
    with kron(nat, fs) as K:
        for off in (0, 1):
            a, b, done = lanczos(nat, K, n, shift, 1, seed=3, probe=2, off=off)
            assert done == 1
            print("lanczos %s one step off=%d: |alpha - ref| %.2e |beta - ref| %.2e (tol %.2e)"
                  % (ms, off, abs(a[0] - float(alpha)), abs(b[0] - float(beta)), tol))
            assert abs(a[0] - float(alpha)) <= tol and abs(b[0] - float(beta)) <= 2 * tol


def test_lanczos_block_and_grid_bases_agree(nat, monkeypatch):
    """(4, 40, 40) has an unpadded block basis with d >= 3: the tridiagonals
    of GG_LZ_BASIS=0 and 1 agree to 1e-8 on the first 8 steps, and
    gg_lanczos_info reports the basis and its launches."""
    ms = (4, 40, 40)
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    out = {}
    for basis in ("0", "1"):
        monkeypatch.setenv("GG_LZ_BASIS", basis)
        with kron(nat, fs) as K:
            blk, la = ctypes.c_int(-1), ctypes.c_int(-1)
            nat.check(nat.lib().gg_lanczos_info(K, ctypes.byref(blk), ctypes.byref(la)))
            assert (blk.value, la.value) == ((1, 2) if basis == "1" else (0, 3))
            out[basis] = lanczos(nat, K, n, 0.3, 8)
    monkeypatch.delenv("GG_LZ_BASIS")
    (a0, b0, d0), (a1, b1, d1) = out["0"], out["1"]
    assert d0 == d1 == 8
    scale = float(np.max(np.abs(a0)))
    assert np.max(np.abs(a0 - a1)) <= 1e-8 * scale and np.max(np.abs(b0 - b1)) <= 1e-8 * scale
    # and both are the oracle's
    z = ocg.probe_signs(0, 0, n)
    oa, ob = ocg.lanczos_tridiag(lambda v: oracle.kron_matvec(fs, v) + 0.3 * v, z, 8)
    assert np.max(np.abs(a0 - oa)) <= 1e-8 * scale and np.max(np.abs(b0[:7] - ob)) <= 1e-8 * scale
    with kron(nat, fs) as K:       # the default: the block basis where it is unpadded
        blk, la = ctypes.c_int(-1), ctypes.c_int(-1)
        nat.check(nat.lib().gg_lanczos_info(K, ctypes.byref(blk), ctypes.byref(la)))
        assert (blk.value, la.value) == (1, 2)


def test_lanczos_refusals(nat):
    """steps = 0, a non-square operator and NULL arrays: GG_ERR_VALUE, the
    host arrays and the workspace untouched."""
    L = nat.lib()
    fs = R.toeplitz_factors((8, 6))
    n = 48

    def call(K, steps, wg, a, b):
        done = ctypes.c_int(-7)
        st = L.gg_lanczos_probe(K, 0.3, 0, 0, steps, null_or(wg), a, b, ctypes.byref(done),
                                nat.stream_ptr())
        assert done.value == -7
        return st

    with kron(nat, fs) as K:
        wg = Guard(4 * n)
        a = (ctypes.c_double * 4)(*([SENT] * 4))
        b = (ctypes.c_double * 4)(*([SENT] * 4))
        assert call(K, 0, wg, a, b) == GG_ERR_VALUE
        assert call(K, -3, wg, a, b) == GG_ERR_VALUE
        assert call(K, 4, wg, None, b) == GG_ERR_VALUE
        assert call(K, 4, wg, a, None) == GG_ERR_VALUE
        assert call(K, 4, None, a, b) == GG_ERR_VALUE
        assert call(None, 4, wg, a, b) == GG_ERR_VALUE
        assert list(a) == [SENT] * 4 and list(b) == [SENT] * 4
        wg.unchanged()
        blk = ctypes.c_int(-1)
        assert L.gg_lanczos_info(K, ctypes.byref(blk), None) == GG_ERR_VALUE
        # steps_done may be NULL
        nat.check(L.gg_lanczos_probe(K, 0.3, 0, 0, 4, wg.ptr, a, b, None, nat.stream_ptr()))
        assert all(np.isfinite(a[:])) and all(np.isfinite(b[:]))
        wg.read()
    gf = R.matvec_case("growing")[0]
    with kron(nat, gf) as K:
        n_out, n_in, _ = kron_shape(nat, K, 0)
        wg = Guard(4 * max(n_out, n_in))
        a = (ctypes.c_double * 4)(*([SENT] * 4))
        b = (ctypes.c_double * 4)(*([SENT] * 4))
        assert call(K, 4, wg, a, b) == GG_ERR_VALUE
        assert list(a) == [SENT] * 4 and list(b) == [SENT] * 4
        wg.unchanged()


# ========================================================== E. decoded diagonal
def diag_problem(m, seed):
    rng = np.random.default_rng(seed)
    lam = [rng.uniform(0.2, 3.0, mk) for mk in m]
    t = np.ones(1, dtype=LD)
    for l in lam:
        t = np.kron(t, l.astype(LD))
    return lam, t


@pytest.mark.parametrize("m,shift", [([2] * 16, 0.3), ([2] * 16, 0.0), ([1], 0.3), ([1], 0.0),
                                     ([3, 1, 4], 0.0)],
                         ids=["d16", "d16_shift0", "d1m1", "d1m1_shift0", "d3_shift0"])
def test_diag_scale_and_logdet_edges(nat, m, shift):
    """d = 16 with m = 2, d = 1 with m = 1 and shift = 0.  diag_scale: (d + 3) u
    |ref| (d - 1 products, the sum and at most two more operations, each
    rounded once: d + 2 roundings, one unit for their second-order terms); the
    log det against a long-double sum within (n + 64) u sum |log|."""
    L = nat.lib()
    d = len(m)
    lam, t = diag_problem(m, 100 * d + len(m))
    n = t.size
    x = R.vector(n, 43)
    xL = x.astype(LD)
    ts = t + LD(shift)
    refs = {0: xL / ts, 1: t * LD(shift) / ts, 2: xL * ts}
    lg = Guard(sum(m), np.concatenate(lam))
    for mode in (0, 1, 2):
        xg, yg = Guard(n, x), Guard(n)
        nat.check(L.gg_kron_diag_scale(d, nat.i64_array(m), lg.ptr, shift, mode, xg.ptr, yg.ptr,
                                       nat.stream_ptr()), "gg_kron_diag_scale")
        got = yg.read().astype(LD)
        xg.unchanged()
        assert np.all(np.abs(got - refs[mode]) <= (d + 3) * U * np.abs(refs[mode])), (m, mode)
    out = ctypes.c_double(SENT)
    nat.check(L.gg_kron_logdet_shifted(d, nat.i64_array(m), lg.ptr, shift, ctypes.byref(out),
                                       nat.stream_ptr()), "gg_kron_logdet_shifted")
    logs = np.log(ts)
    want, mass = np.sum(logs), np.sum(np.abs(logs))
    print("logdet d=%d shift=%g: |got - ref| %.2e, bound %.2e"
          % (d, shift, abs(out.value - float(want)), float((n + 64) * U * mass)))
    assert abs(LD(out.value) - want) <= (n + 64) * U * mass
    lg.unchanged()


def test_diag_refusals(nat):
    """d = 17 and d = 0, and a NULL m (checked before it is read), are
    GG_ERR_VALUE for the three entry points that decode the diagonal."""
    L = nat.lib()
    lg, xg, yg = Guard(34, np.ones(34)), Guard(4, np.ones(4)), Guard(4)
    s = nat.stream_ptr()
    out = ctypes.c_double(SENT)
    two = (ctypes.c_double * 2)(SENT, SENT)
    for d, m in ((17, nat.i64_array([2] * 17)), (0, nat.i64_array([2])), (2, None),
                 (2, nat.i64_array([2, 0]))):
        assert L.gg_kron_diag_scale(d, m, lg.ptr, 0.3, 0, xg.ptr, yg.ptr, s) == GG_ERR_VALUE
        assert L.gg_kron_logdet_shifted(d, m, lg.ptr, 0.3, ctypes.byref(out), s) == GG_ERR_VALUE
        assert L.gg_kron_trace_ratio(d, m, lg.ptr, 0.3, 1, lg.ptr, two, s) == GG_ERR_VALUE
    assert out.value == SENT and list(two) == [SENT, SENT]
    for g in (lg, xg, yg):
        g.unchanged()
