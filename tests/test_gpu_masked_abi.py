"""The masked CG, masked Lanczos and sampling sections of
include/gp_grief_amd.h at their edges, called through ctypes exactly as a C
caller would (gg_cgm_*, gg_lanczos_probe_masked / _timed / _noise,
gg_sample_*, gg_kron_*_coeffs).

Guarded buffers (abi_guard): every double operand is a payload of exactly the
documented size between 64 NaN doubles, outputs and scratch pre-filled with
NaN; the mask is a payload of exactly n bytes between 64 bytes of 0xFF.  A
refused call must leave every operand and host output bit for bit untouched.

A-D  gg_cgm_*.  The first iterate elementwise inside the derived bound of
     tests/masked_abi_ref.py (x, and r read from the workspace's first vector)
     at every shape, two of them past the grid-stride wrap of the 16-byte-lane
     kernels (n >= 2^20 + 2); three iterations there and 30 at (12, 10, 8)
     against the long-double twin at 100 x float64 NumPy's own distance from
     it (floored at 1e-13); converged solves against dense K_oo algebra at
     1e-8 with the twin's iteration count within 5 %; every combination of
     operand alignments; the iteration-control contract bit for bit.
E    the masked probes: the observed count and three steps past the wrap, an
     exact workspace at both alignments, breakdown at one observed point,
     steps above n_obs, the empty mask, refusals.
F    the sampling kernels past the wrap and with one operand at a time off a
     16-byte boundary.

Float64 NumPy against the long-double twins (tests/test_masked_abi_ref.py,
x86-64): wrap shapes after 3 iterations / steps, x 1.1e-16 .. 5.1e-16, |r|
2.9e-17 .. 8.4e-16, alphas 1.9e-16 .. 4.3e-16, betas 1.3e-16 .. 2.5e-16 (every
tolerance there is the floor, 1e-13); (12, 10, 8) after 30 iterations, x
5.0e-13 (noise) .. 2.1e-10 (noise, preconditioned), |r| 3.8e-16 .. 2.3e-7.

Measured on MI355X (worst ratios, printed by the tests):
  B.1 / C  first iterate, err / bound: x 0.0003 .. 0.033, r 0.0002 .. 0.035
           (highest at the short chains (6, 4) and (5, 1, 4), below 0.0005 past
           the wrap); every alignment combination gives the ratios of the
           aligned run.
  B.2      err / tolerance: wrap shapes x 0.003 .. 0.009 (the second trip
           alone the same), |r| 0.003 .. 0.007; (12, 10, 8) x 0.007 .. 0.033,
           |r| 0.005 .. 0.019.
  B.3      errors 3.5e-13 .. 6.9e-12; iteration counts 0 .. 3.8 % above the
           twin's (1122 against 1081 at (48, 6, 5), noise).
  E        wrap shapes, err / tolerance: alphas 0.003 .. 0.007, betas 0.001 ..
           0.006; small shapes below 4e-7 of the 1e-8 / 1e-7; one observed
           point: alpha_0 to the bit; six points, 12 steps: 1.4e-14 relative.
  F        err / bound: residuals 0.002, accumulation 0.08, coefficients
           0.0003 .. 0.0025.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import kron_abi_ref as R
import masked_abi_ref as M
import masked_ref as mr
import noise_ref as nr
import posterior_sample_ref as ps

from abi_guard import ByteGuard, Guard, bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GG_OK, GG_ERR_VALUE = 0, -1
SENT = -12345.0
NORMAL_TOL = 1e-12
VARIANTS = ["shift", "noise"]
EVEN_WRAP = (104, 101, 100)


def ids(ms):
    return "x".join(map(str, ms)) if isinstance(ms, tuple) else str(ms)


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


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


def fold_mask(nat, K):
    m = ctypes.c_int64(-1)
    nat.check(nat.lib().gg_kron_fold_mask(K, 0, ctypes.byref(m)))
    return m.value


def mixed(mask):
    """The mask with its observed bytes a mix of 1, 2 and 255."""
    vals = np.random.default_rng(17).choice(np.array([1, 2, 255], dtype=np.uint8), mask.size)
    return np.where(mask, vals, 0).astype(np.uint8)


def work_elems(nat, K):
    we = ctypes.c_int64(-1)
    nat.check(nat.lib().gg_cgm_work_elems(K, ctypes.byref(we)), "gg_cgm_work_elems")
    return we.value


class Cgm(object):
    """gg_cgm_* on a guarded workspace of exactly gg_cgm_work_elems doubles,
    NaN-filled (fill None) or filled with a value."""

    def __init__(self, nat, K, n, mg, shift=M.SHIFT, off=0, fill=None):
        self.nat, self.L, self.n = nat, nat.lib(), n
        we = work_elems(nat, K)
        self.wg = Guard(we, None if fill is None else np.full(we, fill), off)
        self.h = ctypes.c_void_p()
        nat.check(self.L.gg_cgm_create(K, shift, mg.ptr, self.wg.ptr, ctypes.byref(self.h)),
                  "gg_cgm_create")

    def start(self, bg, xg, rtol, atol=0.0):
        return self.L.gg_cgm_start(self.h, bg.ptr, xg.ptr, rtol, atol, self.nat.stream_ptr())

    def iterate(self, max_iters, check_every):
        return self.L.gg_cgm_iterate(self.h, max_iters, check_every, self.nat.stream_ptr())

    def status(self):
        it, cv = ctypes.c_int(-1), ctypes.c_int(-1)
        rn, tol = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        self.nat.check(self.L.gg_cgm_status(self.h, ctypes.byref(it), ctypes.byref(cv),
                                            ctypes.byref(rn), ctypes.byref(tol),
                                            self.nat.stream_ptr()))
        return it.value, cv.value, rn.value, tol.value

    def r(self):
        """The residual: the first vector of the workspace after rounding
        work_dev up to 256 bytes."""
        base = (self.wg.ptr.value + 255) & ~255
        o = (base - self.wg.d.data_ptr()) // 8
        assert self.wg.lo <= o and o + self.n <= self.wg.lo + self.wg.n
        return self.wg._host()[o:o + self.n].copy()

    def close(self):
        import torch
        torch.cuda.synchronize()
        assert self.L.gg_cgm_destroy(self.h) == GG_OK
        self.wg.read()


class Precond(object):
    """The eigenvector operator and eigenvalue table of gg_cgm_set_precond,
    from masked_ref.factor_eigh (the twin's own float64 eigenpairs)."""

    def __init__(self, nat, F):
        Q, lam = mr.factor_eigh(F)
        self.ctx = kron(nat, Q)
        self.Q = self.ctx.__enter__()
        self.lg = Guard(sum(l.size for l in lam), np.concatenate(lam))

    def close(self):
        self.lg.unchanged()
        self.ctx.__exit__(None, None, None)


def pshift(c, variant):
    return M.SHIFT if variant == "shift" else nr.geometric_mean(c["mask"], c["noise"])


def solve(nat, K, c, variant, iters, rtol=0.0, precond=None, mask_bytes=None, moff=0, boff=0,
          xoff=0, noff=0, woff=0, fill=None, b=None, noise=None, chunks=None, stream=None,
          check_every=1, want_r=False):
    """One guarded solve: dict(x, r, status); asserts b, the noise, the mask and
    the workspace's guards untouched.  chunks: a list of (max_iters,
    check_every) calls instead of one."""
    import torch
    n = c["n"]
    mg = ByteGuard(c["mask"].astype(np.uint8) if mask_bytes is None else mask_bytes, moff)
    bg, xg = Guard(n, c["b"] if b is None else b, boff), Guard(n, None, xoff)
    ng = Guard(n, c["noise"] if noise is None else noise, noff) if variant == "noise" else None
    pc = Precond(nat, c["F"]) if precond else None
    ctx = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with ctx:
        cg = Cgm(nat, K, n, mg, pshift(c, variant), woff, fill)
        if pc is not None:
            nat.check(cg.L.gg_cgm_set_precond(cg.h, pc.Q, pc.lg.ptr), "gg_cgm_set_precond")
        if ng is not None:
            nat.check(cg.L.gg_cgm_set_noise(cg.h, ng.ptr), "gg_cgm_set_noise")
        assert cg.start(bg, xg, rtol) == GG_OK
        for mi, ce in (chunks if chunks is not None else [(iters, check_every)]):
            assert cg.iterate(mi, ce) == GG_OK
        st = cg.status()
    out = dict(x=xg.read(), status=st, r=cg.r() if want_r else None)
    bg.unchanged()
    mg.unchanged()
    if ng is not None:
        ng.unchanged()
    cg.close()
    if pc is not None:
        pc.close()
    return out


def same_bits(a, b):
    return np.array_equal(bits(a["x"]), bits(b["x"])) and a["status"] == b["status"]


# ======================================================= A. handle and setters
def test_cgm_create_and_setter_refusals(nat):
    L = nat.lib()
    ms = (7, 5, 3)
    c = M.small_case(ms)
    n = c["n"]
    HSENT = 0x5A5A5A5A
    with kron(nat, c["F"]) as K:
        we = work_elems(nat, K)
        e = ctypes.c_int64(-9)
        assert L.gg_cgm_work_elems(None, ctypes.byref(e)) == GG_ERR_VALUE and e.value == -9
        assert L.gg_cgm_work_elems(K, None) == GG_ERR_VALUE
        mg, wg = ByteGuard(c["mask"]), Guard(we)

        def refused(Kh, shift, mp, wp, with_out=True):
            out = ctypes.c_void_p(HSENT)
            st = L.gg_cgm_create(Kh, shift, mp, wp, ctypes.byref(out) if with_out else None)
            assert st == GG_ERR_VALUE and out.value == HSENT, (st, out.value)

        refused(None, M.SHIFT, mg.ptr, wg.ptr)
        refused(K, M.SHIFT, mg.ptr, None)
        refused(K, M.SHIFT, mg.ptr, wg.ptr, with_out=False)
        refused(K, M.SHIFT, None, wg.ptr)
        refused(K, 0.0, mg.ptr, wg.ptr)
        refused(K, -1.0, mg.ptr, wg.ptr)
        refused(K, float("nan"), mg.ptr, wg.ptr)
        refused(K, M.SHIFT, mg.ptr, ctypes.c_void_p(wg.ptr.value + 4))
        wg.unchanged()
        mg.unchanged()
        assert L.gg_cgm_destroy(None) == GG_OK

        # ---- gg_cgm_set_precond
        pc = Precond(nat, c["F"])
        Qf = mr.factor_eigh(c["F"])[0]
        cg = Cgm(nat, K, n, mg)
        bg, xg, ng = Guard(n, c["b"]), Guard(n), Guard(n, c["noise"])
        assert L.gg_cgm_set_precond(None, pc.Q, pc.lg.ptr) == GG_ERR_VALUE
        assert L.gg_cgm_set_precond(cg.h, pc.Q, None) == GG_ERR_VALUE
        with kron(nat, [np.eye(7), np.eye(15)]) as Q2:                       # another d
            assert L.gg_cgm_set_precond(cg.h, Q2, pc.lg.ptr) == GG_ERR_VALUE
        with kron(nat, [Qf[0], np.eye(4), Qf[2]]) as Q3:                     # one other order
            assert L.gg_cgm_set_precond(cg.h, Q3, pc.lg.ptr) == GG_ERR_VALUE
        with kron(nat, [Qf[0], np.eye(5)[:, :4], Qf[2]]) as Q4:              # not square
            assert L.gg_cgm_set_precond(cg.h, Q4, pc.lg.ptr) == GG_ERR_VALUE
        # ---- gg_cgm_set_noise
        assert L.gg_cgm_set_noise(None, ng.ptr) == GG_ERR_VALUE
        assert L.gg_cgm_set_noise(cg.h, ctypes.c_void_p(ng.ptr.value + 4)) == GG_ERR_VALUE
        # after the refusals the handle is the plain one
        assert cg.start(bg, xg, 0.0) == GG_OK
        assert L.gg_cgm_set_precond(cg.h, pc.Q, pc.lg.ptr) == GG_ERR_VALUE   # after start
        assert L.gg_cgm_set_precond(cg.h, None, None) == GG_ERR_VALUE
        assert L.gg_cgm_set_noise(cg.h, ng.ptr) == GG_ERR_VALUE
        assert L.gg_cgm_set_noise(cg.h, None) == GG_ERR_VALUE
        assert cg.iterate(5, 1) == GG_OK
        got = dict(x=xg.read(), status=cg.status())
        cg.close()
        for g in (bg, ng, pc.lg, mg):
            g.unchanged()
        plain = solve(nat, K, c, "shift", 5)
        assert same_bits(got, plain)

        # set and taken back before start: the bits of a handle that never had it
        cg = Cgm(nat, K, n, mg)
        nat.check(L.gg_cgm_set_precond(cg.h, pc.Q, pc.lg.ptr))
        nat.check(L.gg_cgm_set_precond(cg.h, None, pc.lg.ptr))
        nat.check(L.gg_cgm_set_noise(cg.h, ng.ptr))
        nat.check(L.gg_cgm_set_noise(cg.h, None))
        xg = Guard(n)
        assert cg.start(bg, xg, 0.0) == GG_OK and cg.iterate(5, 1) == GG_OK
        assert same_bits(dict(x=xg.read(), status=cg.status()), plain)
        cg.close()
        pc.close()


def test_cgm_status_before_start_and_null_outputs(nat):
    """A created, unstarted handle: iters = 0, converged = 0 (its zeroed
    scalars are not a solved system).  Each output pointer may be NULL."""
    L = nat.lib()
    c = M.small_case((7, 5, 3))
    with kron(nat, c["F"]) as K:
        mg = ByteGuard(c["mask"])
        cg = Cgm(nat, K, c["n"], mg)
        it, conv, rn, tol = cg.status()
        assert (it, conv) == (0, 0), (it, conv)
        assert cg.iterate(5, 1) == GG_ERR_VALUE
        assert L.gg_cgm_status(None, None, None, None, None, nat.stream_ptr()) == GG_ERR_VALUE
        bg, xg = Guard(c["n"], c["b"]), Guard(c["n"])
        assert cg.start(bg, xg, 1e-6) == GG_OK and cg.iterate(3, 1) == GG_OK
        full = cg.status()
        assert full[:2] == (3, 0)
        s = nat.stream_ptr()
        assert L.gg_cgm_status(cg.h, None, None, None, None, s) == GG_OK
        for k in range(4):
            it, cv = ctypes.c_int(-1), ctypes.c_int(-1)
            rn, tol = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
            args = [ctypes.byref(it), ctypes.byref(cv), ctypes.byref(rn), ctypes.byref(tol)]
            args[k] = None
            assert L.gg_cgm_status(cg.h, *args, s) == GG_OK
            got = [it.value, cv.value, rn.value, tol.value]
            want = list(full)
            want[k] = -1
            assert got == want, (k, got, want)
        cg.close()


# ============================================= B. the solve against the reference
@pytest.mark.parametrize("ms", M.SMALL_SHAPES + M.WRAP_SHAPES, ids=ids)
def test_first_iterate_within_bound(nat, ms):
    """B.1: one iteration; x and r elementwise inside first_iterate's bound,
    exactly 0 at the missing points.  The mask at byte offset 1 with observed
    bytes 1, 2 and 255 gives the same bits."""
    c = M.cg_case(ms)
    miss = ~c["mask"]
    with kron(nat, c["F"]) as K:
        assert fold_mask(nat, K) == R.fold_mask(c["F"])
        for variant in VARIANTS:
            fi = M.first_case(ms, variant)
            a = solve(nat, K, c, variant, 1, want_r=True)
            assert a["status"][0] == 1
            rx = R.worst_ratio(a["x"], fi["x"], fi["bx"])
            rr = R.worst_ratio(a["r"], fi["r"], fi["br"])
            print("first iterate %s %s: err/bound x %.4f r %.4f" % (ms, variant, rx, rr))
            assert rx <= 1.0 and rr <= 1.0, (ms, variant, rx, rr)
            assert np.all(bits(a["x"][miss]) == 0) and np.all(a["r"][miss] == 0)
            rn = float(M.norm(a["r"]))
            assert abs(a["status"][2] - rn) <= (c["n"] + 8) * U * rn
            b = solve(nat, K, c, variant, 1, mask_bytes=mixed(c["mask"]), moff=1, want_r=True)
            assert same_bits(a, b) and np.array_equal(bits(a["r"]), bits(b["r"]))


FIXED = [(ms, v, None, M.WRAP_ITERS) for ms in M.WRAP_SHAPES for v in VARIANTS] + \
        [((12, 10, 8), v, p, 30) for v in VARIANTS for p in (None, "kron")]


@pytest.mark.parametrize("ms,variant,precond,iters", FIXED,
                         ids=["%s-%s-%s" % (ids(m), v, p) for m, v, p, _ in FIXED])
def test_fixed_iterations_against_the_twin(nat, ms, variant, precond, iters):
    """B.2: rtol = 0; x norm-wise against the long-double twin, over all
    indices and over those of the second grid-stride trip alone, and
    gg_cgm_status's resid_norm against the twin's |r|."""
    c = M.cg_case(ms)
    tw = M.cg_twin(ms, variant, precond, iters)
    tol_x, tol_r = M.tolerance(tw["fig_x"]), M.tolerance(tw["fig_rn"])
    with kron(nat, c["F"]) as K:
        a = solve(nat, K, c, variant, iters, precond=precond, check_every=0)
    it, conv, rn, tol = a["status"]
    assert (it, conv, tol) == (iters, 0, 0.0)
    ex = M.rel(a["x"], tw["x"])
    er = float(abs(LD(rn) - tw["rn"]) / tw["rn"])
    print("fixed %d iterations %s %s precond=%s: x err/tol %.4f (tol %.1e), |r| err/tol %.4f "
          "(tol %.1e)" % (iters, ms, variant, precond, ex / tol_x, tol_x, er / tol_r, tol_r))
    assert ex <= tol_x and er <= tol_r
    assert np.all(bits(a["x"][~c["mask"]]) == 0)
    if c["n"] > M.WRAP:
        et = M.rel(a["x"][M.WRAP:], tw["x"][M.WRAP:])
        print("    second trip alone: x err/tol %.4f" % (et / tol_x))
        assert et <= tol_x


@pytest.mark.parametrize("ms", M.SMALL_SHAPES, ids=ids)
def test_converged_solves(nat, ms):
    """B.3: rtol = 1e-11, the four variants; dense K_oo algebra at 1e-8, the
    twin's iteration count within 5 %."""
    c = M.small_case(ms)
    with kron(nat, c["F"]) as K:
        for variant in VARIANTS:
            for precond in (None, "kron"):
                tw = M.converged_twin(ms, variant, precond)
                a = solve(nat, K, c, variant, 20 * c["n"], rtol=M.CONVERGED_RTOL, precond=precond,
                          check_every=1)
                it, conv, rn, tol = a["status"]
                e = M.rel(a["x"], tw["dense"])
                print("converged %s %s precond=%s: %d iters (twin %d), err %.2e"
                      % (ms, variant, precond, it, tw["iters"], e))
                assert conv == 1 and rn < tol and e < 1e-8
                assert abs(it - tw["iters"]) <= 0.05 * tw["iters"], (it, tw["iters"])
                assert np.all(bits(a["x"][~c["mask"]]) == 0)


# =========================================== C. alignment, scratch, determinism
@pytest.mark.parametrize("ms", [(12, 10, 8), EVEN_WRAP], ids=ids)
def test_alignment_combinations(nat, ms):
    """b and x (no noise), x and noise (noise) independently 16-byte aligned
    or one double off: each combination inside B.1's bound.  The workspace of
    exactly gg_cgm_work_elems doubles at offset 0 and 1: guards intact (checked
    by every solve), the same bits."""
    c = M.cg_case(ms)
    with kron(nat, c["F"]) as K:
        for variant in VARIANTS:
            fi = M.first_case(ms, variant)
            for o1 in (0, 1):
                for o2 in (0, 1):
                    kw = dict(boff=o1, xoff=o2) if variant == "shift" else dict(xoff=o1, noff=o2)
                    a = solve(nat, K, c, variant, 1, want_r=True, **kw)
                    rx = R.worst_ratio(a["x"], fi["x"], fi["bx"])
                    rr = R.worst_ratio(a["r"], fi["r"], fi["br"])
                    print("alignment %s %s %s: err/bound x %.4f r %.4f" % (ms, variant, kw, rx, rr))
                    assert rx <= 1.0 and rr <= 1.0, (ms, variant, kw, rx, rr)
            w0 = solve(nat, K, c, variant, M.WRAP_ITERS, woff=0, want_r=True)
            w1 = solve(nat, K, c, variant, M.WRAP_ITERS, woff=1, want_r=True)
            assert same_bits(w0, w1) and np.array_equal(bits(w0["r"]), bits(w1["r"]))


@pytest.mark.parametrize("ms", [(12, 10, 8), EVEN_WRAP], ids=ids)
def test_bitwise_pairs(nat, ms):
    """NaN-filled against zero-filled scratch; NaN against finite b and noise
    at the missing points; a restarted against a fresh handle; a side stream
    against the default one; three ways of chunking the same iterations."""
    import torch
    c = M.cg_case(ms)
    n, mask = c["n"], c["mask"]
    iters = 30 if n < M.WRAP else M.WRAP_ITERS
    other = np.random.default_rng(23).standard_normal(n)
    with kron(nat, c["F"]) as K:
        for variant in VARIANTS:
            precs = (None, "kron") if n < M.WRAP else (None,)
            for precond in precs:
                base = solve(nat, K, c, variant, iters, precond=precond)
                assert base["status"][0] == iters and np.all(np.isfinite(base["x"]))
                zero = solve(nat, K, c, variant, iters, precond=precond, fill=0.0)
                assert same_bits(base, zero), "uninitialised scratch reached the result"
                nanb = solve(nat, K, c, variant, iters, precond=precond,
                             b=np.where(mask, c["b"], np.nan),
                             noise=np.where(mask, c["noise"], np.nan))
                assert same_bits(base, nanb)
                side = solve(nat, K, c, variant, iters, precond=precond,
                             stream=torch.cuda.Stream())
                assert same_bits(base, side)
                if n < M.WRAP:
                    chunkings = ([(10, 0)] * 3, [(30, 7)], [(30, 0)])
                else:
                    chunkings = ([(1, 0)] * 3, [(3, 2)], [(3, 0)])
                for ch in chunkings:
                    assert same_bits(base, solve(nat, K, c, variant, iters, precond=precond,
                                                 chunks=ch)), ch
            # a second gg_cgm_start on a started handle, against a fresh handle
            mg = ByteGuard(mask)
            ng = Guard(n, c["noise"]) if variant == "noise" else None
            cg = Cgm(nat, K, n, mg, pshift(c, variant))
            if ng is not None:
                nat.check(cg.L.gg_cgm_set_noise(cg.h, ng.ptr))
            og, xg = Guard(n, other), Guard(n)
            assert cg.start(og, xg, 0.0) == GG_OK and cg.iterate(2, 1) == GG_OK
            assert cg.status()[0] == 2
            bg, x2 = Guard(n, c["b"]), Guard(n)
            assert cg.start(bg, x2, 0.0) == GG_OK
            assert cg.status()[0] == 0
            assert cg.iterate(iters, 0) == GG_OK
            again = dict(x=x2.read(), status=cg.status())
            cg.close()
            assert same_bits(again, solve(nat, K, c, variant, iters))


# ========================================================= D. iteration control
def test_iteration_control(nat):
    c = M.small_case((12, 10, 8))
    n, mask = c["n"], c["mask"]
    with kron(nat, c["F"]) as K:
        p1 = solve(nat, K, c, "shift", 10 * n, rtol=1e-6, check_every=1)
        it1, conv, rn, tol = p1["status"]
        assert conv == 1 and 0 < it1 < 10 * n and rn < tol
        p0 = solve(nat, K, c, "shift", 3 * it1 + 7, rtol=1e-6, check_every=0)
        pk = solve(nat, K, c, "shift", 3 * it1 + 7, rtol=1e-6, check_every=1000)
        assert same_bits(p1, p0) and same_bits(p1, pk)
        print("iteration control: stops at %d iterations under every polling mode" % it1)
        # further calls after convergence; max_iters <= 0
        more = solve(nat, K, c, "shift", 0, rtol=1e-6,
                     chunks=[(0, 1), (-3, 1), (0, 0), (-3, 0), (10 * n, 1), (5, 1), (5, 0)])
        assert same_bits(p1, more)
        none = solve(nat, K, c, "shift", 0, rtol=1e-6, chunks=[(0, 1), (-3, 1), (0, 0), (-3, 0)])
        assert none["status"][:2] == (0, 0) and np.all(bits(none["x"]) == 0)
        # b = 0 on the observed set, NaN elsewhere
        z = solve(nat, K, c, "shift", 5, rtol=1e-6, b=np.where(mask, 0.0, np.nan))
        assert z["status"][:3] == (0, 1, 0.0) and np.all(bits(z["x"]) == 0)
        # a NaN in b at one observed point: the done flag stops on NaN
        bn = c["b"].copy()
        bn[np.nonzero(mask)[0][3]] = np.nan
        q = solve(nat, K, c, "shift", 5, rtol=1e-6, b=bn)
        assert q["status"][:2] == (0, 0) and np.all(bits(q["x"]) == 0)
        # tolerances
        mg = ByteGuard(mask)
        cg = Cgm(nat, K, n, mg)
        bg, xg = Guard(n, c["b"]), Guard(n)
        for rtol, atol in ((-1e-3, 0.0), (float("nan"), 0.0), (1e-6, float("nan")), (1e-6, -1.0)):
            assert cg.start(bg, xg, rtol, atol) == GG_ERR_VALUE
        s = nat.stream_ptr()
        assert cg.L.gg_cgm_start(cg.h, None, xg.ptr, 1e-6, 0.0, s) == GG_ERR_VALUE
        assert cg.L.gg_cgm_start(cg.h, bg.ptr, None, 1e-6, 0.0, s) == GG_ERR_VALUE
        assert cg.L.gg_cgm_start(None, bg.ptr, xg.ptr, 1e-6, 0.0, s) == GG_ERR_VALUE
        xg.unchanged()
        bg.unchanged()
        assert cg.iterate(1, 1) == GG_ERR_VALUE        # still not started
        assert cg.status()[:2] == (0, 0)
        assert cg.start(bg, xg, 0.0, 0.0) == GG_OK and cg.iterate(3, 1) == GG_OK
        assert cg.status()[:2] == (3, 0) and cg.status()[3] == 0.0
        cg.close()


# ============================================================ E. masked Lanczos
def lz(nat, K, n, mg, steps, shift=None, ng=None, wg=None, seed=M.WRAP_SEED, probe=M.WRAP_PROBE,
       done=True, nobs=True, timed=False, expect=GG_OK):
    """One probe on a guarded workspace of exactly 4 n doubles: dict(a, b, done,
    nobs) with the host outputs pre-filled with sentinels."""
    L = nat.lib()
    wg = Guard(4 * n) if wg is None else wg
    a = (ctypes.c_double * steps)(*([SENT] * steps))
    b = (ctypes.c_double * steps)(*([SENT] * steps))
    dn, no = ctypes.c_int(-7), ctypes.c_int64(-7)
    dp = ctypes.byref(dn) if done else None
    npt = ctypes.byref(no) if nobs else None
    s = nat.stream_ptr()
    if ng is not None:
        st = L.gg_lanczos_probe_masked_noise(K, ng.ptr, mg.ptr, seed, probe, steps, wg.ptr, a, b,
                                             dp, npt, s)
    elif timed:
        ms_ = (ctypes.c_double * steps)(*([SENT] * steps))
        st = L.gg_lanczos_probe_masked_timed(K, shift, mg.ptr, seed, probe, steps, wg.ptr, a, b,
                                             dp, npt, ms_, s)
    else:
        st = L.gg_lanczos_probe_masked(K, shift, mg.ptr, seed, probe, steps, wg.ptr, a, b, dp,
                                       npt, s)
    assert st == expect, (st, nat.last_error())
    wg.read()
    mg.unchanged()
    if ng is not None:
        ng.unchanged()
    return dict(a=np.array(a[:]), b=np.array(b[:]), done=dn.value, nobs=no.value)


@pytest.mark.parametrize("ms", M.WRAP_SHAPES, ids=ids)
def test_lanczos_past_the_wrap(nat, ms):
    """Three steps: *n_observed is mask.sum() exactly (a skipped or doubled
    trip of the count pass shows here alone); alphas and betas against the
    long-double twin."""
    c = M.wrap_case(ms, "lanczos")
    n, k = c["n"], M.WRAP_ITERS
    with kron(nat, c["F"]) as K:
        for fam in ("lz", "lz_noise"):
            tw = M.wrap_twin(ms, fam)
            mg = ByteGuard(mixed(c["mask"]), 1)
            ng = Guard(n, np.where(c["mask"], c["noise"], np.nan)) if fam == "lz_noise" else None
            g = lz(nat, K, n, mg, k, shift=M.WRAP_SHIFT, ng=ng)
            assert g["nobs"] == int(c["mask"].sum()) and g["done"] == k
            ea, eb = M.max_rel(g["a"], tw["alphas"]), M.max_rel(g["b"], tw["betas"])
            ta, tb = M.tolerance(tw["fig_a"]), M.tolerance(tw["fig_b"])
            print("lanczos %s %s: alphas err/tol %.4f betas err/tol %.4f (tol %.1e, %.1e)"
                  % (fam, ms, ea / ta, eb / tb, ta, tb))
            assert ea <= ta and eb <= tb


@pytest.mark.parametrize("ms", [(7, 5, 3), (12, 10, 8)], ids=ids)
def test_lanczos_exact_workspace_and_alignment(nat, ms):
    """work_dev of exactly 4 n doubles, 16-byte aligned and one double off
    (with an odd n every vector of the rotation then changes alignment),
    NaN-filled and zero-filled; the noise independently aligned or not.  Each
    run against the twin at the feature tests' 1e-8 (alphas) / 1e-7 (betas);
    the two fills bit for bit."""
    c = M.small_case(ms)
    n, steps = c["n"], 8
    with kron(nat, c["F"]) as K:
        for fam in ("lz", "lz_noise"):
            kw = dict(shift=M.SHIFT) if fam == "lz" else dict(noise=c["noise"])
            ta, tb, done = M.lanczos_ld(c["F"], c["mask"], seed=3, probe=2, steps=steps, **kw)
            assert done == steps
            worst = 0.0
            for woff in (0, 1):
                for noff in (0, 1) if fam == "lz_noise" else (0,):
                    runs = []
                    for fill in (None, 0.0):
                        mg = ByteGuard(c["mask"], woff)
                        ng = Guard(n, c["noise"], noff) if fam == "lz_noise" else None
                        wg = Guard(4 * n, None if fill is None else np.zeros(4 * n), woff)
                        g = lz(nat, K, n, mg, steps, shift=M.SHIFT, ng=ng, wg=wg, seed=3, probe=2)
                        assert g["done"] == steps and g["nobs"] == int(c["mask"].sum())
                        ea, eb = M.max_rel(g["a"], ta), M.max_rel(g["b"], tb)
                        worst = max(worst, ea / 1e-8, eb / 1e-7)
                        assert ea <= 1e-8 and eb <= 1e-7, (fam, woff, noff, fill, ea, eb)
                        runs.append(g)
                    assert np.array_equal(bits(runs[0]["a"]), bits(runs[1]["a"]))
                    assert np.array_equal(bits(runs[0]["b"]), bits(runs[1]["b"]))
            print("lanczos %s %s, exact workspace: worst err/tol %.2e" % (fam, ms, worst))
        # shift = 0 is accepted by the scalar probe and matches the twin
        mg = ByteGuard(c["mask"])
        g = lz(nat, K, n, mg, 4, shift=0.0, seed=3, probe=2)
        ta, tb, _ = M.lanczos_ld(c["F"], c["mask"], shift=0.0, seed=3, probe=2, steps=4)
        assert M.max_rel(g["a"], ta) <= 1e-8 and M.max_rel(g["b"], tb) <= 1e-7
        # NULL steps_done, NULL n_observed, both: the same bits
        ref = lz(nat, K, n, mg, 4, shift=M.SHIFT, seed=3, probe=2)
        ng = Guard(n, c["noise"])
        refn = lz(nat, K, n, mg, 4, ng=ng, seed=3, probe=2)
        for done, nobs in ((False, True), (True, False), (False, False)):
            g = lz(nat, K, n, mg, 4, shift=M.SHIFT, seed=3, probe=2, done=done, nobs=nobs)
            assert np.array_equal(bits(g["a"]), bits(ref["a"]))
            assert np.array_equal(bits(g["b"]), bits(ref["b"]))
            assert g["done"] == (4 if done else -7) and g["nobs"] == (ref["nobs"] if nobs else -7)
            g = lz(nat, K, n, mg, 4, ng=ng, seed=3, probe=2, done=done, nobs=nobs)
            assert np.array_equal(bits(g["a"]), bits(refn["a"]))
            g = lz(nat, K, n, mg, 4, shift=M.SHIFT, seed=3, probe=2, done=done, nobs=nobs,
                   timed=True)
            assert np.array_equal(bits(g["a"]), bits(ref["a"]))


@pytest.mark.parametrize("where", ["last", "first"])
def test_lanczos_one_observed_point(nat, where):
    """v_0 = +-e_i: beta_0 is an exact 0 (w = Y - (u Y) u, u = +-1), one step
    done, alpha_0 = K_ii + shift (+ noise_i) and the later entries exact
    zeros."""
    ms = (7, 5, 3)
    c = M.small_case(ms)
    n = c["n"]
    i = n - 1 if where == "last" else 0
    mask = np.zeros(n, dtype=np.uint8)
    mask[i] = 255
    kii = np.prod([LD(f[j, j]) for f, j in zip(c["F"], np.unravel_index(i, ms))])
    with kron(nat, c["F"]) as K:
        mg = ByteGuard(mask)
        for ng, add in ((None, LD(M.SHIFT)), (Guard(n, c["noise"]), LD(c["noise"][i]))):
            g = lz(nat, K, n, mg, 4, shift=M.SHIFT, ng=ng)
            want = float(kii + add)
            assert g["done"] == 1 and g["nobs"] == 1
            ulps = abs(g["a"][0] - want) / np.spacing(want)
            print("one observed point (%s, noise %s): alpha_0 off by %.1f ulp"
                  % (where, ng is not None, ulps))
            assert ulps <= 8
            assert np.all(g["b"] == 0.0) and np.all(g["a"][1:] == 0.0), (g["a"], g["b"])


def test_lanczos_steps_above_n_obs(nat):
    """Six observed points, 12 steps: every entry finite, and n_obs times the
    quadrature of the leading steps_done block equals z_o^T log(K_oo + s I)
    z_o within 1e-9 relative (the bound of the unmasked
    test_lanczos_near_breakdown_and_steps_above_n)."""
    ms = M.SIX_SHAPE
    F = mr.rbf_factors(ms)
    n = int(np.prod(ms))
    mask = np.zeros(n, dtype=bool)
    mask[M.SIX_POINTS] = True
    want = M.dense_quadratic_log(F, mask, M.SHIFT, 3, 2)
    with kron(nat, F) as K:
        g = lz(nat, K, n, ByteGuard(mask), 12, shift=M.SHIFT, seed=3, probe=2)
    assert g["nobs"] == 6 and 1 <= g["done"] <= 12
    assert np.all(np.isfinite(g["a"])) and np.all(np.isfinite(g["b"])), (g["a"], g["b"])
    got = 6 * M.quadrature(g["a"], g["b"], g["done"])
    print("six points, 12 steps: done %d, min beta %.2e, device %.15g dense %.15g rel diff %.2e"
          % (g["done"], float(np.min(g["b"][:g["done"]])), got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-9 * abs(want)


def test_lanczos_empty_mask_and_refusals(nat):
    L = nat.lib()
    c = M.small_case((7, 5, 3))
    n = c["n"]
    with kron(nat, c["F"]) as K:
        empty = ByteGuard(np.zeros(n, dtype=np.uint8))
        ng = Guard(n, c["noise"])
        # found after the run: the count is written, nothing else
        for kw in (dict(shift=M.SHIFT), dict(shift=M.SHIFT, timed=True), dict(ng=ng)):
            g = lz(nat, K, n, empty, 4, expect=GG_ERR_VALUE, **kw)
            assert g["nobs"] == 0 and g["done"] == -7
            assert list(g["a"]) == [SENT] * 4 and list(g["b"]) == [SENT] * 4
        # before any launch: everything untouched
        mg, wg = ByteGuard(c["mask"]), Guard(4 * n)
        a = (ctypes.c_double * 4)(*([SENT] * 4))
        b = (ctypes.c_double * 4)(*([SENT] * 4))
        dn, no = ctypes.c_int(-7), ctypes.c_int64(-7)
        s = nat.stream_ptr()

        def noise_call(Kh, npx, mp, steps, wp, ap, bp):
            return L.gg_lanczos_probe_masked_noise(Kh, npx, mp, 3, 2, steps, wp, ap, bp,
                                                   ctypes.byref(dn), ctypes.byref(no), s)

        ok = (K, ng.ptr, mg.ptr, 4, wg.ptr, a, b)
        for k, bad in ((1, ctypes.c_void_p(ng.ptr.value + 4)), (1, None), (4, None), (5, None),
                       (6, None), (3, 0), (3, -2), (2, None), (0, None)):
            args = list(ok)
            args[k] = bad
            assert noise_call(*args) == GG_ERR_VALUE, (k, bad)

        def scalar_call(shift, mp, steps, wp, ap, bp):
            return L.gg_lanczos_probe_masked(K, shift, mp, 3, 2, steps, wp, ap, bp,
                                             ctypes.byref(dn), ctypes.byref(no), s)

        for args in ((-1e-3, mg.ptr, 4, wg.ptr, a, b), (M.SHIFT, None, 4, wg.ptr, a, b),
                     (M.SHIFT, mg.ptr, 0, wg.ptr, a, b), (M.SHIFT, mg.ptr, 4, None, a, b),
                     (M.SHIFT, mg.ptr, 4, wg.ptr, None, b), (M.SHIFT, mg.ptr, 4, wg.ptr, a, None)):
            assert scalar_call(*args) == GG_ERR_VALUE, args
        assert L.gg_lanczos_probe_masked_timed(K, M.SHIFT, mg.ptr, 3, 2, 4, wg.ptr, a, b,
                                               ctypes.byref(dn), ctypes.byref(no), None,
                                               s) == GG_ERR_VALUE
        assert list(a) == [SENT] * 4 and list(b) == [SENT] * 4
        assert dn.value == -7 and no.value == -7
        for g in (wg, mg, ng):
            g.unchanged()


# ================================================================== F. sampling
class Sent(object):
    """n doubles between two pairs of 777.0 sentinels, the payload `off`
    doubles past a 16-byte boundary."""

    def __init__(self, n, data=None, off=0):
        import torch
        self.n, self.lo = int(n), 2 + int(off)
        h = np.full(self.lo + self.n + 2, 777.0)
        if data is not None:
            h[self.lo:self.lo + self.n] = data
        self.h0 = h
        self.d = torch.from_numpy(h.copy()).cuda()
        assert self.d.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.d.data_ptr() + 8 * self.lo)

    def read(self):
        import torch
        torch.cuda.synchronize()
        g = self.d.cpu().numpy()
        assert np.all(g[:self.lo] == 777.0) and np.all(g[self.lo + self.n:] == 777.0)
        return g[self.lo:self.lo + self.n].copy()

    def unchanged(self):
        import torch
        torch.cuda.synchronize()
        assert np.array_equal(bits(self.d.cpu().numpy()), bits(self.h0))


BIG = (1 << 20) + 3
SD = 0.1
_sample = {}


def sample_problem(n):
    """y, f, w, mask, noise and the streams' normals at length n, once."""
    if n not in _sample:
        rng = np.random.default_rng(29)
        mask = rng.random(n) < 0.7
        mask[0], mask[n - 1] = False, True
        p = dict(mask=mask, y=np.where(mask, rng.standard_normal(n), np.nan),
                 f=rng.standard_normal(n), noise=np.where(mask, nr.NOISE_VAR * nr.noise_scale(n),
                                                          np.nan),
                 F3=rng.standard_normal((n, 3)), W3=rng.standard_normal((n, 3)),
                 z=ps.normal_stream(5, 9, n))
        for a in p.values():
            a.setflags(write=False)
        _sample[n] = p
    return _sample[n]


def residual_check(p, got, noise):
    mask = p["mask"]
    sd = np.sqrt(np.where(mask, p["noise"], 0.0)) if noise else np.full(mask.size, SD)
    with np.errstate(invalid="ignore"):
        ref = np.where(mask, p["y"] - p["f"] - sd * p["z"], 0.0)
    assert np.all(bits(got[~mask]) == 0)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (1e-12 * np.abs(ref) + NORMAL_TOL * sd))
    assert np.all(r <= 1.0), float(np.max(r))
    return float(np.max(r))


def run_residual(nat, p, noise, offs=(0, 0, 0, 0)):
    """offs: the offsets of y, f, noise, b."""
    n = p["mask"].size
    yg, fg, bg = Sent(n, p["y"], offs[0]), Sent(n, p["f"], offs[1]), Sent(n, None, offs[3])
    mg = ByteGuard(mixed(p["mask"]), 1)
    L, s = nat.lib(), nat.stream_ptr()
    if noise:
        ng = Sent(n, p["noise"], offs[2])
        nat.check(L.gg_sample_residual_noise(yg.ptr, fg.ptr, ng.ptr, mg.ptr, 5, 9, bg.ptr, n, s))
        ng.unchanged()
    else:
        nat.check(L.gg_sample_residual(yg.ptr, fg.ptr, mg.ptr, SD, 5, 9, bg.ptr, n, s))
    got = bg.read()
    for g in (yg, fg, mg):
        g.unchanged()
    return got


def accumulate_check(p, out, mean, m2):
    """out is f + w to the bit.  mean and m2 against
    posterior_sample_ref.welford: with s = max_k |x_k| every quantity of a
    Welford step is at most 2 s (dlt, x - mean) or 4 s^2 (their product), a
    step adds a few u of those, and the restatement carries as much: 32 u s
    and 128 u s^2 over the two updating steps."""
    X = p["F3"] + p["W3"]
    assert np.array_equal(bits(out), bits(X[:, 2]))
    rm, rq = ps.welford(X)
    s = np.max(np.abs(X), axis=1)
    em = float(np.max(np.abs(mean - rm) / (32 * U * s)))
    eq = float(np.max(np.abs(m2 - rq) / (128 * U * s * s)))
    assert em <= 1.0 and eq <= 1.0, (em, eq)
    return max(em, eq)


def run_accumulate(nat, p, offs=(0, 0, 0, 0, 0), alias=None):
    """Three draws folded in; offs: the offsets of f, w, out, mean, m2.
    alias 'f' or 'w': out is that operand."""
    n = p["mask"].size
    L, s = nat.lib(), nat.stream_ptr()
    og, eg, qg = Sent(n, None, offs[2]), Sent(n, None, offs[3]), Sent(n, None, offs[4])
    for k in range(3):
        fg, wg = Sent(n, p["F3"][:, k], offs[0]), Sent(n, p["W3"][:, k], offs[1])
        tgt = {None: og, "f": fg, "w": wg}[alias]
        nat.check(L.gg_sample_accumulate(fg.ptr, wg.ptr, tgt.ptr, eg.ptr, qg.ptr, k + 1, n, s))
        out = tgt.read()
        for g, a in ((fg, "f"), (wg, "w")):
            if alias != a:
                g.unchanged()
    if alias is not None:
        og.unchanged()
    return out, eg.read(), qg.read()


def test_sampling_streams_past_the_wrap(nat):
    """n = 2^20 + 3: the pair kernels take a second grid-stride trip and end
    on an odd tail.  The residuals at the NORMAL_TOL bounds of
    test_gpu_posterior_sample.py, the accumulation after three draws, out ==
    w."""
    p = sample_problem(BIG)
    for noise in (False, True):
        r = residual_check(p, run_residual(nat, p, noise), noise)
        print("sample_residual%s n=%d: worst err/bound %.4f" % ("_noise" if noise else "", BIG, r))
    r = accumulate_check(p, *run_accumulate(nat, p))
    print("sample_accumulate n=%d, 3 draws: worst err/bound %.4f" % (BIG, r))
    accumulate_check(p, *run_accumulate(nat, p, alias="w"))


def test_sampling_mixed_alignment(nat):
    """Exactly one operand one double off a 16-byte boundary, in turn: the
    whole pass must leave the 16-byte lanes.  Each result inside the bounds of
    the all-aligned one; out == f and out == w."""
    p = sample_problem(1441)
    for noise in (False, True):
        for k in (0, 1, 2, 3) if noise else (0, 1, 3):
            offs = [0, 0, 0, 0]
            offs[k] = 1
            residual_check(p, run_residual(nat, p, noise, offs), noise)
        residual_check(p, run_residual(nat, p, noise), noise)
    for k in range(5):
        offs = [0] * 5
        offs[k] = 1
        accumulate_check(p, *run_accumulate(nat, p, offs))
    for alias in ("f", "w"):
        for off in (0, 1):
            accumulate_check(p, *run_accumulate(nat, p, (off, off, 0, 0, 0), alias))


def coeff_tables(ms):
    """Per-factor eigenvalues in [0.2, 3), the first of the largest factor
    slightly negative (the clamp), and their Kronecker product."""
    rng = np.random.default_rng(31 + sum(ms))
    lam = [rng.uniform(0.2, 3.0, m) for m in ms]
    lam[int(np.argmax(ms))][0] = -1e-9
    return lam, mr.kron_eigs(lam)


COEFF_SHAPES = [(1031, 1019, 1), (6,), (5, 1), (3, 2), (1, 1, 6)]


@pytest.mark.parametrize("ms", COEFF_SHAPES, ids=ids)
def test_coefficient_kernels_pair_decoding(nat, ms):
    """A last factor of order 1 (every pair straddles two runs), of order 2
    (none does), d = 1, and n = 1031 * 1019 past the wrap; yt and c aligned and
    each alone one double off.  The bounds of test_gpu_posterior_sample.py."""
    L, s = nat.lib(), nat.stream_ptr()
    lam, t = coeff_tables(ms)
    n, d = t.size, len(ms)
    assert t.min() < 0 and (ms != COEFF_SHAPES[0] or n > (1 << 20) + 2)
    m = nat.i64_array(ms)
    lg = Guard(sum(ms), np.concatenate(lam))
    yt = np.random.default_rng(2).standard_normal(n)
    z = ps.normal_stream(11, 4, n)
    S2 = 0.01
    refp = ps.posterior_coeffs(t, S2, yt, z)
    gain = np.sqrt(np.maximum(t, 0.0) * S2 / (t + S2))
    ref0 = ps.prior_coeffs(t, z)
    worst = 0.0
    for yoff, coff in ((0, 0), (1, 0), (0, 1)):
        yg, cg = Sent(n, yt, yoff), Sent(n, None, coff)
        nat.check(L.gg_kron_posterior_coeffs(d, m, lg.ptr, S2, yg.ptr, 11, 4, cg.ptr, s))
        err = np.abs(cg.read() - refp)
        bound = 1e-12 * np.abs(refp) + NORMAL_TOL * gain + 1e-300
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (ms, yoff, coff)
        yg.unchanged()
        if yoff:
            continue
        cg = Sent(n, None, coff)
        nat.check(L.gg_kron_prior_coeffs(d, m, lg.ptr, 11, 4, cg.ptr, s))
        got = cg.read()
        bound = 1e-12 * np.abs(ref0) + NORMAL_TOL * np.sqrt(np.maximum(t, 0.0))
        assert np.all(np.abs(got - ref0) <= bound), (ms, coff)
        assert np.all(got[t < 0] == 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.max(np.where(bound > 0, np.abs(got - ref0) / bound, 0.0))))
    lg.unchanged()
    print("coefficient kernels %s: worst err/bound %.4f" % (ms, worst))
