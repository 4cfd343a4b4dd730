"""The sharded section of include/gp_grief_amd.h at its edges, called through
ctypes exactly as a C caller would: gg_kron_dist_* (phases, push mode, the CG
prologue), gg_cgs_* (textbook and fused scalars in lockstep, the vector
kernels' edges, the done latch), gg_parity_fold and gg_shard0_fold.

All ranks are handles in one process and one thread, run one after the other;
the all-to-all is the reference's host permutation, the all-reduce a host sum
of the ranks' out_dev, push mode is gg_kron_dist_set_peers with plain pointers.
No CG is iterated to convergence: every call is compared with the long-double
reference step (tests/shard_abi_ref.py) applied to the device's own state from
before the call, so each bound is one step wide.

Guarded buffers (tests/abi_guard.py): payloads of exactly the documented size
between 64 NaN doubles, outputs and scratch pre-filled with NaN, guards and
inputs compared bit for bit; a refused call leaves everything untouched.

Bounds (derived in tests/shard_abi_ref.py, u = 2^-53; not tuned):
  matvec phases   c u mag, c = sum (q_k + 3) + 2 over the stages of the call
  dots            chain u sum |x_i y_i|
  x, r, p updates 4 u (|x| + |a p|); shift_dot's q + s p: 2 u (|q| + |s p|);
                  the fused r - a (q + s p): 6 u (|r| + |a| (|q| + |s p|));
                  the fused p_new also carries its beta's cancellation error
  parity fold     (2^K + 1) u scale sum |corner values|; shard0 bit for bit

Measured on MI355X (worst err / bound per case, printed by the tests):
  matvec phases, dense cases 0.11 .. 0.25 (the whole K x 0.004 .. 0.065),
  folded cases 0.07 .. 0.22 (K x 0.002 .. 0.005); 16-byte aligned and one
  double off alike
  textbook lockstep: p 0.27 .. 0.37, q 0.48 .. 0.49, x 0.26 .. 0.36,
  r 0.24 .. 0.38, dots 0.035 .. 0.052, phases 0.23 .. 0.25
  prologue cases: p 0.23 .. 0.41, q 0.50, x 0.28 .. 0.36, r 0.19 .. 0.30
  vector kernels alone: n = 1 .. 3 at most 0.09; n = 2 * 256 * 2048 + 3:
  dots 0.09, q 0.50, x 0.36, r 0.37
  fused lockstep: r 0.29 .. 0.32, p 0.23 .. 0.31, x 0.22 .. 0.24, phases
  0.23 .. 0.27, dots 0.04 .. 0.05, the prologue's sums 0.0002 .. 0.0024 (the
  any-order bound), closed state against the textbook recurrence below 5e-5
  of its it^2 kappa eps bound; the repair case r, p 0.08
  parity fold: forward 0.12 .. 0.57, inverse up to 0.50, sum of the ranks'
  contributions 0.04 .. 0.55 (world 1: 0); shard0 fold bit for bit"""
import contextlib
import ctypes

import numpy as np
import pytest

import kron_abi_ref as R
import shard_abi_ref as S

from abi_guard import Guard, bits

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
GG_OK, GG_ERR_VALUE = 0, -1
CASES = S.matvec_cases()


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


def vp(g, shift=0):
    """Pointer `shift` doubles into a Guard's payload."""
    return ctypes.c_void_p(g.ptr.value + 8 * int(shift))


def set_fold_env(monkeypatch, env):
    monkeypatch.delenv("GG_KRON_FOLD", raising=False)
    monkeypatch.delenv("GG_KRON_FOLD_MIN", raising=False)
    if env:
        monkeypatch.setenv(env[0], env[1])


def dist_create(nat, fs, world, rank):
    fs = [np.ascontiguousarray(F, dtype=np.float64) for F in fs]
    d = len(fs)
    ptrs = (ctypes.c_void_p * d)(*[F.ctypes.data for F in fs])
    out = ctypes.c_void_p()
    nat.check(nat.lib().gg_kron_dist_create(d, nat.i64_array([F.shape[0] for F in fs]), ptrs,
                                            world, rank, ctypes.byref(out)), "gg_kron_dist_create")
    return out


@contextlib.contextmanager
def dist(nat, fs, world):
    """The world's handles, made the way a C caller makes them."""
    hs = []
    try:
        for g in range(world):
            hs.append(dist_create(nat, fs, world, g))
        yield hs
    finally:
        import torch
        torch.cuda.synchronize()
        for h in hs:
            assert nat.lib().gg_kron_dist_destroy(h) == GG_OK


@contextlib.contextmanager
def cgs(nat, count=1):
    hs = []
    try:
        for _ in range(count):
            c = ctypes.c_void_p()
            nat.check(nat.lib().gg_cgs_create(ctypes.byref(c)), "gg_cgs_create")
            hs.append(c)
        yield hs
    finally:
        import torch
        torch.cuda.synchronize()
        for c in hs:
            assert nat.lib().gg_cgs_destroy(c) == GG_OK


def scalars_ptr(nat, c):
    p = ctypes.c_void_p()
    nat.check(nat.lib().gg_cgs_scalars(c, ctypes.byref(p)))
    assert p.value
    return p


def sizes(nat, D):
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    nat.check(nat.lib().gg_kron_dist_sizes(D, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def fold_mask_of(nat, D):
    v = ctypes.c_int64(-1)
    nat.check(nat.lib().gg_kron_dist_fold_mask(D, ctypes.byref(v)))
    return v.value


def status(nat, c):
    it, dn, rho, tol = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_double(-7.0), \
        ctypes.c_double(-7.0)
    nat.check(nat.lib().gg_cgs_status(c, ctypes.byref(it), ctypes.byref(dn), ctypes.byref(rho),
                                      ctypes.byref(tol), nat.stream_ptr()))
    return it.value, dn.value, rho.value, tol.value


def set_peers(nat, hs, xbufs):
    G = len(hs)
    ptrs = (ctypes.c_void_p * G)(*[b.ptr.value for b in xbufs])
    for g in range(G):
        nat.check(nat.lib().gg_kron_dist_set_peers(hs[g], xbufs[g].ptr, 0, None, None, ptrs),
                  "gg_kron_dist_set_peers")


def case_problem(m, G, mask):
    fs = S.case_factors(m, mask)
    x = R.vector(int(np.prod(m)), 5)
    return fs, x, [S.scatter(x, m, G, g) for g in range(G)]


class Ranks(object):
    """One sharded matvec over the world's handles, both modes, every buffer
    checked after every call (module docstring).  off: every operand `off`
    doubles past a 16-byte boundary."""

    def __init__(self, nat, hs, fs, mask, push, off, xbuf=None):
        self.nat, self.L, self.hs, self.fs, self.mask = nat, nat.lib(), hs, fs, mask
        self.G, self.push, self.off = len(hs), push, off
        self.m = [F.shape[0] for F in fs]
        self.nl = int(np.prod(self.m)) // self.G
        self.worst = 0.0
        for D in hs:
            assert sizes(nat, D) == (self.nl, self.nl)
            assert fold_mask_of(nat, D) == mask
        if push and xbuf is not None:
            self.xbuf = xbuf            # the peers are set already
        elif push:
            self.xbuf = [Guard(2 * self.nl, None, off) for _ in hs]
            set_peers(nat, hs, self.xbuf)

    def ratio(self, got, ref, bound):
        r = R.worst_ratio(got, ref, bound)
        self.worst = max(self.worst, r)
        return r

    def matvec(self, xs, cg=None):
        """xs: the ranks' Guards of x_local (p, updated in place, with cg =
        (r Guards, scalars pointers, reference prologue function)).  Returns
        the ranks' K x as host arrays (push mode: it also stays in the out
        halves of self.xbuf)."""
        nat, L, G, nl, fs, mask, off = self.nat, self.L, self.G, self.nl, self.fs, self.mask, \
            self.off
        st = nat.stream_ptr()
        if self.push:
            for b in self.xbuf:
                b.reset()
        sends, works, refs = [], [], []
        for g, D in enumerate(self.hs):
            send, work = Guard(nl, None, off), Guard(nl, None, off)
            r_ptr = cg[0][g].ptr if cg else None
            s_ptr = cg[1][g] if cg else None
            before = xs[g].read()
            r_before = cg[0][g].read() if cg else None
            if self.push:
                nat.check(L.gg_kron_dist_phase1_push(D, xs[g].ptr, send.ptr, work.ptr, r_ptr, s_ptr,
                                                     st), "gg_kron_dist_phase1_push")
            else:
                nat.check(L.gg_kron_dist_phase1(D, xs[g].ptr, send.ptr, work.ptr, r_ptr, s_ptr, st),
                          "gg_kron_dist_phase1")
            xin = xs[g].read()
            if cg:
                cg[2](g, before, xin)
                assert np.array_equal(bits(cg[0][g].read()), bits(r_before)), "r was written"
            else:
                assert np.array_equal(bits(xin), bits(before)), "x was written"
            ref, mag = S.phase1_ref(fs, G, xin, mask)
            refs.append((ref, S.phase1_bound(fs, xin, mag)))
            work.read()
            sends.append(send)
            works.append(work)
        if self.push:
            for s_ in sends:
                s_.read()          # scratch: its guards
            recv = [b.read()[:nl] for b in self.xbuf]
            want = S.exchange([r_[0] for r_ in refs])
            wb = S.exchange([r_[1] for r_ in refs])
            for g in range(G):
                assert self.ratio(recv[g], want[g], wb[g]) <= 1.0, ("phase1_push", g)
                assert np.all(np.isnan(self.xbuf[g].read()[nl:])), "out written by phase 1"
            refs2 = []
            for g, D in enumerate(self.hs):
                ref, mag = S.phase2_ref(fs, G, recv[g], mask)
                refs2.append((ref, S.phase2_bound(fs, recv[g], mag)))
                nat.check(L.gg_kron_dist_phase2_push(D, st), "gg_kron_dist_phase2_push")
            want = S.exchange([r_[0] for r_ in refs2])
            wb = S.exchange([r_[1] for r_ in refs2])
            outs = []
            for g in range(G):
                full = self.xbuf[g].read()
                assert np.array_equal(bits(full[:nl]), bits(recv[g])), "recv written by phase 2"
                assert self.ratio(full[nl:], want[g], wb[g]) <= 1.0, ("phase2_push", g)
                outs.append(full[nl:])
            return outs
        got = []
        for g in range(G):
            s_ = sends[g].read()
            assert self.ratio(s_, refs[g][0], refs[g][1]) <= 1.0, ("phase1", g)
            got.append(s_)
        recv = S.exchange(got)
        got = []
        for g, D in enumerate(self.hs):
            rg, send = Guard(nl, recv[g], off), Guard(nl, None, off)
            nat.check(L.gg_kron_dist_phase2(D, rg.ptr, send.ptr, st), "gg_kron_dist_phase2")
            rg.unchanged()
            ref, mag = S.phase2_ref(fs, G, recv[g], mask)
            s_ = send.read()
            assert self.ratio(s_, ref, S.phase2_bound(fs, recv[g], mag)) <= 1.0, ("phase2", g)
            got.append(s_)
        return S.exchange(got)


# ============================================================ a. matvec phases
@pytest.mark.parametrize("push", [0, 1], ids=["a2a", "push"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matvec_phases(nat, monkeypatch, case, push):
    name, m, G, env, mask = case
    set_fold_env(monkeypatch, env)
    fs, x, loc = case_problem(m, G, mask)
    full, fmag = R.matvec_ref(fs, x, False, 0.0, mask)
    fb = R.matvec_bound(fs, x, fmag)
    for off in (0, 1):
        with dist(nat, fs, G) as hs:
            rk = Ranks(nat, hs, fs, mask, push, off)
            xs = [Guard(rk.nl, loc[g], off) for g in range(G)]
            y = rk.matvec(xs)
            for g in range(G):
                xs[g].unchanged()
            whole = R.worst_ratio(S.gather(y, m), full, fb)
            print("shard matvec %s %s off=%d: phases err/bound %.4f, K x %.4f"
                  % (name, "push" if push else "a2a", off, rk.worst, whole))
            assert whole <= 1.0, (name, push, off, whole)


# ========================================= b. textbook scalars, in lockstep
def lockstep(nat, m, G, fs, mask, iters, push, off, shift=0.05):
    """`iters` textbook iterations, every call against the reference step on
    the device's own state.  Returns the worst ratios by kind."""
    L, st = nat.lib(), nat.stream_ptr()
    n = int(np.prod(m))
    b = R.vector(n, 9)
    loc = [S.scatter(b, m, G, g) for g in range(G)]
    worst = dict(p=0.0, q=0.0, x=0.0, r=0.0, dot=0.0, phases=0.0)

    def up(k, v):
        worst[k] = max(worst[k], v)
        assert v <= 1.0, (k, v)

    with dist(nat, fs, G) as hs, cgs(nat, G) as cs:
        rk = Ranks(nat, hs, fs, mask, push, off)
        nl = rk.nl
        scp = [scalars_ptr(nat, c) for c in cs]
        rg = [Guard(nl, loc[g], off) for g in range(G)]
        xg = [Guard(nl, np.zeros(nl), off) for g in range(G)]
        pg = [Guard(nl, np.zeros(nl), off) for g in range(G)]
        red = [Guard(1) for _ in range(G)]

        def allreduce():
            vals = [r_.read()[0] for r_ in red]
            s = float(np.sum(np.asarray(vals, dtype=np.float64)))
            for g in range(G):
                red[g] = Guard(1, [s])
            return s, vals

        # local_dot needs aligned vectors: r.r from an aligned copy
        for g in range(G):
            ra = Guard(nl, loc[g])
            nat.check(L.gg_cgs_local_dot(cs[g], ra.ptr, ra.ptr, nl, red[g].ptr, st))
            ref, mag = S.dot_ref(loc[g], loc[g])
            up("dot", R.worst_ratio(red[g].read(), ref, S.dot_bound(nl, 2, mag)))
            ra.unchanged()
        rr, _ = allreduce()
        sc = S.init_ref(None, rr, 1e-10, 0.0)
        for g in range(G):
            nat.check(L.gg_cgs_init(cs[g], red[g].ptr, 1e-10, 0.0, st))
            it, dn, rho, tol = status(nat, cs[g])
            assert (it, dn, rho) == (0, 0, rr) and abs(tol - sc["tol"]) <= 2 * U * sc["tol"]
        for itn in range(iters):
            def pro(g, before, after, sc=sc):
                pref, pmag = S.prologue_ref(sc, before, rg[g].read())
                if sc["first"]:
                    assert np.array_equal(bits(after), bits(rg[g].read())), "first: p = r"
                else:
                    assert not np.array_equal(bits(after), bits(before))
                    up("p", R.worst_ratio(after, pref, S.AXPY_C * U * pmag))
            q = rk.matvec(pg, cg=(rg, scp, pro))
            up("phases", rk.worst)
            lane = 1 if off else 2
            for g in range(G):
                p = pg[g].read()
                if push:      # q = the out half of the exchange buffer, in place
                    qptr, qbuf = vp(rk.xbuf[g], nl), rk.xbuf[g]
                    lane_q = 2 if (qptr.value % 16 == 0 and pg[g].ptr.value % 16 == 0) else 1
                else:
                    qbuf = Guard(nl, q[g], off)
                    qptr, lane_q = qbuf.ptr, lane
                qref, qmag = S.shift_dot_ref(sc, q[g], p, shift)
                nat.check(L.gg_cgs_shift_dot(cs[g], qptr, pg[g].ptr, nl, shift, red[g].ptr, st))
                qn = qbuf.read()[nl:] if push else qbuf.read()
                up("q", R.worst_ratio(qn, qref, 2 * U * qmag))
                ref, mag = S.dot_ref(p, qn)
                up("dot", R.worst_ratio(red[g].read(), ref, S.dot_bound(nl, lane_q, mag)))
                pg[g].read()
                q[g] = (qn, qptr, qbuf)     # qbuf: keeps the allocation alive
            pq, _ = allreduce()
            sc = S.alpha_ref(sc, pq)
            for g in range(G):
                nat.check(L.gg_cgs_alpha(cs[g], red[g].ptr, st))
                x0, r0, p = xg[g].read(), rg[g].read(), pg[g].read()
                qn, qptr, qbuf = q[g]
                xr, rref, mx, mr = S.update_ref(sc, x0, r0, p, qn)
                nat.check(L.gg_cgs_update(cs[g], xg[g].ptr, rg[g].ptr, pg[g].ptr, qptr, nl,
                                          red[g].ptr, st))
                x1, r1 = xg[g].read(), rg[g].read()
                up("x", R.worst_ratio(x1, xr, S.AXPY_C * U * mx))
                up("r", R.worst_ratio(r1, rref, S.AXPY_C * U * mr))
                assert np.array_equal(bits(pg[g].read()), bits(p))
                assert np.array_equal(bits(qbuf.read()[nl:] if push else qbuf.read()), bits(qn))
                la = 2 if all(v % 16 == 0 for v in (xg[g].ptr.value, rg[g].ptr.value,
                                                    pg[g].ptr.value, qptr.value)) else 1
                ref, mag = S.dot_ref(r1, r1)
                up("dot", R.worst_ratio(red[g].read(), ref, S.dot_bound(nl, la, mag)))
            rr, _ = allreduce()
            sc = S.rho_ref(sc, rr)
            for g in range(G):
                nat.check(L.gg_cgs_rho(cs[g], red[g].ptr, st))
                it, dn, rho, tol = status(nat, cs[g])
                assert (it, dn, rho) == (sc["iters"], int(sc["done"]), rr) and not sc["done"]
    return worst


@pytest.mark.parametrize("m,G", S.TEXTBOOK_SHAPES)
def test_textbook_lockstep(nat, monkeypatch, m, G):
    set_fold_env(monkeypatch, ("GG_KRON_FOLD", "0"))
    fs = R.toeplitz_factors(m)
    for push, off in ((0, 0), (1, 0), (1, 1)):
        w = lockstep(nat, m, G, fs, 0, 4, push, off)
        print("shard textbook %s w%d %s off=%d: %s" % (
            "x".join(map(str, m)), G, "push" if push else "a2a", off,
            " ".join("%s %.4f" % kv for kv in sorted(w.items()))))


@pytest.mark.parametrize("m,G,fmin", S.PROLOGUE_SHAPES)
@pytest.mark.parametrize("push", [0, 1], ids=["a2a", "push"])
def test_phase1_prologue(nat, monkeypatch, m, G, fmin, push):
    """Phase 1 with the CG prologue: first = 1 gives p = r bit for bit; after
    one full textbook step p = r + beta p inside the bound; nonsymmetric
    factors (the matvec need not be SPD for one step)."""
    folded = fmin is not None
    set_fold_env(monkeypatch, ("GG_KRON_FOLD_MIN", str(fmin)) if folded else ("GG_KRON_FOLD", "0"))
    mask = (1 << len(m)) - 1 if folded else 0
    fs = S.case_factors(m, mask)
    assert S.fold_mask(fs, fmin or 48, folded) == mask
    for off in (0, 1):
        w = lockstep(nat, m, G, fs, mask, 2, push, off, shift=3.0)
        print("shard prologue %s w%d %s off=%d: %s" % (
            "x".join(map(str, m)), G, "push" if push else "a2a", off,
            " ".join("%s %.4f" % kv for kv in sorted(w.items()))))


def live_cgs(nat, c, alpha_pq=3.0):
    """rho = 1, alpha = 1 / alpha_pq, not done."""
    L, st = nat.lib(), nat.stream_ptr()
    one, pq = Guard(1, [1.0]), Guard(1, [alpha_pq])
    nat.check(L.gg_cgs_init(c, one.ptr, 1e-12, 0.0, st))
    nat.check(L.gg_cgs_alpha(c, pq.ptr, st))
    assert status(nat, c)[:3] == (0, 0, 1.0)
    return S.alpha_ref(S.init_ref(None, 1.0, 1e-12, 0.0), alpha_pq)


BIG = 2 * 256 * 2048 + 3


def edge_vectors(n, k):
    """k seeded vectors of length n with a distinctive large value at 0,
    n - 2, n - 1 and at both kernels' grid-stride wrap indices."""
    out = []
    for j in range(k):
        v = R.vector(n, 40 + j).copy()
        for t, i in enumerate((0, 256 * 2048, 2 * 256 * 2048, n - 2, n - 1)):
            if 0 <= i < n:
                v[i] = (-1.0) ** t * 1e3 * (t + 1 + j)
        out.append(v)
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 3, BIG])
def test_vector_kernel_edges(nat, n):
    """local_dot, shift_dot and update alone at n = 0..3 and past the
    grid-stride wrap, every alignment combination the call accepts (a sample
    of them at the large n) and the ones local_dot refuses."""
    L, st = nat.lib(), nat.stream_ptr()
    x, r, p, q = edge_vectors(n, 4)
    worst = dict(dot=0.0, q=0.0, x=0.0, r=0.0)

    def up(k, v, what):
        worst[k] = max(worst[k], v)
        assert v <= 1.0, (k, v, what)

    with cgs(nat) as (c,):
        sc = live_cgs(nat, c)
        # local_dot: aligned only
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            a, b_, out = Guard(n, x, ox), Guard(n, p, oy), Guard(1)
            stt = L.gg_cgs_local_dot(c, a.ptr, b_.ptr, n, out.ptr, st)
            if ox or oy:
                assert stt == GG_ERR_VALUE
                out.unchanged()
            else:
                assert stt == GG_OK, nat.last_error()
                ref, mag = S.dot_ref(x, p)
                got = out.read()
                if n == 0:
                    assert bits(got)[0] == 0
                up("dot", R.worst_ratio(got, ref, S.dot_bound(n, 2, mag)), "local_dot")
            a.unchanged()
            b_.unchanged()
        combos2 = [(0, 0), (1, 0), (0, 1), (1, 1)]
        for oq, op in combos2:
            qg, pgd, out = Guard(n, q, oq), Guard(n, p, op), Guard(1)
            nat.check(L.gg_cgs_shift_dot(c, qg.ptr, pgd.ptr, n, 0.37, out.ptr, st))
            qref, qmag = S.shift_dot_ref(sc, q, p, 0.37)
            qn = qg.read()
            pgd.unchanged()
            up("q", R.worst_ratio(qn, qref, 2 * U * qmag), ("shift_dot", oq, op))
            ref, mag = S.dot_ref(p, qn)
            lane = 1 if (oq or op) else 2
            got = out.read()
            if n == 0:
                assert bits(got)[0] == 0
            up("dot", R.worst_ratio(got, ref, S.dot_bound(n, lane, mag)), ("shift_dot", oq, op))
        if n == BIG:
            combos4 = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 1), (1, 1, 1, 1)]
        else:
            combos4 = [tuple((i >> k) & 1 for k in range(4)) for i in range(16)]
        for offs in combos4:
            gs = [Guard(n, v, o) for v, o in zip((x, r, p, q), offs)]
            out = Guard(1)
            nat.check(L.gg_cgs_update(c, gs[0].ptr, gs[1].ptr, gs[2].ptr, gs[3].ptr, n, out.ptr, st))
            xr, rref, mx, mr = S.update_ref(sc, x, r, p, q)
            x1, r1 = gs[0].read(), gs[1].read()
            gs[2].unchanged()
            gs[3].unchanged()
            up("x", R.worst_ratio(x1, xr, S.AXPY_C * U * mx), ("update", offs))
            up("r", R.worst_ratio(r1, rref, S.AXPY_C * U * mr), ("update", offs))
            ref, mag = S.dot_ref(r1, r1)
            got = out.read()
            if n == 0:
                assert bits(got)[0] == 0
            up("dot", R.worst_ratio(got, ref, S.dot_bound(n, 1 if any(offs) else 2, mag)),
               ("update", offs))
        assert status(nat, c)[:3] == (0, 0, 1.0)
    print("shard vector edges n=%d: %s" % (n, " ".join("%s %.4f" % kv
                                                         for kv in sorted(worst.items()))))


# ============================================================ c. the done latch
LATCH = {
    "rhs0": (0.0, 1e-5, 0.0),
    "rr_nan": (float("nan"), 1e-5, 0.0),
    "rr_negative": (-1.0, 1e-5, 0.0),
    "atol_above_b": (4.0, 0.0, 2.5),
    "rho_mid_run": (4.0, 0.1, 0.0),
}


@pytest.mark.parametrize("name", sorted(LATCH))
def test_done_latch(nat, monkeypatch, name):
    """Once the latch is set, every gg_cgs_* step and a phase 1 with the
    prologue leave x, r, p, q bit for bit unchanged, the status frozen, and
    out_dev at the documented 0 (red_dev: five zeros)."""
    set_fold_env(monkeypatch, ("GG_KRON_FOLD", "0"))
    L, st = nat.lib(), nat.stream_ptr()
    m, G = (5, 7, 3), 1
    fs = S.case_factors(m, 0)
    rr0, rtol, atol = LATCH[name]
    with dist(nat, fs, G) as (D,), cgs(nat) as (c,):
        nl = sizes(nat, D)[0]
        for off in (0, 1):
            vecs = edge_vectors(nl, 4)
            xg, rg, pg, qg = [Guard(nl, v, off) for v in vecs]
            rrg = Guard(1, [rr0])
            nat.check(L.gg_cgs_init(c, rrg.ptr, rtol, atol, st))
            sc = S.init_ref(None, rr0, rtol, atol)
            if name == "rho_mid_run":
                assert status(nat, c)[:2] == (0, 0)
                pq, small = Guard(1, [8.0]), Guard(1, [0.01])
                nat.check(L.gg_cgs_alpha(c, pq.ptr, st))
                nat.check(L.gg_cgs_rho(c, small.ptr, st))
                sc = S.rho_ref(S.alpha_ref(sc, 8.0), 0.01)
            assert sc["done"]
            s0 = status(nat, c)
            assert s0[:2] == (sc["iters"], 1)
            assert bits([s0[2]])[0] == bits([sc["rho"]])[0]

            def frozen(what):
                for g_ in (xg, rg, pg, qg):
                    g_.unchanged()
                s1 = status(nat, c)
                assert s1[:2] == s0[:2] and np.array_equal(bits(s1[2:]), bits(s0[2:])), what

            out, other = Guard(1), Guard(1, [123.0])
            nat.check(L.gg_cgs_shift_dot(c, qg.ptr, pg.ptr, nl, 0.37, out.ptr, st))
            assert bits(out.read())[0] == 0
            frozen("shift_dot")
            nat.check(L.gg_cgs_alpha(c, other.ptr, st))
            frozen("alpha")
            out = Guard(1)
            nat.check(L.gg_cgs_update(c, xg.ptr, rg.ptr, pg.ptr, qg.ptr, nl, out.ptr, st))
            assert bits(out.read())[0] == 0
            frozen("update")
            nat.check(L.gg_cgs_rho(c, other.ptr, st))
            frozen("rho")
            send, work = Guard(nl, None, off), Guard(nl, None, off)
            nat.check(L.gg_kron_dist_phase1(D, pg.ptr, send.ptr, work.ptr, rg.ptr,
                                            scalars_ptr(nat, c), st))
            send.read()
            work.read()
            frozen("phase1 with the prologue")
            red5 = Guard(5, [1.0, 2.0, 3.0, 0.0, 4.0])
            nat.check(L.gg_cgs_fused_scalars(c, red5.ptr, pg.ptr, st))
            red5.unchanged()
            frozen("fused_scalars")
            out = Guard(1)
            nat.check(L.gg_cgs_fused_close(c, xg.ptr, rg.ptr, qg.ptr, pg.ptr, nl, S.half(nl), 0.37,
                                           out.ptr, st))
            assert bits(out.read())[0] == 0
            frozen("fused_close")
            nat.check(L.gg_cgs_fused_close_rho(c, other.ptr, st))
            frozen("fused_close_rho")
            other.unchanged()
            # local_dot is no CG step: it still computes
            out = Guard(1)
            a = Guard(nl, vecs[0])
            nat.check(L.gg_cgs_local_dot(c, a.ptr, a.ptr, nl, out.ptr, st))
            ref, mag = S.dot_ref(vecs[0], vecs[0])
            assert R.worst_ratio(out.read(), ref, S.dot_bound(nl, 2, mag)) <= 1.0
            frozen("local_dot")


# ============================================================ e. refusals
def test_create_and_peer_refusals(nat, monkeypatch):
    set_fold_env(monkeypatch, ("GG_KRON_FOLD", "0"))
    L, st = nat.lib(), nat.stream_ptr()
    i64 = nat.i64_array
    F4 = np.ascontiguousarray(S.case_factors((4, 4), 0)[0])
    F3 = np.ascontiguousarray(np.eye(3))
    F257 = np.ascontiguousarray(np.eye(257))
    SENT = 0x5A5A5A5A

    def refused(d, m, fs, world, rank, with_out=True, null_fs=False, null_m=False):
        ptrs = None if null_fs else (ctypes.c_void_p * len(fs))(
            *[None if F is None else F.ctypes.data for F in fs])
        out = ctypes.c_void_p(SENT)
        stt = L.gg_kron_dist_create(d, None if null_m else i64(m), ptrs, world, rank,
                                    ctypes.byref(out) if with_out else None)
        assert stt == GG_ERR_VALUE and out.value == SENT, (stt, out.value, m, world, rank)

    refused(1, [4], [F4], 1, 0)                       # d = 1
    refused(2, [4, 4], [F4, F4], 0, 0)                # world 0
    refused(2, [4, 4], [F4, F4], 2, 2)                # rank = world
    refused(2, [4, 4], [F4, F4], 2, -1)
    refused(2, [3, 4], [F3, F4], 2, 0)                # m_0 not divisible
    refused(2, [4, 3], [F4, F3], 2, 0)                # m_1 not divisible
    refused(2, [4, 257], [F4, F257], 1, 0)            # a factor of 257
    refused(2, [257, 4], [F257, F4], 1, 0)
    refused(2, [4, 0], [F4, F4], 1, 0)                # an empty factor
    refused(2, [4, 4], [F4, F4], 1, 0, with_out=False)
    refused(2, [4, 4], [F4, F4], 1, 0, null_fs=True)
    refused(2, [4, 4], [F4, F4], 1, 0, null_m=True)
    refused(2, [4, 4], [F4, None], 1, 0)              # NULL factors_host[1]
    assert L.gg_kron_dist_destroy(None) == GG_OK
    assert L.gg_cgs_destroy(None) == GG_OK
    assert L.gg_cgs_create(None) == GG_ERR_VALUE

    fs = S.case_factors((4, 4), 0)
    x = R.vector(16, 5)
    with dist(nat, fs, 2) as hs:
        nl = 8
        loc = [S.scatter(x, (4, 4), 2, g) for g in range(2)]
        xg, send, work = Guard(nl, loc[0]), Guard(nl), Guard(nl)
        xbuf = [Guard(2 * nl), Guard(2 * nl)]
        # push calls before set_peers
        assert L.gg_kron_dist_phase1_push(hs[0], xg.ptr, send.ptr, work.ptr, None, None,
                                          st) == GG_ERR_VALUE
        assert L.gg_kron_dist_phase2_push(hs[0], st) == GG_ERR_VALUE
        # set_peers without pointers, with a NULL peer, with a NULL own buffer
        assert L.gg_kron_dist_set_peers(hs[0], xbuf[0].ptr, 0, None, None, None) == GG_ERR_VALUE
        assert L.gg_kron_dist_set_peers(hs[0], xbuf[0].ptr, 1, None, None, None) == GG_ERR_VALUE
        half_ = (ctypes.c_void_p * 2)(xbuf[0].ptr.value, None)
        assert L.gg_kron_dist_set_peers(hs[0], xbuf[0].ptr, 0, None, None, half_) == GG_ERR_VALUE
        ptrs = (ctypes.c_void_p * 2)(xbuf[0].ptr.value, xbuf[1].ptr.value)
        assert L.gg_kron_dist_set_peers(hs[0], None, 0, None, None, ptrs) == GG_ERR_VALUE
        assert L.gg_kron_dist_phase2_push(hs[0], st) == GG_ERR_VALUE     # still unset
        set_peers(nat, hs, xbuf)
        assert L.gg_kron_dist_set_peers(hs[0], xbuf[0].ptr, 0, None, None, ptrs) == GG_ERR_VALUE
        assert "already" in nat.last_error()
        # phase 1: r without the scalars and the reverse; NULLs; phase 2 in place
        with cgs(nat) as (c,):
            scp = scalars_ptr(nat, c)
            for fn in (L.gg_kron_dist_phase1, L.gg_kron_dist_phase1_push):
                assert fn(hs[0], xg.ptr, send.ptr, work.ptr, xg.ptr, None, st) == GG_ERR_VALUE
                assert fn(hs[0], xg.ptr, send.ptr, work.ptr, None, scp, st) == GG_ERR_VALUE
                assert fn(hs[0], None, send.ptr, work.ptr, None, None, st) == GG_ERR_VALUE
                assert fn(hs[0], xg.ptr, None, work.ptr, None, None, st) == GG_ERR_VALUE
                assert fn(hs[0], xg.ptr, send.ptr, None, None, None, st) == GG_ERR_VALUE
                assert fn(None, xg.ptr, send.ptr, work.ptr, None, None, st) == GG_ERR_VALUE
            assert L.gg_kron_dist_phase2(hs[0], send.ptr, send.ptr, st) == GG_ERR_VALUE
            assert L.gg_kron_dist_phase2(hs[0], None, send.ptr, st) == GG_ERR_VALUE
            assert L.gg_kron_dist_phase2(hs[0], xg.ptr, None, st) == GG_ERR_VALUE
            # the fused phase 1 on d = 2 (needs d >= 4)
            assert L.gg_kron_dist_phase1_fused(hs[0], xg.ptr, send.ptr, send.ptr, work.ptr, xg.ptr,
                                               xg.ptr, xg.ptr, c, 0.1, 0, st) == GG_ERR_VALUE
        assert L.gg_kron_dist_sizes(None, None, None) == GG_ERR_VALUE
        assert L.gg_kron_dist_fold_mask(hs[0], None) == GG_ERR_VALUE
        nat.check(L.gg_kron_dist_sizes(hs[0], None, None))
        for g_ in (xg, send, work, xbuf[0], xbuf[1]):
            g_.unchanged()
        # two handles of different shapes alive at once, both usable afterwards
        f2, x2, loc2 = case_problem((5, 7, 3), 1, 0)
        with dist(nat, f2, 1) as h2:
            rk1 = Ranks(nat, hs, fs, 0, 1, 0, xbuf=xbuf)
            rk2 = Ranks(nat, h2, f2, 0, 0, 0)
            y2 = rk2.matvec([Guard(105, loc2[0])])
            y1 = rk1.matvec([Guard(nl, loc[g]) for g in range(2)])
            y2b = rk2.matvec([Guard(105, loc2[0])])
            assert np.array_equal(bits(y2[0]), bits(y2b[0]))
            ref, mag = R.matvec_ref(fs, x)
            assert R.worst_ratio(S.gather(y1, (4, 4)), ref, R.matvec_bound(fs, x, mag)) <= 1.0


def test_fused_refusals(nat, monkeypatch):
    """gg_kron_dist_phase1_fused and gg_cgs_fused_post / _close: every
    requirement met once, nothing written."""
    set_fold_env(monkeypatch, ("GG_KRON_FOLD_MIN", "8"))
    L, st = nat.lib(), nat.stream_ptr()

    def fused(D, c, bufs, push=0):
        po, pn, send, work, r, q, x = bufs
        return L.gg_kron_dist_phase1_fused(D, po.ptr, pn.ptr, send.ptr, work.ptr, r.ptr, q.ptr,
                                           x.ptr, c, 0.05, push, st)

    def buffers(nl, offs=(0,) * 7):
        v = R.vector(nl, 3)
        return [Guard(nl, v if i in (0, 4, 5, 6) else None, offs[i]) for i in range(7)]

    with cgs(nat) as (c,):
        one = Guard(1, [1.0])
        nat.check(L.gg_cgs_init(c, one.ptr, 1e-12, 0.0, st))
        # d = 3
        with dist(nat, R.toeplitz_factors((4, 8, 8)), 2) as (D, _):
            assert fold_mask_of(nat, D) == 0b110
            bufs = buffers(128)
            assert fused(D, c, bufs) == GG_ERR_VALUE
            [b.unchanged() for b in bufs]
        # an unfolded factor (order 4 < 8)
        with dist(nat, R.toeplitz_factors((4, 8, 4, 8)), 2) as (D, _):
            assert fold_mask_of(nat, D) == 0b1010
            bufs = buffers(512)
            assert fused(D, c, bufs) == GG_ERR_VALUE
            [b.unchanged() for b in bufs]
        # odd n_local
        with dist(nat, R.toeplitz_factors((3, 3, 9, 9)), 3) as hs:
            assert fold_mask_of(nat, hs[0]) == 0b1100 and sizes(nat, hs[0])[0] == 243
            bufs = buffers(243)
            assert fused(hs[0], c, bufs) == GG_ERR_VALUE
            [b.unchanged() for b in bufs]
        # the same with every factor 1..d-1 folded, so the length check itself is met
        with dist(nat, R.toeplitz_factors((3, 9, 9, 9)), 3) as hs:
            assert fold_mask_of(nat, hs[0]) == 0b1110 and sizes(nat, hs[0])[0] == 729
            bufs = buffers(729)
            assert fused(hs[0], c, bufs) == GG_ERR_VALUE
            assert "even-length" in nat.last_error()
            [b.unchanged() for b in bufs]
        # misaligned x or p_new, push without peers, NULLs; fused_post first
        with dist(nat, R.toeplitz_factors((4, 8, 8, 8)), 2) as (D, _):
            assert fold_mask_of(nat, D) == 0b1110
            nl = 1024
            for offs in ((0, 1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 1)):
                bufs = buffers(nl, offs)
                assert fused(D, c, bufs) == GG_ERR_VALUE
                [b.unchanged() for b in bufs]
            bufs = buffers(nl)
            assert fused(D, c, bufs, push=1) == GG_ERR_VALUE
            assert L.gg_kron_dist_phase1_fused(D, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                                               bufs[3].ptr, bufs[4].ptr, bufs[5].ptr, bufs[6].ptr,
                                               None, 0.05, 0, st) == GG_ERR_VALUE
            red = Guard(5)
            assert L.gg_cgs_fused_post(c, bufs[5].ptr, bufs[0].ptr, nl, 0.05, red.ptr,
                                       st) == GG_ERR_VALUE
            assert "fused phase 1" in nat.last_error()
            red.unchanged()
            [b.unchanged() for b in bufs]
            # one accepted fused phase 1, then fused_post's own requirements
            nat.check(fused(D, c, bufs), "gg_kron_dist_phase1_fused")
            import torch
            torch.cuda.synchronize()
            qg, pgd = Guard(nl, R.vector(nl, 4)), Guard(nl, R.vector(nl, 5))
            q1, p1 = Guard(nl, R.vector(nl, 4), 1), Guard(nl, R.vector(nl, 5), 1)
            post = L.gg_cgs_fused_post
            assert post(c, qg.ptr, pgd.ptr, nl - 1, 0.05, red.ptr, st) == GG_ERR_VALUE   # odd n
            assert post(c, qg.ptr, pgd.ptr, 0, 0.05, red.ptr, st) == GG_ERR_VALUE
            assert post(c, q1.ptr, pgd.ptr, nl, 0.05, red.ptr, st) == GG_ERR_VALUE      # misaligned
            assert post(c, qg.ptr, p1.ptr, nl, 0.05, red.ptr, st) == GG_ERR_VALUE
            assert post(c, qg.ptr, pgd.ptr, nl, 0.05, None, st) == GG_ERR_VALUE
            red.unchanged()
            nat.check(post(c, qg.ptr, pgd.ptr, nl, 0.05, red.ptr, st), "gg_cgs_fused_post")
            got = red.read()
            pq, qq, mpq, mqq, _ = S.fused_post_ref(qg.read(), pgd.read(), 0.05)
            assert bits(got)[3] == 0
            assert R.worst_ratio(got[2], pq, S.dot_bound(nl, 2, mpq, 1)) <= 1.0
            assert R.worst_ratio(got[4], qq, S.dot_bound(nl, 2, mqq, 2)) <= 1.0
            # latched: a fused phase 1 touches nothing, a skipped fused_post
            # writes five zeros
            zero = Guard(1, [0.0])
            nat.check(L.gg_cgs_init(c, zero.ptr, 1e-12, 0.0, st))
            assert status(nat, c)[:2] == (0, 1)
            bufs = buffers(nl)
            nat.check(fused(D, c, bufs), "gg_kron_dist_phase1_fused, latched")
            [b.unchanged() for b in bufs]
            red = Guard(5)
            nat.check(post(c, qg.ptr, pgd.ptr, nl, 0.05, red.ptr, st), "gg_cgs_fused_post, latched")
            assert np.all(bits(red.read()) == 0)
            qg.unchanged()
            pgd.unchanged()


def test_cgs_refusals(nat):
    """Negative n, half out of range, bad tolerances, NULLs: GG_ERR_VALUE,
    nothing written, the handle usable afterwards."""
    L, st = nat.lib(), nat.stream_ptr()
    n = 5
    x, r, p, q = edge_vectors(n, 4)
    with cgs(nat) as (c,):
        sc = live_cgs(nat, c)
        s0 = status(nat, c)
        xg, rg, pg, qg, out = Guard(n, x), Guard(n, r), Guard(n, p), Guard(n, q), Guard(1, [7.0])
        for neg in (-1, -2, -5):
            assert L.gg_cgs_local_dot(c, xg.ptr, pg.ptr, neg, out.ptr, st) == GG_ERR_VALUE
            assert L.gg_cgs_shift_dot(c, qg.ptr, pg.ptr, neg, 0.1, out.ptr, st) == GG_ERR_VALUE
            assert L.gg_cgs_update(c, xg.ptr, rg.ptr, pg.ptr, qg.ptr, neg, out.ptr,
                                   st) == GG_ERR_VALUE
            assert L.gg_cgs_fused_close(c, xg.ptr, rg.ptr, qg.ptr, pg.ptr, neg, 0, 0.1, out.ptr,
                                        st) == GG_ERR_VALUE
            assert L.gg_cgs_fused_close(c, xg.ptr, rg.ptr, qg.ptr, pg.ptr, neg, neg, 0.1, out.ptr,
                                        st) == GG_ERR_VALUE
        for half_ in (-1, n + 1):
            assert L.gg_cgs_fused_close(c, xg.ptr, rg.ptr, qg.ptr, pg.ptr, n, half_, 0.1, out.ptr,
                                        st) == GG_ERR_VALUE
        for rtol, atol in ((float("nan"), 0.0), (0.0, float("nan")), (-1e-3, 0.0), (0.0, -1.0)):
            assert L.gg_cgs_init(c, out.ptr, rtol, atol, st) == GG_ERR_VALUE
        assert L.gg_cgs_init(c, None, 1e-5, 0.0, st) == GG_ERR_VALUE
        assert L.gg_cgs_init(None, out.ptr, 1e-5, 0.0, st) == GG_ERR_VALUE
        assert L.gg_cgs_local_dot(c, None, pg.ptr, n, out.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_local_dot(c, xg.ptr, pg.ptr, n, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_shift_dot(c, None, pg.ptr, n, 0.1, out.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_shift_dot(None, qg.ptr, pg.ptr, n, 0.1, out.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_update(c, xg.ptr, rg.ptr, pg.ptr, None, n, out.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_update(c, xg.ptr, rg.ptr, pg.ptr, qg.ptr, n, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_alpha(c, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_rho(c, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_rho(None, out.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_fused_scalars(c, None, pg.ptr, st) == GG_ERR_VALUE
        assert L.gg_cgs_fused_scalars(c, out.ptr, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_fused_close_rho(c, None, st) == GG_ERR_VALUE
        assert L.gg_cgs_scalars(c, None) == GG_ERR_VALUE
        assert L.gg_cgs_status(None, None, None, None, None, st) == GG_ERR_VALUE
        nat.check(L.gg_cgs_status(c, None, None, None, None, st), "status, all outputs NULL")
        for g_ in (xg, rg, pg, qg, out):
            g_.unchanged()
        assert status(nat, c) == s0
        # still usable
        nat.check(L.gg_cgs_update(c, xg.ptr, rg.ptr, pg.ptr, qg.ptr, n, out.ptr, st))
        xr, rref, mx, mr = S.update_ref(sc, x, r, p, q)
        assert R.worst_ratio(xg.read(), xr, S.AXPY_C * U * mx) <= 1.0
        assert R.worst_ratio(rg.read(), rref, S.AXPY_C * U * mr) <= 1.0


# ================================================================== f. folds
def cu_count():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def parity_cases():
    wrap = 256 * 16 * cu_count()
    # n_local just above the grid: m = (2, 2, w) sharded on axis 0, w odd
    w = wrap // 2 + 3
    return [("world1", (5, 7, 3), 1), ("K_eq_d", (2, 4), 4), ("order2", (2, 6, 3), 2),
            ("K1", (4, 5), 2), ("K3", (4, 2, 6, 3), 8), ("d12", (2,) * 12, 8),
            ("wrap", (2, 2, w), 2)]


def test_parity_fold(nat):
    """Every rank, forward and inverse, against the long-double reference; the
    inverse writes every element of a NaN-filled out and the ranks'
    contributions sum to x."""
    L, st = nat.lib(), nat.stream_ptr()
    for name, m, G in parity_cases():
        n = int(np.prod(m))
        nl = n // G
        if name == "wrap":
            assert nl > 256 * 16 * cu_count()
        x = R.vector(n, 21)
        xg = Guard(n, x)
        total = np.zeros(n, dtype=LD)
        tb = np.zeros(n, dtype=LD)
        wf = wi = 0.0
        for g in range(G):
            lg = Guard(nl)
            nat.check(L.gg_parity_fold(len(m), nat.i64_array(m), G, g, 0, xg.ptr, lg.ptr, st),
                      "gg_parity_fold")
            loc = lg.read()
            ref, bound = S.parity_fold_ref(x, m, G, g)
            wf = max(wf, R.worst_ratio(loc, ref, bound))
            lg2, og = Guard(nl, loc), Guard(n)
            nat.check(L.gg_parity_fold(len(m), nat.i64_array(m), G, g, 1, lg2.ptr, og.ptr, st),
                      "gg_parity_fold inverse")
            con = og.read()
            lg2.unchanged()
            assert not np.any(np.isnan(con)), "an element of out was not written"
            cref, cb = S.parity_unfold_ref(loc, m, G, g)
            wi = max(wi, R.worst_ratio(con, cref, cb))
            total += con.astype(LD)
            # the forward bound, spread by P_g^T like the block itself
            tb += cb + np.abs(S.parity_unfold_ref(bound, m, G, g)[0])
        xg.unchanged()
        # the sum of the contributions: each within its bound of P_g^T of a
        # block that is within the fold bound of P_g x, and sum_g P_g^T P_g = I
        ws = R.worst_ratio(total, x, tb + 2.0 ** -60 * G * np.abs(x))
        print("shard parity fold %s: forward %.4f inverse %.4f sum %.4f" % (name, wf, wi, ws))
        assert wf <= 1.0 and wi <= 1.0 and ws <= 1.0, (name, wf, wi, ws)


def test_shard0_fold(nat):
    """Bit for bit, both directions; the inverse leaves the other ranks'
    elements (and NaN) untouched; s0 = 1 and the grid-stride wrap."""
    L, st = nat.lib(), nat.stream_ptr()
    wrap = 256 * 16 * cu_count()
    for m, G in (((6, 5, 3), 3), ((4, 7), 4), ((5, 3), 1), ((2, wrap + 5), 2),
                 ((3, 1, 4), 3)):
        n = int(np.prod(m))
        nl = n // G
        assert nl > wrap or n < 100
        x = R.vector(n, 22)
        xg, og = Guard(n, x), Guard(n)
        seen = np.zeros(n, dtype=bool)
        for g in range(G):
            lg = Guard(nl)
            nat.check(L.gg_shard0_fold(len(m), nat.i64_array(m), G, g, 0, xg.ptr, lg.ptr, st))
            loc = lg.read()
            assert np.array_equal(bits(loc), bits(S.shard0_ref(x, m, G, g)))
            before = og.read()
            lg2 = Guard(nl, loc)
            nat.check(L.gg_shard0_fold(len(m), nat.i64_array(m), G, g, 1, lg2.ptr, og.ptr, st))
            after = og.read()
            pos = S.shard0_positions(m, G, g)
            assert not np.any(seen[pos])
            seen[pos] = True
            assert np.array_equal(bits(after[pos]), bits(x[pos]))
            rest = np.ones(n, dtype=bool)
            rest[pos] = False
            assert np.array_equal(bits(after[rest]), bits(before[rest]))
            lg2.unchanged()
        assert np.all(seen) and np.array_equal(bits(og.read()), bits(x))
        xg.unchanged()


def test_fold_refusals(nat):
    L, st = nat.lib(), nat.stream_ptr()
    i64 = nat.i64_array
    xg, og = Guard(64, R.vector(64, 1)), Guard(64)

    def par(d, m, world, rank, inv=0, a=xg, b=og):
        return L.gg_parity_fold(d, i64(m) if m is not None else None, world, rank, inv,
                                a.ptr if a else None, b.ptr if b else None, st)

    def sh0(d, m, world, rank, inv=0, a=xg, b=og):
        return L.gg_shard0_fold(d, i64(m) if m is not None else None, world, rank, inv,
                                a.ptr if a else None, b.ptr if b else None, st)

    assert par(13, [2] * 13, 2, 0) == GG_ERR_VALUE             # d = 13
    assert par(0, [2], 1, 0) == GG_ERR_VALUE
    assert par(2, [6, 4], 3, 0) == GG_ERR_VALUE                # world 3
    assert par(2, [6, 4], 0, 0) == GG_ERR_VALUE
    assert par(2, [3, 4], 2, 0) == GG_ERR_VALUE                # an odd sharded order
    assert par(2, [4, 3], 4, 0) == GG_ERR_VALUE
    assert par(2, [4, 4], 8, 0) == GG_ERR_VALUE                # K > d
    assert par(2, [4, 4], 2, 2) == GG_ERR_VALUE                # rank = world
    assert par(2, [4, 4], 2, -1) == GG_ERR_VALUE
    assert par(2, [4, 0], 2, 0) == GG_ERR_VALUE                # an order below 1
    assert par(2, [0, 4], 2, 0) == GG_ERR_VALUE
    assert par(2, [4, -4], 2, 0) == GG_ERR_VALUE
    assert par(2, None, 2, 0) == GG_ERR_VALUE
    assert par(2, [4, 4], 2, 0, a=None) == GG_ERR_VALUE
    assert par(2, [4, 4], 2, 0, b=None) == GG_ERR_VALUE
    assert sh0(0, [4], 1, 0) == GG_ERR_VALUE
    assert sh0(2, [4, 4], 0, 0) == GG_ERR_VALUE
    assert sh0(2, [4, 4], 2, 2) == GG_ERR_VALUE                # rank = world
    assert sh0(2, [4, 4], 2, -1) == GG_ERR_VALUE
    assert sh0(2, [4, 4], 3, 0) == GG_ERR_VALUE                # m_0 % world != 0
    assert sh0(2, [4, 0], 2, 0) == GG_ERR_VALUE                # an order below 1, any position
    assert sh0(3, [4, 4, -1], 2, 0) == GG_ERR_VALUE
    assert sh0(2, [0, 4], 2, 0) == GG_ERR_VALUE
    assert sh0(2, [-4, 4], 2, 0) == GG_ERR_VALUE
    assert sh0(2, None, 2, 0) == GG_ERR_VALUE
    assert sh0(2, [4, 4], 2, 0, a=None) == GG_ERR_VALUE
    assert sh0(2, [4, 4], 2, 0, b=None) == GG_ERR_VALUE
    xg.unchanged()
    og.unchanged()
    nat.check(sh0(2, [4, 4], 2, 1))
    assert np.array_equal(bits(og.read()[:8]), bits(S.shard0_ref(xg.read()[:16], (4, 4), 2, 1)))


# ========================================= d. the fused recurrence, in lockstep
def textbook_ld(fs, b, shift, iters):
    """`iters` steps of the textbook CG in long double (x_0 = 0): (x, r)."""
    b = np.asarray(b, dtype=LD)
    x, r = np.zeros_like(b), b.copy()
    p, rho = r.copy(), r.dot(r)
    for _ in range(iters):
        q = R.matvec_ref(fs, p)[0] + LD(shift) * p
        a = rho / p.dot(q)
        x, r = x + a * p, r - a * q
        rho, rho0 = r.dot(r), rho
        p = r + (rho / rho0) * p
    return x, r


def fused_lockstep(nat, m, G, push, shift=0.05, iters=6, close_after=(3, 6), b=None,
                   expect_repair_at=None):
    """The fused sharded recurrence call by call (module docstring); returns
    the worst ratios by kind."""
    L, st = nat.lib(), nat.stream_ptr()
    fs = R.toeplitz_factors(m)
    n = int(np.prod(m))
    b = R.vector(n, 9) if b is None else b
    loc = [S.scatter(b, m, G, g) for g in range(G)]
    mask = S.fold_mask(fs, 8)
    assert mask & ~1 == ((1 << len(m)) - 1) & ~1 and S.lean_flags(m, G) == S.FUSED_LEAN[tuple(m)]
    worst = dict(r=0.0, p=0.0, x=0.0, phases=0.0, red=0.0, dot=0.0, close=0.0)

    def up(k, v, what=None):
        worst[k] = max(worst[k], v)
        assert v <= 1.0, (k, v, what)

    with dist(nat, fs, G) as hs, cgs(nat, G) as cs:
        nl = sizes(nat, hs[0])[0]
        H = S.half(nl)
        for D in hs:
            assert fold_mask_of(nat, D) == mask
        xbuf = [Guard(2 * nl) for _ in range(G)] if push else None
        if push:
            set_peers(nat, hs, xbuf)
            import torch
            for g in range(G):      # q_old of the first prologue: zero (not pending)
                xbuf[g].d[xbuf[g].lo + nl:xbuf[g].lo + 2 * nl] = 0.0
            torch.cuda.synchronize()
        rg = [Guard(nl, loc[g]) for g in range(G)]
        xg = [Guard(nl, np.zeros(nl)) for g in range(G)]
        qg = [Guard(nl, np.zeros(nl)) for g in range(G)]
        pb = [[Guard(nl, np.zeros(nl)) for _ in range(4)] for g in range(G)]
        red1 = [Guard(1) for _ in range(G)]

        def qread(g):
            return xbuf[g].read()[nl:] if push else qg[g].read()

        def qptr(g):
            return vp(xbuf[g], nl) if push else qg[g].ptr

        for g in range(G):
            nat.check(L.gg_cgs_local_dot(cs[g], rg[g].ptr, rg[g].ptr, nl, red1[g].ptr, st))
        rr = float(np.sum(np.asarray([r_.read()[0] for r_ in red1], dtype=np.float64)))
        sc = S.init_ref(None, rr, 1e-12, 0.0)
        for g in range(G):
            red1[g] = Guard(1, [rr])
            nat.check(L.gg_cgs_init(cs[g], red1[g].ptr, 1e-12, 0.0, st))
        closed = 0
        for it in range(1, iters + 1):
            pro, sends = [], []
            for g, D in enumerate(hs):
                p_old, p_new = pb[g][0], pb[g][1]
                vecs = {j: pb[g][j].read() for j in range(4)}   # direction ids: slots of pb
                po, r0, q0, x0 = p_old.read(), rg[g].read(), qread(g), xg[g].read()
                ref = S.fused_prologue_ref(sc, po, r0, q0, x0, shift, vecs)
                send, work = Guard(nl), Guard(nl)
                nat.check(L.gg_kron_dist_phase1_fused(D, p_old.ptr, p_new.ptr, send.ptr, work.ptr,
                                                      rg[g].ptr, qptr(g), xg[g].ptr, cs[g], shift,
                                                      push, st), "gg_kron_dist_phase1_fused")
                r1, pn, x1 = rg[g].read(), p_new.read(), xg[g].read()
                p_old.read()
                work.read()
                up("r", R.worst_ratio(r1, ref["r"], ref["b_r"]), (it, g))
                up("p", R.worst_ratio(pn, ref["p_new"], ref["b_p"]), (it, g))
                up("x", R.worst_ratio(x1, ref["x"], ref["b_x"]), (it, g))
                if expect_repair_at is not None and it == expect_repair_at + 1:
                    assert sc["repair"] and sc["beta"] == 0
                    assert np.array_equal(bits(pn), bits(r1 + 0.0)), "repair: beta = 0, p = r"
                assert np.array_equal(bits(qread(g)), bits(q0)), "q_old was written"
                sref, smag = S.phase1_ref(fs, G, pn, mask)
                sends.append((send, sref, S.phase1_bound(fs, pn, smag)))
                # the prologue's partial sums, on the device's own vectors
                qe = np.asarray(q0, dtype=LD) + LD(shift) * np.asarray(po, dtype=LD)
                pro.append((S.dot_ref(r1, r1), S.dot_ref(pn, qe)))
            if push:
                recv = [xb.read()[:nl] for xb in xbuf]
                want, wb = S.exchange([s_[1] for s_ in sends]), S.exchange([s_[2] for s_ in sends])
                for g in range(G):
                    sends[g][0].read()
                    up("phases", R.worst_ratio(recv[g], want[g], wb[g]), ("phase1 push", it, g))
                refs2 = []
                for g, D in enumerate(hs):
                    ref2, mag2 = S.phase2_ref(fs, G, recv[g], mask)
                    refs2.append((ref2, S.phase2_bound(fs, recv[g], mag2)))
                    nat.check(L.gg_kron_dist_phase2_push(D, st), "gg_kron_dist_phase2_push")
                want, wb = S.exchange([r_[0] for r_ in refs2]), S.exchange([r_[1] for r_ in refs2])
                for g in range(G):
                    up("phases", R.worst_ratio(qread(g), want[g], wb[g]), ("phase2 push", it, g))
            else:
                got = []
                for g in range(G):
                    s_ = sends[g][0].read()
                    up("phases", R.worst_ratio(s_, sends[g][1], sends[g][2]), ("phase1", it, g))
                    got.append(s_)
                recv = S.exchange(got)
                got = []
                for g, D in enumerate(hs):
                    rcv, send = Guard(nl, recv[g]), Guard(nl)
                    nat.check(L.gg_kron_dist_phase2(D, rcv.ptr, send.ptr, st))
                    ref2, mag2 = S.phase2_ref(fs, G, recv[g], mask)
                    s_ = send.read()
                    up("phases", R.worst_ratio(s_, ref2, S.phase2_bound(fs, recv[g], mag2)),
                       ("phase2", it, g))
                    got.append(s_)
                for g, v in enumerate(S.exchange(got)):
                    qg[g] = Guard(nl, v)
            red = np.zeros(5)
            reds = []
            for g in range(G):
                p_new = pb[g][1]
                rd = Guard(5)
                nat.check(L.gg_cgs_fused_post(cs[g], qptr(g), p_new.ptr, nl, shift, rd.ptr, st),
                          "gg_cgs_fused_post")
                got = rd.read()
                q1, pn = qread(g), p_new.read()
                pq, qq, mpq, mqq, _ = S.fused_post_ref(q1, pn, shift)
                (rr_, mrr), (pqo, mpqo) = pro[g]
                assert bits(got)[3] == 0, "red[3] must be +0.0"
                # the prologue's sums run inside the mode product, in an order
                # this file does not restate: the any-order bound, n terms
                # (r.r only where the prologue applied a pending update, p.q_old
                # not on the first step: +0.0 otherwise, as the header says)
                if sc["pending"]:
                    up("red", R.worst_ratio(got[0], rr_, (nl + 1) * U * mrr), ("rr", it, g))
                else:
                    assert bits(got)[0] == 0, ("rr, nothing pending", it, g)
                if not sc["first"]:
                    up("red", R.worst_ratio(got[1], pqo, (nl + 2) * U * mpqo), ("pqo", it, g))
                else:
                    assert bits(got)[1] == 0, ("pqo, first step", it, g)
                up("dot", R.worst_ratio(got[2], pq, S.dot_bound(nl, 2, mpq, 1)), ("pq", it, g))
                up("dot", R.worst_ratio(got[4], qq, S.dot_bound(nl, 2, mqq, 2)), ("qq", it, g))
                reds.append(got)
            red = np.sum(np.asarray(reds, dtype=np.float64), axis=0)
            red[3] = 0.0
            sc = S.fused_scalars_ref(sc, red, 1)
            for g in range(G):
                rd = Guard(5, red)
                nat.check(L.gg_cgs_fused_scalars(cs[g], rd.ptr, pb[g][1].ptr, st))
                rd.unchanged()
                pb[g][0], pb[g][1], pb[g][2], pb[g][3] = pb[g][1], pb[g][3], pb[g][0], pb[g][2]
            # the reference's direction ids are slots of pb, rotated with it
            rot = {1: 0, 3: 1, 0: 2, 2: 3}
            sc["xp"] = [None if v is None else rot[v] for v in sc["xp"]]
            sc["xsp"] = None if sc["xsp"] is None else rot[sc["xsp"]]
            assert expect_repair_at is not None or not sc["done"]
            if it in close_after:
                outs = []
                for g in range(G):
                    vecs = {j: pb[g][j].read() for j in range(4)}
                    x0, r0, q0, p0 = xg[g].read(), rg[g].read(), qread(g), pb[g][0].read()
                    sc2, xr, rref, bx, br = S.fused_close_ref(sc, x0, r0, q0, p0, shift, vecs)
                    out = Guard(1)
                    nat.check(L.gg_cgs_fused_close(cs[g], xg[g].ptr, rg[g].ptr, qptr(g),
                                                   pb[g][0].ptr, nl, H, shift, out.ptr, st),
                              "gg_cgs_fused_close")
                    x1, r1 = xg[g].read(), rg[g].read()
                    up("x", R.worst_ratio(x1, xr, bx), ("close", it, g))
                    up("r", R.worst_ratio(r1, rref, br), ("close", it, g))
                    assert np.array_equal(bits(qread(g)), bits(q0))
                    ref, mag = S.dot_ref(r1, r1)
                    up("dot", R.worst_ratio(out.read(), ref, S.dot_bound(nl, 1, mag)), ("close rr", g))
                    outs.append(out.read()[0])
                rr = float(np.sum(np.asarray(outs, dtype=np.float64)))
                sc = S.fused_close_rho_ref(sc2, rr)
                for g in range(G):
                    o = Guard(1, [rr])
                    nat.check(L.gg_cgs_fused_close_rho(cs[g], o.ptr, st))
                    assert status(nat, cs[g])[:3] == (sc["iters"], int(sc["done"]), rr)
                assert sc["iters"] == it and not sc["pending"]
                closed += 1
                # against the textbook recurrence of the same iterations: each
                # iteration's vectors carry a relative error of at most
                # eps = (c + 16) u (the one-step bounds above); a perturbation
                # of r or p is carried by the later iterations with a gain of
                # at most kappa(A), and `it` of them accumulate over at most
                # `it` steps:  it^2 kappa eps, normwise
                lam = [np.linalg.eigvalsh(F) for F in fs]
                hi = float(np.prod([l[-1] for l in lam])) + shift
                lo = float(np.prod([l[0] for l in lam])) + shift
                eps = (R.matvec_c(fs) + 16) * U
                xt, rt = textbook_ld(fs, b, shift, it)
                xd = S.gather([v.read() for v in xg], m)
                rd_ = S.gather([v.read() for v in rg], m)
                nx = float(np.sqrt(np.sum((xd - xt) ** 2)) / np.sqrt(np.sum(xt ** 2)))
                nr = float(np.sqrt(np.sum((rd_ - rt) ** 2)) / np.sqrt(np.sum(xt ** 2)) / hi)
                bound = it * it * (hi / lo) * eps
                up("close", nx / bound, ("x vs textbook", it))
                up("close", nr / bound, ("r vs textbook", it))
        assert closed == len([c for c in close_after if c <= iters])
    return worst


@pytest.mark.parametrize("push", [0, 1], ids=["a2a", "push"])
@pytest.mark.parametrize("m,G", S.FUSED_SHAPES)
def test_fused_lockstep(nat, monkeypatch, m, G, push):
    set_fold_env(monkeypatch, ("GG_KRON_FOLD_MIN", "8"))
    w = fused_lockstep(nat, m, G, push)
    print("shard fused %s w%d %s: %s" % ("x".join(map(str, m)), G, "push" if push else "a2a",
                                        " ".join("%s %.3g" % kv for kv in sorted(w.items()))))


def test_fused_repair_branch(nat, monkeypatch):
    """An rhs along an eigenvector: |r_1|^2 cancels in the expansion, the
    scalars ask for the repair, and the next prologue runs with beta = 0."""
    set_fold_env(monkeypatch, ("GG_KRON_FOLD_MIN", "8"))
    m, G = (4, 8, 10, 12), 2
    fs = R.toeplitz_factors(m)
    v = np.ones(1)
    for k, F in enumerate(fs):
        v = np.kron(v, np.linalg.eigh(F)[1][:, (k + 1) % F.shape[0]])
    w = fused_lockstep(nat, m, G, 0, iters=2, close_after=(), b=v / np.linalg.norm(v),
                       expect_repair_at=1)
    print("shard fused repair: %s" % " ".join("%s %.4f" % kv for kv in sorted(w.items())))
