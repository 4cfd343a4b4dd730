"""The dense / vector C ABI of include/gp_grief_amd.h at its edges, called
through ctypes exactly as a C caller would: leading dimensions larger than the
row, operands that start one double into their allocation, tile and split-K
tails, every alpha / beta and right-hand-side width the models use, and the
primitives that had no direct parity test.

Padded operands: a matrix lives in the first `cols` columns of a (rows, ld)
buffer whose padding holds NaN.  A correct kernel never reads the padding into
arithmetic (so no NaN can reach a result) and never writes it (checked bit for
bit after every call).

GEMM / GEMV / dot bound (elementwise, derived, not tuned): a sum of K products
accumulated in any order, with or without FMA, then reduced over at most S = 64
split-K slabs and passed through the alpha / beta epilogue, obeys
    |got - ref| <= (K + S + 4) u (|alpha| |op(A)| |op(B)| + |beta| |C0|),
u = 2^-53, against a reference accumulated in np.longdouble.  NumPy's own
float64 product meets it for every case below (checked on the host)."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SLABS = 64          # the library's cap on split-K slabs (splitk_factor, tn_splitk)
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GG_ERR_VALUE = -1


def _kbk():
    src = open(os.path.join(ROOT, "gp_grief_amd", "csrc", "gg_dense.hip")).read()
    return int(re.search(r"\bkBK\s*=\s*(\d+)", src).group(1))


KBK = _kbk()


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ld_variants(cols):
    """(ld, pointer offset in doubles): cols + 1 (flips the parity of the row
    stride, rows no longer 16-byte aligned), cols + 3, an even padded ld, and a
    view that starts one double into its allocation."""
    even = cols + 2 - cols % 2
    out = [(cols + 1, 0), (cols + 3, 0)]
    if (even, 0) not in out:
        out.append((even, 0))
    out.append((even, 1))
    return out


class Pad(object):
    """A rows x cols matrix inside a (rows, ld) device buffer that starts `off`
    doubles into its allocation; everything that is not the matrix is NaN."""

    def __init__(self, mat, ld, off=0):
        import torch
        mat = np.asarray(mat, dtype=np.float64)
        self.rows, self.cols = mat.shape
        assert ld >= self.cols
        self.ld, self.off = int(ld), int(off)
        self.h0 = np.full(self.off + self.rows * self.ld, np.nan)
        self.view(self.h0)[...] = mat
        self.d = torch.from_numpy(self.h0.copy()).cuda()

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[
            :, :self.cols]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.d.data_ptr() + 8 * self.off)

    def read(self, keep=None):
        """The matrix after a call; asserts that every double outside it -- and,
        with `keep` (a boolean rows x cols mask), inside it where keep is set --
        is bit for bit what it was."""
        flat = self.d.cpu().numpy()
        a, b = bits(flat).copy(), bits(self.h0).copy()
        hole = np.ones((self.rows, self.cols), dtype=bool) if keep is None else ~keep
        self.view(a)[hole] = 0
        self.view(b)[hole] = 0
        assert np.array_equal(a, b), "padding (or a protected region) was written"
        return self.view(flat).copy()

    def snapshot(self):
        """Take the buffer as it is now as the image later reads compare with."""
        self.h0 = self.d.cpu().numpy().copy()
        return self


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()


def dev_at(x, off=0):
    """A device copy of vector x that starts `off` doubles into its allocation
    (the tensor, and the pointer to x[0]; valid for an empty x too)."""
    import torch
    h = np.full(off + x.size + 1, np.nan)
    h[off:off + x.size] = x
    t = torch.from_numpy(h).cuda()
    return t, ctypes.c_void_p(t.data_ptr() + 8 * off)


def ldmm(a, b):
    return np.asarray(a, dtype=LD) @ np.asarray(b, dtype=LD)


def assert_gamma(got, ref, mag, K, what=""):
    """|got - ref| <= (K + S + 4) u mag elementwise; NaN fails."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    bound = (K + SLABS + 4) * U * np.asarray(mag, dtype=LD)
    ok = err <= bound
    if not np.all(ok):
        bad = np.flatnonzero(~ok.reshape(-1))
        raise AssertionError("%s: %d of %d elements outside the bound; first: got %r ref %r bound %r"
                             % (what, bad.size, ok.size, np.asarray(got).reshape(-1)[bad[0]],
                                np.asarray(ref).reshape(-1)[bad[0]], bound.reshape(-1)[bad[0]]))


# ------------------------------------------------------------------ GEMM
GEMM_SHAPES = [(1, 1, 1), (2, 2, 3), (2, 128, 1), (129, 1, 3), (127, 129, 4 * KBK),
               (129, 127, 4 * KBK + 1), (128, 128, 4 * KBK + 1), (130, 130, 4 * KBK),
               (130, 2, 4097), (1, 129, 4097), (128, 128, 4097)]
ALPHA_BETA = [(1.0, 0.0), (0.5, -2.0), (-1.0, 1.0)]
_gemm_cache = {}


def gemm_problem(M, N, K):
    """op(A), op(B), C0, the long-double product and the float64 magnitude
    product of one shape (computed once, shared by the four transposes)."""
    key = (M, N, K)
    if key not in _gemm_cache:
        rng = np.random.default_rng(1000003 * M + 1009 * N + K)
        oa = rng.standard_normal((M, K))
        ob = rng.standard_normal((K, N))
        c0 = rng.standard_normal((M, N))
        prod = ldmm(oa, ob)
        # |op(A)| |op(B)| in float64: its own rounding (K u relative) is far
        # below anything the bound resolves
        mag = np.abs(oa) @ np.abs(ob)
        for v in (oa, ob, c0, prod, mag):
            v.setflags(write=False)
        _gemm_cache[key] = (oa, ob, c0, prod, mag)
    return _gemm_cache[key]


def run_gemm(nat, ta, tb, M, N, K, alpha, beta, uplo, Ap, Bp, Cp):
    need = ctypes.c_int64(0)
    work = None
    if K >= 4096:
        nat.check(nat.lib().gg_gemm_workspace_elems(int(ta), int(tb), M, N, K, uplo,
                                                    ctypes.byref(need)))
        if need.value > 0:
            import torch
            work = torch.empty(need.value, dtype=torch.float64, device="cuda")
    nat.check(nat.lib().gg_gemm(int(ta), int(tb), M, N, K, alpha, Ap.ptr, Ap.ld, Bp.ptr, Bp.ld,
                                beta, Cp.ptr, Cp.ld, uplo,
                                nat.dptr(work) if work is not None else None, need.value,
                                nat.stream_ptr()), "gg_gemm")


def check_gemm(nat, ta, tb, shape, alpha, beta, uplo, va, vb, vc, what):
    M, N, K = shape
    oa, ob, c0, prod, mag = gemm_problem(M, N, K)
    A = oa.T if ta else oa
    B = ob.T if tb else ob
    Ap = Pad(A, A.shape[1] + va[0], va[1])
    Bp = Pad(B, B.shape[1] + vb[0], vb[1])
    Cp = Pad(c0, N + vc[0], vc[1])
    run_gemm(nat, ta, tb, M, N, K, alpha, beta, uplo, Ap, Bp, Cp)
    i, j = np.indices((M, N))
    written = (i >= j) if uplo == 1 else (i <= j) if uplo == 2 else np.ones((M, N), dtype=bool)
    got = Cp.read(keep=~written)     # the other strict triangle: bit for bit C0
    ref = LD(alpha) * prod + LD(beta) * c0.astype(LD)
    bound_mag = abs(alpha) * mag + abs(beta) * np.abs(c0)
    assert_gamma(got[written], ref[written], bound_mag[written], K, what)


def pads_of(cols):
    """ld_variants as (padding, offset) pairs."""
    return [(ld - cols, off) for ld, off in ld_variants(cols)]


@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
def test_gemm_padded(nat, shape, ta, tb):
    """All four transposes, uplo 0 / 1 / 2 and the three alpha / beta pairs at
    shapes that straddle the 128 x 128 tile and the split thresholds, every
    operand padded (each of the ld variants on each of A, B, C) or offset."""
    M, N, K = shape
    acols = M if ta else K
    bcols = K if tb else N
    combos = list(itertools.product([0, 1, 2], ALPHA_BETA))
    for idx, (uplo, (alpha, beta)) in enumerate(combos):
        va = pads_of(acols)
        vb = pads_of(bcols)
        vc = pads_of(N)
        a = va[(idx + int(ta)) % len(va)]
        b = vb[(idx + 1 + int(tb)) % len(vb)]
        c = vc[(idx + 2) % len(vc)]
        check_gemm(nat, ta, tb, shape, alpha, beta, uplo, a, b, c,
                   "gemm ta=%d tb=%d %s uplo=%d alpha=%g beta=%g pads %s %s %s"
                   % (ta, tb, shape, uplo, alpha, beta, a, b, c))


@pytest.mark.parametrize("shape", [(2, 2, 3), (128, 128, 4 * KBK + 1), (130, 130, 4 * KBK),
                                   (130, 2, 4097), (128, 128, 4097)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("uplo", [0, 1])
def test_gemm_tn_dispatch(nat, monkeypatch, shape, uplo):
    """TN at even shapes: once eligible for the LDS-DMA kernel (even lda / ldb,
    16-byte aligned A and B), then forced onto the register-staged kernel by an
    odd lda, by an odd ldb, by a misaligned A, and by GG_GEMM_TN=0."""
    M, N, K = shape
    alpha, beta = 0.5, -2.0
    routes = [("dma", (2, 0), (2, 0)), ("dma-packed", (0, 0), (0, 0)),
              ("odd-lda", (1, 0), (2, 0)), ("odd-ldb", (2, 0), (3, 0)),
              ("misaligned-A", (2, 1), (2, 0)), ("misaligned-B", (2, 0), (2, 1))]
    for name, va, vb in routes:
        check_gemm(nat, True, False, shape, alpha, beta, uplo, va, vb, (2, 0),
                   "gemm TN %s %s uplo=%d" % (name, shape, uplo))
    monkeypatch.setenv("GG_GEMM_TN", "0")
    nat.knobs_reload()
    try:
        check_gemm(nat, True, False, shape, alpha, beta, uplo, (2, 0), (2, 0), (2, 0),
                   "gemm TN GG_GEMM_TN=0 %s uplo=%d" % (shape, uplo))
    finally:
        monkeypatch.delenv("GG_GEMM_TN")
        nat.knobs_reload()


# ------------------------------------------------------------------ GEMV
def gemv_work_sizes(cols):
    """What dense.matvec passes (2048 * cols) and the smallest buffer gemv()
    accepts: it clamps the row split S to work_elems / cols and then requires
    work_elems >= S * cols, so one slab of `cols` doubles is the minimum."""
    return [2048 * cols, cols]


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 257), (64, 1), (65, 300), (4097, 37),
                                       (1000, 513)])
def test_gemv_padded(nat, rows, cols):
    import torch
    rng = np.random.default_rng(7 * rows + cols)
    A = rng.standard_normal((rows, cols))
    xs = {False: rng.standard_normal(cols), True: rng.standard_normal(rows)}
    y0s = {False: rng.standard_normal(rows), True: rng.standard_normal(cols)}
    absA = np.abs(A)
    for trans in (False, True):
        x, y0 = xs[trans], y0s[trans]
        opA = A.T if trans else A
        prod = ldmm(opA, x)
        mag = (absA.T if trans else absA) @ np.abs(x)
        K = rows if trans else cols
        works = gemv_work_sizes(cols) if trans else [0]
        for (alpha, beta), welems in itertools.product(ALPHA_BETA, works):
            ref = LD(alpha) * prod + LD(beta) * y0.astype(LD)
            bmag = abs(alpha) * mag + abs(beta) * np.abs(y0)
            results = []
            for ld, off in [(cols, 0)] + ld_variants(cols):
                Ap = Pad(A, ld, off)
                y, xd = dev(y0), dev(x)
                work = torch.empty(welems, dtype=torch.float64, device="cuda") if welems else None
                nat.check(nat.lib().gg_gemv(int(trans), rows, cols, alpha, Ap.ptr, ld, nat.dptr(xd),
                                            beta, nat.dptr(y),
                                            nat.dptr(work) if work is not None else None, welems,
                                            nat.stream_ptr()), "gg_gemv")
                Ap.read(keep=np.ones((rows, cols), dtype=bool))   # A untouched, padding too
                got = y.cpu().numpy()
                assert_gamma(got, ref, bmag, K, "gemv trans=%d %dx%d lda=%d off=%d alpha=%g beta=%g "
                             "work=%d" % (trans, rows, cols, ld, off, alpha, beta, welems))
                results.append(got)
            # neither GEMV kernel looks at the stride or the alignment for
            # anything but addressing: padded == packed, bit for bit
            for got in results[1:]:
                assert np.array_equal(bits(got), bits(results[0]))


# ------------------------------------------------------------------ Cholesky family
CHOL_N = [1, 63, 64, 65, 129, 257, 577, 640]
RHS = [(1, 1), (1, 3)] + [(r, r + e) for r in (3, 64, 65, 130, 200) for e in (0, 1)]
_chol_cache = {}


def chol_problem(n):
    if n not in _chol_cache:
        rng = np.random.default_rng(n)
        G = rng.standard_normal((n, n + 10))
        P = G.dot(G.T) / n + 0.1 * np.eye(n)
        B = rng.standard_normal((n, 200))
        for v in (P, B):
            v.setflags(write=False)
        _chol_cache[n] = (P, B, np.linalg.slogdet(P)[1])
    return _chol_cache[n]


def potrf(nat, P, ld, off):
    import torch
    n = P.shape[0]
    Ap = Pad(P, ld, off)
    we = ctypes.c_int64()
    nat.check(nat.lib().gg_potrf_work_elems(n, ctypes.byref(we)))
    winv = torch.empty(we.value, dtype=torch.float64, device="cuda")
    logdet = ctypes.c_double()
    nat.check(nat.lib().gg_potrf(n, Ap.ptr, ld, nat.dptr(winv), ctypes.byref(logdet),
                                 nat.stream_ptr()), "gg_potrf")
    return Ap, winv, logdet.value


def potrs(nat, n, r, Lp, winv, Bp, which):
    import torch
    tmp = torch.empty(64 * max(r, 1), dtype=torch.float64, device="cuda")
    nat.check(nat.lib().gg_potrs(n, r, Lp.ptr, Lp.ld, nat.dptr(winv), Bp.ptr, Bp.ld, which,
                                 nat.dptr(tmp), nat.stream_ptr()), "gg_potrs")


@pytest.mark.parametrize("n", CHOL_N)
def test_potrf_padded(nat, n):
    """gg_potrf in place inside a padded buffer: L L^T, log-det, the strict
    upper triangle (which the header promises is never written) and the
    padding unchanged; the factor equals the packed call's bit for bit."""
    P, _, logdet_ref = chol_problem(n)
    strict_upper = np.triu(np.ones((n, n), dtype=bool), 1)
    factors = []
    for ld, off in [(n, 0)] + ld_variants(n):
        Ap, _, logdet = potrf(nat, P, ld, off)
        A = Ap.read(keep=strict_upper)
        L = np.tril(A)
        assert rel(L.dot(L.T), P) < 1e-13, (n, ld, off)
        assert abs(logdet - logdet_ref) < 1e-10 * max(1, abs(logdet)), (n, ld, off)
        factors.append((L, logdet))
    # every potrf kernel takes lda for addressing only, and the wide update's
    # TN GEMM reads the panel from the library's own (even-stride, aligned)
    # transposed copy whatever lda is: padded == packed, bit for bit
    for L, logdet in factors[1:]:
        assert np.array_equal(bits(L), bits(factors[0][0]))
        assert logdet == factors[0][1]


def _potrs_cases(nat, n, chain):
    P, Bfull, _ = chol_problem(n)
    lda = n + 3
    Lp, winv, _ = potrf(nat, P, lda, 0)
    Lpk, winvk, _ = potrf(nat, P, n, 0)                 # the packed factor
    L = np.tril(Lp.read(keep=np.triu(np.ones((n, n), dtype=bool), 1)))
    Lp.snapshot()
    Linv = np.linalg.inv(L)
    for r, ldb in RHS:
        B = Bfull[:, :r]
        Btri = np.tril(B)                # lower triangular n x r (zero for j > i)
        Xref = np.linalg.solve(P, B)
        Tref = Linv.dot(Btri)
        for which in (1, 2, 3, 5):
            rhs = Btri if which & 4 else B
            Bp = Pad(rhs, ldb, 0)
            potrs(nat, n, r, Lp, winv, Bp, which)
            X = Bp.read()
            tag = (n, r, ldb, which, chain)
            if which == 1:
                assert rel(L.dot(X), B) < 1e-12, tag
            elif which == 2:
                assert rel(L.T.dot(X), B) < 1e-12, tag
            elif which == 3:
                assert rel(X, Xref) < 1e-10, tag
            else:
                assert rel(X, Tref) < 1e-10, tag
                assert np.all(np.triu(X, 1) == 0), tag
            # Bitwise against the packed factor and a packed right-hand side
            # where the route cannot depend on a stride: the chained kernels
            # (trsv for r == 1 with ldb == 1, trsm for r > 1) and the blocked
            # forward substitution (NN GEMMs only) use strides for addressing
            # alone.  Not asserted: r == 1 with ldb > 1 (ldb itself moves the
            # call from the chained kernel to the blocked path) and the
            # blocked backward substitution (its TN GEMMs take the LDS-DMA or
            # the register-staged kernel by the parity of lda / ldb).
            chained = chain and not (r == 1 and (ldb != 1 or which & 4))
            if chained or (not chain and not which & 2):
                Bk = Pad(rhs, r, 0)
                potrs(nat, n, r, Lpk, winvk, Bk, which)
                assert np.array_equal(bits(Bk.read()), bits(X)), tag
    Lp.read(keep=np.ones((n, n), dtype=bool))            # the factor is read-only


@pytest.mark.parametrize("n", CHOL_N)
def test_potrs_padded_chain(nat, monkeypatch, n):
    """gg_potrs with lda > n at every right-hand-side width the models reach:
    the chained single-vector kernel, r == 1 with ldb > 1, one and several
    64-column chunks with tails, triangular right-hand sides."""
    monkeypatch.delenv("GG_TRSV_CHAIN", raising=False)
    nat.knobs_reload()
    _potrs_cases(nat, n, True)


@pytest.mark.parametrize("n", CHOL_N)
def test_potrs_padded_blocked(nat, monkeypatch, n):
    """The same under GG_TRSV_CHAIN=0, the documented blocked fallback."""
    monkeypatch.setenv("GG_TRSV_CHAIN", "0")
    nat.knobs_reload()
    try:
        _potrs_cases(nat, n, False)
    finally:
        monkeypatch.delenv("GG_TRSV_CHAIN")
        nat.knobs_reload()


@pytest.mark.parametrize("n", CHOL_N)
def test_trtri_colsumsq_padded(nat, n):
    """gg_trtri into a padded X whose strict upper triangle holds a sentinel,
    then gg_colsumsq_lower on that padded X."""
    P, _, _ = chol_problem(n)
    Lp, winv, _ = potrf(nat, P, n + 1, 0)
    L = np.tril(Lp.read(keep=np.triu(np.ones((n, n), dtype=bool), 1)))
    Linv = np.linalg.inv(L)
    dref = np.diag(np.linalg.inv(P))
    i, j = np.indices((n, n))
    in_block = (i // 64) == (j // 64)
    X0 = np.where(j > i, np.nan, 0.0)
    outs = []
    for ldx, off in [(n, 0)] + ld_variants(n):
        Xp = Pad(X0, ldx, off)
        nat.check(nat.lib().gg_trtri(n, Lp.ptr, Lp.ld, nat.dptr(winv), Xp.ptr, ldx,
                                     nat.stream_ptr()), "gg_trtri")
        # above the diagonal and outside the 64 x 64 diagonal blocks: the
        # sentinel, bit for bit ("neither read nor written")
        X = Xp.read(keep=(j > i) & ~in_block)
        assert rel(np.tril(X), Linv) < 1e-10, (n, ldx, off)
        assert np.all(X[(j > i) & in_block] == 0.0), (n, ldx, off)
        out = dev(np.full(n, np.nan))
        Xp.snapshot()
        nat.check(nat.lib().gg_colsumsq_lower(n, Xp.ptr, ldx, nat.dptr(out), nat.stream_ptr()),
                  "gg_colsumsq_lower")
        Xp.read(keep=np.ones((n, n), dtype=bool))      # its input is read-only
        d = out.cpu().numpy()
        assert rel(d, dref) < 1e-10, (n, ldx, off)
        outs.append((np.tril(X), d))
    # trtri's levels run the register-staged NN tile and colsumsq a plain
    # column loop; both take strides for addressing only: padded == packed
    for X, d in outs[1:]:
        assert np.array_equal(bits(X), bits(outs[0][0]))
        assert np.array_equal(bits(d), bits(outs[0][1]))


@pytest.mark.parametrize("n", [1, 3, 64, 65, 257])
def test_add_diag_padded(nat, n):
    rng = np.random.default_rng(100 + n)
    A = rng.standard_normal((n, n))
    w = rng.uniform(0.5, 2.0, n)
    s = 0.37
    for wv in (None, w):
        add = np.full(n, s) if wv is None else s / wv.astype(LD)
        ref = A.astype(LD) + np.diag(np.asarray(add, dtype=LD))
        # one division and one addition: 2 u (|A_ii| + |s / w_i|); off the
        # diagonal a copy
        bound = 2 * U * np.diag(np.abs(A).diagonal() + np.abs(np.asarray(add, dtype=np.float64)))
        outs = []
        variants = [(n, 0, n, 0)] + [(la, oa, lp, op) for (la, oa), (lp, op) in
                                     zip(ld_variants(n), reversed(ld_variants(n)))]
        for lda, offa, ldp, offp in variants:
            Ap = Pad(A, lda, offa)
            Pp = Pad(np.full((n, n), np.nan), ldp, offp)
            wd = dev(wv) if wv is not None else None
            nat.check(nat.lib().gg_add_diag(n, Ap.ptr, lda, s, nat.dptr(wd) if wd is not None
                                            else None, Pp.ptr, ldp, nat.stream_ptr()), "gg_add_diag")
            got = Pp.read()
            Ap.read(keep=np.ones((n, n), dtype=bool))
            assert np.all(np.abs(got.astype(LD) - ref) <= bound), (n, lda, ldp, wv is None)
            outs.append(got)
        for got in outs[1:]:     # an elementwise kernel: strides only address
            assert np.array_equal(bits(got), bits(outs[0]))


# ------------------------------------------------------------------ vector primitives
VEC_N = [0, 1, 2, 3, 255, 256, 257, 511, 513, 2 * 256 * 2048 + 3]


def vec_data(n, seed):
    rng = np.random.default_rng(seed + n)
    return rng.standard_normal(max(n, 1))[:n], rng.standard_normal(max(n, 1))[:n]


@pytest.mark.parametrize("n", VEC_N)
@pytest.mark.parametrize("offx,offy", [(0, 0), (1, 1), (1, 0)])
def test_dot(nat, n, offx, offy):
    x, y = vec_data(n, 11)
    xt, xp = dev_at(x, offx)
    yt, yp = dev_at(y, offy)
    out = ctypes.c_double(np.nan)
    nat.check(nat.lib().gg_dot(xp, yp, n, ctypes.byref(out), nat.stream_ptr()), "gg_dot")
    ref = np.sum(x.astype(LD) * y.astype(LD)) if n else LD(0)
    mag = float(np.sum(np.abs(x) * np.abs(y))) if n else 0.0
    if n == 0:
        assert out.value == 0.0
    assert_gamma(np.array([out.value]), np.array([ref]), np.array([mag]), n, "dot n=%d" % n)


@pytest.mark.parametrize("n", VEC_N)
def test_axpby(nat, n):
    x, y0 = vec_data(n, 13)
    for a, b in [(0.7, -1.3), (0.0, 2.5), (1.5, 0.0), (0.0, 0.0)]:
        for off in (0, 1):
            xt, xp = dev_at(x, off)
            yt, yp = dev_at(y0, off)
            nat.check(nat.lib().gg_axpby(a, xp, b, yp, n, nat.stream_ptr()), "gg_axpby")
            got = yt.cpu().numpy()
            assert np.isnan(got[:off]).all() and np.isnan(got[off + n:]).all()
            got = got[off:off + n]
            ref = LD(a) * x.astype(LD) + LD(b) * y0.astype(LD)
            assert np.all(np.abs(got.astype(LD) - ref) <= 3 * U * (np.abs(a * x) + np.abs(b * y0)))
        # x is y (models.py scales in place with axpby(0, v, s, v)): y = (a + b) y
        yt, yp = dev_at(y0, 0)
        nat.check(nat.lib().gg_axpby(a, yp, b, yp, n, nat.stream_ptr()), "gg_axpby")
        got = yt.cpu().numpy()[:n]
        ref = LD(a) * y0.astype(LD) + LD(b) * y0.astype(LD)
        assert np.all(np.abs(got.astype(LD) - ref) <= 3 * U * (np.abs(a * y0) + np.abs(b * y0)))


@pytest.mark.parametrize("rows", VEC_N)
def test_scale_rows(nat, rows):
    """modes 0 / 1 / 2 on a vector (cols = 1, the 1-D call) and on 2-D blocks."""
    big = rows > 100000
    for cols in ([1, 3] if big else [1, 3, 64, 65]):
        rng = np.random.default_rng(17 * rows + cols)
        A = rng.standard_normal((rows, cols))
        w = rng.uniform(0.5, 2.0, max(rows, 1))[:rows]
        for mode in (0, 1, 2):
            Ad, Aptr = dev_at(A.reshape(-1))
            wd, wptr = dev_at(w)
            nat.check(nat.lib().gg_scale_rows(Aptr, rows, cols, None if mode == 2 else wptr, mode,
                                              nat.stream_ptr()), "gg_scale_rows")
            got = Ad.cpu().numpy()[:rows * cols].reshape(rows, cols)
            AL, wL = A.astype(LD), w.astype(LD)[:, None]
            ref = AL * wL if mode == 0 else AL / wL if mode == 1 else AL * AL
            assert np.all(np.abs(got.astype(LD) - ref) <= 2 * U * np.abs(ref)), (rows, cols, mode)


KRON_SIZES = {1: [[1], [2], [257]], 2: [[3, 1], [1, 64], [5, 7]], 3: [[2, 1, 3], [4, 5, 6]],
              5: [[3, 1, 4, 2, 5], [2, 2, 1, 3, 2]]}


@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_kron_diag_scale(nat, d):
    """The three modes against the expanded long-double eigenvalue product
    (t > 0 and shift > 0: nothing cancels).  Bound 4 u |ref|: the kernel rounds
    d - 1 products, one sum and one or two more operations, each by at most
    u; float64 NumPy in the kernel's operation order stays below 3.6 u on
    these data at d = 5 (2.3 u for d <= 3)."""
    for m in KRON_SIZES[d]:
        rng = np.random.default_rng(d * 100 + sum(m))
        lam = [rng.uniform(0.2, 3.0, mk) for mk in m]
        n = int(np.prod(m))
        x = rng.standard_normal(n)
        shift = 0.3
        t = np.ones(1, dtype=LD)
        for l in lam:
            t = np.kron(t, l.astype(LD))
        xL = x.astype(LD)
        refs = {0: xL / (t + LD(shift)), 1: t * LD(shift) / (t + LD(shift)),
                2: xL * (t + LD(shift))}
        for mode in (0, 1, 2):
            yd, ld_, xd = dev(np.full(n, np.nan)), dev(np.concatenate(lam)), dev(x)
            nat.check(nat.lib().gg_kron_diag_scale(d, nat.i64_array(m), nat.dptr(ld_), shift, mode,
                                                   nat.dptr(xd), nat.dptr(yd), nat.stream_ptr()),
                      "gg_kron_diag_scale")
            got = yd.cpu().numpy()
            assert np.all(np.abs(got.astype(LD) - refs[mode]) <= 4 * U * np.abs(refs[mode])), (m, mode)


@pytest.mark.parametrize("n", VEC_N)
def test_diag_divide(nat, n):
    rng = np.random.default_rng(19 + n)
    t = rng.uniform(0.2, 3.0, max(n, 1))[:n]
    x = rng.standard_normal(max(n, 1))[:n]
    shift = 0.3
    (td, tp), (xd, xp), (yd, yp) = dev_at(t), dev_at(x), dev_at(np.full(n, np.nan))
    nat.check(nat.lib().gg_diag_divide(tp, shift, xp, yp, n, nat.stream_ptr()), "gg_diag_divide")
    ref = x.astype(LD) / (t.astype(LD) + LD(shift))
    assert np.all(np.abs(yd.cpu().numpy()[:n].astype(LD) - ref) <= 4 * U * np.abs(ref))


@pytest.mark.parametrize("n", VEC_N)
def test_kr_hadamard_plain(nat, n):
    """mode 0: P = X (first), then P *= X (running)."""
    x1, x2 = vec_data(n, 23)
    (Pd, Pp), (x1d, x1p), (x2d, x2p) = dev_at(np.full(n, np.nan)), dev_at(x1), dev_at(x2)
    nat.check(nat.lib().gg_kr_hadamard(n, x1p, Pp, None, 0, 1, nat.stream_ptr()),
              "gg_kr_hadamard")
    assert np.array_equal(bits(Pd.cpu().numpy()[:n]), bits(x1))
    nat.check(nat.lib().gg_kr_hadamard(n, x2p, Pp, None, 0, 0, nat.stream_ptr()),
              "gg_kr_hadamard")
    ref = x1.astype(LD) * x2.astype(LD)
    assert np.all(np.abs(Pd.cpu().numpy()[:n].astype(LD) - ref) <= 2 * U * np.abs(ref))


@pytest.mark.parametrize("n", VEC_N)
def test_kr_hadamard_logged(nat, n):
    """mode 1 against the header's rule restated literally: S *= sign(X);
    P += log|X| with X taken as 1 where S == 0 (first: S = 1, P = 0 before)."""
    rng = np.random.default_rng(29 + n)
    xs = []
    for k in range(3):
        x = rng.standard_normal(max(n, 1))[:n]
        x[rng.random(n) < 0.15] = 0.0          # exact zeros; negatives come by themselves
        xs.append(x)
    (Pd, Pp), (Sd, Sp) = dev_at(np.full(n, np.nan)), dev_at(np.full(n, np.nan))
    S = np.ones(n)
    P = np.zeros(n, dtype=LD)
    for k, x in enumerate(xs):
        xd, xp = dev_at(x)
        nat.check(nat.lib().gg_kr_hadamard(n, xp, Pp, Sp, 1, int(k == 0), nat.stream_ptr()),
                  "gg_kr_hadamard")
        S = S * np.sign(x)
        P = P + np.log(np.abs(np.where(S == 0, 1.0, x)).astype(LD))
        if n == 0:
            continue
        assert np.array_equal(Sd.cpu().numpy()[:n], S)
        got = Pd.cpu().numpy()[:n]
        assert np.all(np.isfinite(got))
        assert rel(got, P.astype(np.float64)) < 1e-14


def test_rows_orthonormalize(nat):
    blocks = [(1, 1), (3, 7), (12, 200), (0, 5)]
    rng = np.random.default_rng(31)
    V0 = [rng.standard_normal((k, m)) for k, m in blocks]
    Vd = dev(np.concatenate([v.reshape(-1) for v in V0]))
    nat.check(nat.lib().gg_rows_orthonormalize(len(blocks), nat.i64_array([k for k, _ in blocks]),
                                               nat.i64_array([m for _, m in blocks]),
                                               nat.dptr(Vd), nat.stream_ptr()),
              "gg_rows_orthonormalize")
    out = Vd.cpu().numpy()
    o = 0
    for (k, m), v0 in zip(blocks, V0):
        Q = out[o:o + k * m].reshape(k, m)
        o += k * m
        if k == 0:
            continue
        assert np.abs(Q.dot(Q.T) - np.eye(k)).max() < 1e-12, (k, m)
        # same row space: the input rows projected onto the output rows
        assert np.abs(v0.dot(Q.T).dot(Q) - v0).max() < 1e-12 * np.abs(v0).max(), (k, m)


# ------------------------------------------------------------------ argument validation
def test_ld_below_columns_is_rejected(nat):
    """ld < cols (or < n) is GG_ERR_VALUE from every dense entry point, before
    any device work.  Every buffer is large enough that no access could leave
    it even without the check."""
    import torch
    lib = nat.lib()
    n = 8
    big = [torch.ones(8192, dtype=torch.float64, device="cuda") for _ in range(4)]
    a, b, c, w = [nat.dptr(t) for t in big]
    s = nat.stream_ptr()
    ld = ctypes.c_double()
    # gg_gemm: A is M x K (K x M transposed), B is K x N (N x K), C is M x N
    M, N, K = 4, 6, 8
    for ta, tb, lda, ldb, ldc in [(0, 0, K - 1, N, N), (1, 0, M - 1, N, N), (0, 0, K, N - 1, N),
                                  (0, 1, K, K - 1, N), (0, 0, K, N, N - 1), (1, 1, M, K, N - 1)]:
        assert lib.gg_gemm(ta, tb, M, N, K, 1.0, a, lda, b, ldb, 0.0, c, ldc, 0, None, 0,
                           s) == GG_ERR_VALUE, (ta, tb, lda, ldb, ldc)
    for trans in (0, 1):
        assert lib.gg_gemv(trans, n, n, 1.0, a, n - 1, b, 0.0, c, w, 8192, s) == GG_ERR_VALUE
    assert lib.gg_add_diag(n, a, n - 1, 1.0, None, c, n, s) == GG_ERR_VALUE
    assert lib.gg_add_diag(n, a, n, 1.0, None, c, n - 1, s) == GG_ERR_VALUE
    assert lib.gg_potrf(n, a, n - 1, w, ctypes.byref(ld), s) == GG_ERR_VALUE
    assert lib.gg_potrs(n, 3, a, n - 1, w, b, 3, 3, c, s) == GG_ERR_VALUE
    assert lib.gg_potrs(n, 3, a, n, w, b, 2, 3, c, s) == GG_ERR_VALUE
    assert lib.gg_trtri(n, a, n - 1, w, c, n, s) == GG_ERR_VALUE
    assert lib.gg_trtri(n, a, n, w, c, n - 1, s) == GG_ERR_VALUE
    assert lib.gg_colsumsq_lower(n, a, n - 1, c, s) == GG_ERR_VALUE
    torch.cuda.synchronize()
    for t in big:                       # nothing ran
        assert bool((t == 1.0).all())
