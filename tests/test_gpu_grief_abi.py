"""The GRIEF basis section of include/gp_grief_amd.h (gg_cov, gg_grief_tables,
gg_grief_tables_all, gg_grief_phi, gg_expand_skc) at its edges, called through
ctypes exactly as a C caller would, against the np.longdouble reference of
tests/grief_abi_ref.py.

Every operand lives inside a larger device buffer whose remainder holds NaN
(int32 outputs: a sentinel).  After every call every byte outside the
documented output region must be what it was, and a NaN in a result means
padding was read into arithmetic.

Bounds (elementwise, u = 2^-53, derived, not tuned; NumPy's own float64
evaluation meets each of them for every case below, tests/test_grief_abi_ref.py):
  gg_cov      |got - ref| <= (D + 8)(1 + t) u |ref|, t the magnitude of the
              exponent's argument: D FMAs for d2, a handful of roundings to
              form the argument, whose error exp amplifies by t, exp itself at
              1 ulp, the polynomial and the variance; plus 2^-1072 absolute,
              for gradual underflow alone (the RBF at l = 0.05, D = 7 reaches
              exp(-710): a subnormal float64 has no relative accuracy; the
              term is invisible for every normal result).  mode 1 (out = k0 k):
              ((D + 8)(1 + t) + 1) u |k0 ref|; mode 2 (out = k0 + k):
              ((D + 8)(1 + t) + 1) u (|k0| + |ref|) -- the same scale plus one
              rounding, of the product and of the sum.
  tables      |got - X| <= (mp + 17) u A, mp = 16 ceil(m / 16), A = |qsel| @
              (|k| (1 + t)): mp accumulations in any order (MFMA or FMA chains
              and shuffles) plus the covariance bound's constant, against the
              majorant, so cancellation in high eigenvector rows does not
              matter.  Log / sign form: S exp(L) meets that plus
              4 u |X| (1 + |L|) (log at 1 ulp, its rounding amplified by exp).
  gg_grief_phi |got - ref| <= (3 d + 4) u |ref| against the tables given
              (for the log form the table S exp(L) they stand for): d
              multiplies, the scale's exp, one exp per factor.
  gg_expand_skc (d + 1) u |ref| not logged; logged 2 (d + 1) u sum_f (1 +
              |log|v_f||) with the sign exact.

Which case reaches which kernel (from the dispatch conditions of
gg_grief.hip, whose thresholds are parsed from the source below; the routes
are recomputed from them and asserted, so a moved threshold moves the shapes
or fails here):
  tables  (1,1) (3,2) (17,15) (24,16) (24,17) (64,33): grief_tables_mfma_kernel
          with padded m, a partial row group, and two / three row groups;
          (480,5): the last m whose staging fits 64 KiB, still MFMA;
          (481,5) (512,18): grief_tables_kernel<true> (lane quads, LDS);
          (513,18): grief_tables_kernel<false> (lane quads, global memory);
          the delta RBF (l = 1e-7) and GG_GRIEF_TABLES=0: the lane-quad
          kernels at every shape; gg_grief_tables_all: one batched MFMA launch
          (m = 24, 7, 64), the per-factor fallback of a whole batch
          (m = 24, 500, 7) and a 16 + 1 split (nf = 17).
  phi     row-major, aligned, even p, d <= 8: grief_phi_pair_kernel ((2,9,2),
          (3,20,256), (5,40,514) and (8,64,600): the second pass of its jp
          loop); odd p ((1,3,1), (3,20,255), (3,20,257)), a buffer one double
          past alignment, GG_PHI_PAIR=0 and d > 8: grief_phi_kernel<64,false,kD>
          (p > 256: a second blockIdx.y with a column tail); d = 9, 17, 64:
          kD = 0; transposed: grief_phi_kernel<32,true,kD>.
"""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

import grief_abi_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GG_OK, GG_ERR_VALUE = 0, -1
KINDS = (0, 1, 2, 3)


def _src_consts():
    src = open(os.path.join(ROOT, "gp_grief_amd", "csrc", "gg_grief.hip")).read()

    def one(pat):
        m = re.search(pat, src)
        assert m, "gg_grief.hip no longer matches %r: update the test's dispatch model" % pat
        return int(m.group(1))
    return dict(
        tab_lds=1024 * one(r"16 \* \(mp \+ 1\) \+ mp\) \* sizeof\(double\) > (\d+) \* 1024"),
        quad_lds_m=one(r"in_lds = m <= (\d+)"),
        tab_max_f=one(r"kTabMaxF = (\d+)"),
        rows=one(r"kPhiRows = (\d+)"), rows_t=one(r"kPhiRowsT = (\d+)"),
        cols=one(r"kPhiCols = (\d+)"), max_dim=one(r"kMaxDim = (\d+)"),
        phi_lds=1024 * one(r"GG_REQUIRE\(lds <= (\d+) \* 1024"))


C = _src_consts()
# the largest m whose MFMA staging (16 padded rows of mp + 1 and the grid) fits
M_MFMA = max(m for m in range(1, 4096)
             if (16 * (((m + 15) & ~15) + 1) + ((m + 15) & ~15)) * 8 <= C["tab_lds"])
M_QUAD = C["quad_lds_m"]


def tables_route(kind, ls, m, knob_off):
    """The kernel gg_grief_tables launches, from the dispatch conditions."""
    if not knob_off and not (kind == 0 and ls < 1e-6) and m <= M_MFMA:
        return "mfma"
    return "quad_lds" if m <= M_QUAD else "quad_global"


def phi_route(d, p, aligned, pair_on, transposed, U):
    if transposed:
        return "T"
    if pair_on and d <= 8 and p % 2 == 0 and aligned and C["rows"] * U * 8 <= C["phi_lds"]:
        return "pair"
    return "cols"


def phi_u_cap(d, transposed):
    """The largest U whose block fits the LDS cap (gg_grief_phi's lds formula)."""
    kr = C["rows_t"] if transposed else C["rows"]
    fixed = d * C["cols"] * 4 + (C["cols"] * (kr + 1) * 8 if transposed else 0)
    return (C["phi_lds"] - fixed) // (kr * 8)


WORST = {}


def check(entry, got, ref, bound, what=""):
    """|got - ref| <= bound elementwise (NaN fails); records the worst ratio."""
    got = np.asarray(got)
    assert not np.any(np.isnan(got)), "%s %s: NaN in the result (padding was read)" % (entry, what)
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    ok = err <= bound
    if err.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        WORST[entry] = max(WORST.get(entry, 0.0), float(ratio.max()))
    if not np.all(ok):
        bad = np.flatnonzero(~ok.reshape(-1))
        raise AssertionError(
            "%s %s: %d of %d elements outside the bound; first at %d: got %r ref %r bound %r"
            % (entry, what, bad.size, ok.size, bad[0], got.reshape(-1)[bad[0]],
               np.asarray(ref).reshape(-1)[bad[0]], bound.reshape(-1)[bad[0]]))


@pytest.fixture(scope="module")
def nat(gpu):
    from gp_grief_amd import native
    return native


@contextlib.contextmanager
def knob(nat, name, value):
    """The library under `name`=value (None: unset) from gg_knobs_reload on;
    the environment is restored and reloaded on the way out."""
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        nat.knobs_reload()
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old
        nat.knobs_reload()


class Buf(object):
    """An array inside a device buffer with `guard` elements before (plus
    `off`) and after it; the guards hold NaN (int32: a sentinel)."""

    def __init__(self, region, guard=64, off=0):
        import torch
        region = np.ascontiguousarray(region)
        self.shape, self.dtype = region.shape, region.dtype
        self.lo = int(guard) + int(off)
        fill = np.nan if region.dtype == np.float64 else -123456789
        self.h0 = np.full(self.lo + region.size + int(guard), fill, dtype=region.dtype)
        self.h0[self.lo:self.lo + region.size] = region.reshape(-1)
        self.d = torch.from_numpy(self.h0.copy()).cuda()

    def ptr(self, elem=0):
        return ctypes.c_void_p(self.d.data_ptr() + self.dtype.itemsize * (self.lo + int(elem)))

    def read(self, written=None):
        """The array now; every element outside it, and inside it wherever
        `written` (a boolean mask; None: the whole array) is False, must be bit
        for bit what it was."""
        flat = self.d.cpu().numpy()
        a, b = flat.copy(), self.h0.copy()
        w = np.ones(self.shape, dtype=bool) if written is None else np.broadcast_to(written, self.shape)
        n = int(np.prod(self.shape))
        a[self.lo:self.lo + n][w.reshape(-1)] = 0
        b[self.lo:self.lo + n][w.reshape(-1)] = 0
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), \
            "a guard block or an element outside the documented output was written"
        return flat[self.lo:self.lo + n].reshape(self.shape).copy()

    def untouched(self):
        self.read(written=np.zeros(self.shape, dtype=bool))


def nans(*shape):
    return np.full(shape, np.nan)


# ---------------------------------------------------------------- gg_cov
COV_SHAPES = [(1, 1), (37, 23), (255, 257)]
COV_DS = (1, 3, 7)
COV_LS = (0.05, 0.3, 2.0)
COV_WRAP = (2, 3, 0.3, 1500, 1500)     # kind, D, ls, nx, nz: > 8192 * 256 elements
COV_VAR = 1.3


def cov_mode_bound(mode, D, out0, k, t):
    """(reference, bound) of out after a mode 0 / 1 / 2 call from out0."""
    o = np.asarray(out0, dtype=LD)
    if mode == 0:
        return k, R.cov_bound(D, k, t)
    if mode == 1:
        return o * k, ((D + 8) * (1 + t) + 1) * R.U53 * np.abs(o * k) + (1 + np.abs(o)) * R.TINY
    return o + k, ((D + 8) * (1 + t) + 1) * R.U53 * (np.abs(o) + np.abs(k)) + R.TINY


def run_cov(nat, kind, var, ls, D, x, z, mode, out0):
    nx, nz = x.shape[0], z.shape[0]
    xb, zb = Buf(x), Buf(z)
    ob = Buf(out0 if mode else nans(nx, nz))
    st = nat.lib().gg_cov(kind, var, ls, D, xb.ptr(), nx, zb.ptr(), nz, mode, ob.ptr(),
                          nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    xb.untouched()
    zb.untouched()
    return ob.read()


@pytest.mark.parametrize("D", COV_DS)
@pytest.mark.parametrize("kind", KINDS)
def test_cov_write(nat, kind, D):
    for ls in COV_LS:
        for nx, nz in COV_SHAPES:
            x, z, out0, k, t = R.cov_problem(kind, D, ls, nx, nz, COV_VAR)
            got = run_cov(nat, kind, COV_VAR, ls, D, x, z, 0, out0)
            check("gg_cov", got, k, R.cov_bound(D, k, t), "kind %d D %d ls %g %dx%d" % (kind, D, ls, nx, nz))


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_cov_modes(nat, kind, mode):
    """out *= k and out += k from a known out."""
    nx, nz = COV_SHAPES[1]
    for D in COV_DS:
        for ls in COV_LS:
            x, z, out0, k, t = R.cov_problem(kind, D, ls, nx, nz, COV_VAR)
            got = run_cov(nat, kind, COV_VAR, ls, D, x, z, mode, out0)
            ref, bound = cov_mode_bound(mode, D, out0, k, t)
            check("gg_cov mode %d" % mode, got, ref, bound, "kind %d D %d ls %g" % (kind, D, ls))


def test_cov_grid_stride_wraps(nat):
    """1500 x 1500 > 8192 blocks x 256 threads: the grid-stride loop's second trip."""
    kind, D, ls, nx, nz = COV_WRAP
    assert nx * nz > 8192 * 256
    x, z, out0, k, t = R.cov_problem(kind, D, ls, nx, nz, COV_VAR)
    got = run_cov(nat, kind, COV_VAR, ls, D, x, z, 0, out0)
    check("gg_cov", got, k, R.cov_bound(D, k, t), "1500 x 1500")


def cov_delta_problem(D):
    rng = np.random.default_rng(40 + D)
    z = rng.random((23, D))
    x = rng.random((37, D))
    x[::3] = z[rng.integers(0, 23, x[::3].shape[0])]      # exact copies of z rows
    return x, z


@pytest.mark.parametrize("D", COV_DS)
def test_cov_delta_rbf(nat, D):
    """l = 1e-7: exactly var where x_i == z_j, exactly 0 elsewhere."""
    x, z = cov_delta_problem(D)
    got = run_cov(nat, 0, COV_VAR, 1e-7, D, x, z, 0, None)
    hit = (x[:, None, :] == z[None, :, :]).all(-1)
    assert hit.sum() >= 13
    assert np.array_equal(got, np.where(hit, COV_VAR, 0.0))


def test_cov_empty_and_errors(nat):
    L, s = nat.lib(), nat.stream_ptr()
    x, z, ob = Buf(np.ones((4, 2))), Buf(np.ones((3, 2))), Buf(nans(4, 3))
    assert L.gg_cov(0, 1.0, 0.3, 2, x.ptr(), 0, z.ptr(), 3, 0, ob.ptr(), s) == GG_OK
    assert L.gg_cov(0, 1.0, 0.3, 2, x.ptr(), 4, z.ptr(), 0, 0, ob.ptr(), s) == GG_OK
    for kind, mode, dims, xp, zp, op in [(-1, 0, 2, x.ptr(), z.ptr(), ob.ptr()),
                                         (4, 0, 2, x.ptr(), z.ptr(), ob.ptr()),
                                         (0, 3, 2, x.ptr(), z.ptr(), ob.ptr()),
                                         (0, 0, 0, x.ptr(), z.ptr(), ob.ptr()),
                                         (0, 0, 2, None, z.ptr(), ob.ptr()),
                                         (0, 0, 2, x.ptr(), None, ob.ptr()),
                                         (0, 0, 2, x.ptr(), z.ptr(), None)]:
        assert L.gg_cov(kind, 1.0, 0.3, dims, xp, 4, zp, 3, mode, op, s) == GG_ERR_VALUE
    ob.untouched()


# ------------------------------------------------- gg_grief_tables(_all)
TAB_SHAPES = [(1, 1), (3, 2), (17, 15), (24, 16), (24, 17), (64, 33), (M_MFMA, 5),
              (M_MFMA + 1, 5), (M_QUAD, 18), (M_QUAD + 1, 18)]
TAB_ROUTES = ["mfma"] * 7 + ["quad_lds"] * 2 + ["quad_global"]
TAB_NS = (1, 15, 16, 17, 83)
TAB_LS = (0.05, 0.3)
TAB_VAR = 0.7
TAB_GAP = (2, 3)          # untouched table columns before / after the factor's


def run_tables(nat, kind, var, ls, x, xg, q, log):
    """One gg_grief_tables call with x a column of an n x 3 array (x_stride =
    d + 2), U = u + 5 and guard rows around the tables; (L, S or None), u x n."""
    n, (u, m) = x.size, q.shape
    xa = nans(n, 3)
    xa[:, 1] = x
    xb, gb, qb = Buf(xa), Buf(xg), Buf(q)
    Ut = u + sum(TAB_GAP)
    lb = Buf(nans(n, Ut), guard=2 * Ut)
    sb = Buf(nans(n, Ut), guard=2 * Ut) if log else None
    st = nat.lib().gg_grief_tables(kind, var, ls, xb.ptr(1), 3, n, gb.ptr(), m, qb.ptr(), u,
                                   lb.ptr(), sb.ptr() if log else None, Ut, TAB_GAP[0],
                                   nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    w = np.zeros((n, Ut), dtype=bool)
    w[:, TAB_GAP[0]:TAB_GAP[0] + u] = True
    for b in (xb, gb, qb):
        b.untouched()
    Lg = lb.read(w)[:, TAB_GAP[0]:TAB_GAP[0] + u].T
    return Lg, (sb.read(w)[:, TAB_GAP[0]:TAB_GAP[0] + u].T if log else None)


def check_log_sign(entry, Lg, Sg, X, bound, q, what):
    """S = sign(X) where |X| exceeds the value bound; S exp(L) within the value
    bound plus 4 u |X| (1 + |L|); an exactly zero qsel row: L == S == +0.0."""
    assert not np.any(np.isnan(Lg)) and not np.any(np.isnan(Sg)), what
    assert np.all(np.isin(Sg, (-1.0, 0.0, 1.0))), what
    sure = np.abs(X) > bound
    assert np.array_equal(Sg[sure], np.sign(X[sure]).astype(np.float64)), what + ": sign"
    val = np.asarray(Sg, dtype=LD) * np.exp(np.asarray(Lg, dtype=LD))
    assert not np.any(np.isnan(val)), what
    err_bound = bound + 4 * R.U53 * np.abs(X) * (1 + np.abs(Lg))
    err = np.abs(val - X)
    WORST[entry] = max(WORST.get(entry, 0.0), float((err / np.where(err_bound > 0, err_bound, 1)).max()))
    assert np.all(err <= err_bound), what + ": S exp(L)"
    for r in np.flatnonzero(~q.any(axis=1)):
        z = np.zeros(Lg.shape[1])
        assert np.array_equal(Lg[r].view(np.uint64), z.view(np.uint64)), what + ": L of a zero row"
        assert np.array_equal(Sg[r].view(np.uint64), z.view(np.uint64)), what + ": S of a zero row"


@pytest.mark.parametrize("tables_knob", [None, "0"], ids=["default", "GG_GRIEF_TABLES=0"])
@pytest.mark.parametrize("shape,route", list(zip(TAB_SHAPES, TAB_ROUTES)),
                         ids=["m%d_u%d" % s for s in TAB_SHAPES])
def test_tables_value(nat, shape, route, tables_knob):
    """Value tables of every branch shape, n and kind, under the default
    dispatch and under GG_GRIEF_TABLES=0 (each kernel meets the bound on its
    own; they are not compared with each other)."""
    m, u = shape
    off = tables_knob is not None
    assert tables_route(1, 0.3, m, False) == route
    assert tables_route(1, 0.3, m, True) == ("quad_global" if m > M_QUAD else "quad_lds")
    with knob(nat, "GG_GRIEF_TABLES", tables_knob):
        for n in TAB_NS:
            for kind in KINDS:
                for ls in TAB_LS:
                    x, xg, q, X, A = R.tables_problem(kind, ls, m, u, n, TAB_VAR)
                    got, _ = run_tables(nat, kind, TAB_VAR, ls, x, xg, q, False)
                    check("gg_grief_tables " + tables_route(kind, ls, m, off), got, X,
                          R.tables_bound(m, A), "m %d u %d n %d kind %d ls %g" % (m, u, n, kind, ls))


@pytest.mark.parametrize("tables_knob", [None, "0"], ids=["default", "GG_GRIEF_TABLES=0"])
@pytest.mark.parametrize("shape", TAB_SHAPES, ids=["m%d_u%d" % s for s in TAB_SHAPES])
def test_tables_log_sign(nat, shape, tables_knob):
    m, u = shape
    zero_row = u - 1 if u >= 2 else None
    with knob(nat, "GG_GRIEF_TABLES", tables_knob):
        for n in (1, 17, 83):
            for kind in KINDS:
                for ls in TAB_LS:
                    x, xg, q, X, A = R.tables_problem(kind, ls, m, u, n, TAB_VAR, zero_row)
                    Lg, Sg = run_tables(nat, kind, TAB_VAR, ls, x, xg, q, True)
                    check_log_sign("gg_grief_tables log/sign", Lg, Sg, X, R.tables_bound(m, A), q,
                                   "m %d u %d n %d kind %d ls %g" % (m, u, n, kind, ls))


def tables_delta_problem(m, u, n):
    rng = np.random.default_rng(m + u + n)
    xg = np.linspace(0.0, 1.0, m)
    x = rng.random(n)
    on = rng.integers(0, m, n)
    x[::2] = xg[on[::2]]                     # every other point exactly on the grid
    return x, xg, R.orth_rows(m, u, 3 * m + u), on


@pytest.mark.parametrize("shape", [(3, 2), (24, 17), (M_MFMA + 1, 5), (M_QUAD + 1, 18)],
                         ids=lambda s: "m%d_u%d" % s)
def test_tables_delta_rbf(nat, shape):
    """l = 1e-7 (the lane-quad kernels at every m): X[u][a] = var qsel[u][k]
    exactly where x[a] == xg[k], exactly 0 elsewhere."""
    m, u = shape
    assert tables_route(0, 1e-7, m, False).startswith("quad")
    with knob(nat, "GG_GRIEF_TABLES", None):
        for n in (1, 17, 83):
            x, xg, q, on = tables_delta_problem(m, u, n)
            got, _ = run_tables(nat, 0, TAB_VAR, 1e-7, x, xg, q, False)
            hit = x[None, :] == xg[:, None]                      # m x n
            assert hit[:, ::2].sum() >= (n + 1) // 2
            want = np.zeros((u, n))
            for k, a in zip(*np.nonzero(hit)):
                want[:, a] += TAB_VAR * q[:, k]
            assert np.array_equal(got, want), (m, u, n)


ALL_CASES = {
    "mixed": dict(kinds=[0, 3, 1], ms=[24, 7, 64], us=[5, 7, 33], ls=[0.3, 0.05, 0.3]),
    "one_large": dict(kinds=[2, 0, 1], ms=[24, M_MFMA + 20, 7], us=[17, 5, 3], ls=[0.3, 0.3, 0.05]),
    "nf17": dict(kinds=[f % 4 for f in range(17)], ms=[3] * 17, us=[2] * 17,
                 ls=[0.05 if f % 2 else 0.3 for f in range(17)]),
}


def all_problem(name, n):
    """x (n x nf), per-factor (xg, qsel), the col0 of every factor (5 gap
    columns spread between them) and U = sum(u) + 5."""
    c = ALL_CASES[name]
    nf = len(c["ms"])
    rng = np.random.default_rng(1000 * nf + n)
    x = rng.random((n, nf))
    xgs = [np.linspace(0.0, 1.0, m) for m in c["ms"]]
    qs = [R.orth_rows(m, u, 7 * f + m) for f, (m, u) in enumerate(zip(c["ms"], c["us"]))]
    gap_before = [1 if f in (0, nf // 3, 2 * nf // 3) else 0 for f in range(nf)]
    col0s, col = [], 0
    for f in range(nf):
        col += gap_before[f]
        col0s.append(col)
        col += c["us"][f]
    return x, xgs, qs, col0s, col + 2


def call_tables_all(nat, c, npts, xb, stride, offs, gbs, qbs, lb, sb, Ut, cols, **over):
    nf = len(c["ms"])
    a = dict(nf=nf, kinds=(ctypes.c_int * nf)(*c["kinds"]),
             vars=(ctypes.c_double * nf)(*[TAB_VAR] * nf), ls=(ctypes.c_double * nf)(*c["ls"]),
             x=xb.ptr(), x_stride=stride, xoffs=(ctypes.c_int64 * nf)(*offs), n=npts,
             xgs=(ctypes.c_void_p * nf)(*[g.ptr().value for g in gbs]),
             ms=(ctypes.c_int * nf)(*c["ms"]),
             qs=(ctypes.c_void_p * nf)(*[q.ptr().value for q in qbs]),
             us=(ctypes.c_int * nf)(*c["us"]), l=lb.ptr(), s=sb.ptr() if sb else None, U=Ut,
             col0s=(ctypes.c_int * nf)(*cols))
    a.update(over)
    return nat.lib().gg_grief_tables_all(a["nf"], a["kinds"], a["vars"], a["ls"], a["x"],
                                         a["x_stride"], a["xoffs"], a["n"], a["xgs"], a["ms"],
                                         a["qs"], a["us"], a["l"], a["s"], a["U"], a["col0s"],
                                         nat.stream_ptr())


def all_setup(name, n):
    c = ALL_CASES[name]
    nf = len(c["ms"])
    x, xgs, qs, col0s, Ut = all_problem(name, n)
    xa = nans(n, nf + 2)                       # x_stride = d + 2, columns 1 .. d used
    xa[:, 1:nf + 1] = x
    w = np.zeros((n, Ut), dtype=bool)
    for f in range(nf):
        w[:, col0s[f]:col0s[f] + c["us"][f]] = True
    return c, nf, x, xgs, qs, col0s, Ut, xa, w


@pytest.mark.parametrize("log", [False, True], ids=["value", "log_sign"])
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_tables_all_equals_single_calls(nat, name, log):
    """gg_grief_tables_all against nf gg_grief_tables calls into tables with
    gap columns and an x of stride d + 2: bitwise equal (the same kernel on
    the same per-factor data), gaps untouched, and within the bound."""
    route = [tables_route(k, l, m, False)
             for k, l, m in zip(*[ALL_CASES[name][key] for key in ("kinds", "ls", "ms")])]
    assert (name == "one_large") == ("quad_lds" in route)
    assert (name == "nf17") == (len(route) > C["tab_max_f"])
    with knob(nat, "GG_GRIEF_TABLES", None):
        for n in (1, 17, 83):
            c, nf, x, xgs, qs, col0s, Ut, xa, w = all_setup(name, n)
            xb, gbs, qbs = Buf(xa), [Buf(g) for g in xgs], [Buf(q) for q in qs]
            lb, sb = Buf(nans(n, Ut), guard=2 * Ut), (Buf(nans(n, Ut), guard=2 * Ut) if log else None)
            st = call_tables_all(nat, c, n, xb, nf + 2, range(1, nf + 1), gbs, qbs, lb, sb, Ut, col0s)
            assert st == GG_OK, nat.last_error()
            l1, s1 = Buf(nans(n, Ut), guard=2 * Ut), (Buf(nans(n, Ut), guard=2 * Ut) if log else None)
            for f in range(nf):
                st = nat.lib().gg_grief_tables(
                    c["kinds"][f], TAB_VAR, c["ls"][f], xb.ptr(1 + f), nf + 2, n, gbs[f].ptr(),
                    c["ms"][f], qbs[f].ptr(), c["us"][f], l1.ptr(), s1.ptr() if log else None, Ut,
                    col0s[f], nat.stream_ptr())
                assert st == GG_OK, nat.last_error()
            for b in [xb] + gbs + qbs:
                b.untouched()
            La, L1 = lb.read(w), l1.read(w)
            assert not np.any(np.isnan(La[w]))
            assert np.array_equal(La[w].view(np.uint64), L1[w].view(np.uint64))
            if log:
                Sa, S1 = sb.read(w), s1.read(w)
                assert np.array_equal(Sa[w].view(np.uint64), S1[w].view(np.uint64))
            for f in range(nf):
                m, u = c["ms"][f], c["us"][f]
                X, A = R.tables_ref(c["kinds"][f], TAB_VAR, c["ls"][f], x[:, f], xgs[f], qs[f])
                sl = slice(col0s[f], col0s[f] + u)
                what = "%s n %d factor %d" % (name, n, f)
                if log:
                    check_log_sign("gg_grief_tables_all log/sign", La[:, sl].T, Sa[:, sl].T, X,
                                   R.tables_bound(m, A), qs[f], what)
                else:
                    check("gg_grief_tables_all", La[:, sl].T, X, R.tables_bound(m, A), what)


def test_tables_empty_and_errors(nat):
    """n == 0 writes nothing; every refusal comes before any launch (the
    GG_REQUIREs of gg_grief_tables / _all precede the n == 0 return and the
    dispatch) and leaves the tables untouched."""
    L, s = nat.lib(), nat.stream_ptr()
    n, m, u, Ut = 5, 6, 3, 8
    xb, gb, qb = Buf(np.linspace(0, 1, 2 * n).reshape(n, 2)), Buf(np.linspace(0, 1, m)), \
        Buf(R.orth_rows(m, u, 1))
    lb, sb = Buf(nans(n, Ut)), Buf(nans(n, Ut))

    def one(kind=0, x=xb.ptr(), n_=n, xg=gb.ptr(), m_=m, q=qb.ptr(), u_=u, l=lb.ptr(), U_=Ut, col0=2):
        return L.gg_grief_tables(kind, 1.0, 0.3, x, 2, n_, xg, m_, q, u_, l, sb.ptr(), U_, col0, s)
    assert one(n_=0) == GG_OK
    for kw in [dict(m_=0), dict(u_=0), dict(col0=Ut - u + 1), dict(col0=-1), dict(kind=-1),
               dict(kind=4), dict(x=None), dict(xg=None), dict(q=None), dict(l=None), dict(n_=-1)]:
        assert one(**kw) == GG_ERR_VALUE, kw
    c = dict(kinds=[0, 1], ms=[m, m], us=[u, u], ls=[0.3, 0.3])
    args = (nat, c, n, xb, 2, [0, 1], [gb, gb], [qb, qb], lb, sb, Ut, [0, 4])
    assert call_tables_all(*args, n=0) == GG_OK
    nf = 2
    bad = [dict(ms=(ctypes.c_int * nf)(m, 0)), dict(us=(ctypes.c_int * nf)(0, u)),
           dict(col0s=(ctypes.c_int * nf)(0, Ut - u + 1)), dict(col0s=(ctypes.c_int * nf)(-1, 4)),
           dict(xoffs=(ctypes.c_int64 * nf)(0, 2)), dict(xoffs=(ctypes.c_int64 * nf)(-1, 1)),
           dict(nf=0), dict(kinds=(ctypes.c_int * nf)(0, 4)), dict(kinds=(ctypes.c_int * nf)(-1, 0)),
           dict(x=None), dict(l=None), dict(kinds=None), dict(vars=None), dict(ls=None),
           dict(xoffs=None), dict(xgs=None), dict(ms=None), dict(qs=None), dict(us=None),
           dict(col0s=None), dict(xgs=(ctypes.c_void_p * nf)(gb.ptr().value, None)),
           dict(qs=(ctypes.c_void_p * nf)(None, qb.ptr().value))]
    for kw in bad:
        assert call_tables_all(*args, **kw) == GG_ERR_VALUE, sorted(kw)
    lb.untouched()
    sb.untouched()


# ------------------------------------------------------------ gg_grief_phi
PHI_CASES = [(1, 3, 1), (2, 9, 2), (3, 20, 255), (3, 20, 256), (3, 20, 257), (5, 40, 514),
             (8, 64, 600), (9, 30, 300), (17, 34, 258), (64, 70, 66)]
PHI_NS = (1, 31, 32, 33, 63, 64, 65, 130)
PHI_SLACK = 64        # guard rows around Phi: a store loop that ignored n stays inside them


def run_phi(nat, Lt, St, cidx, log_lam, n, p, transposed, misalign):
    """One gg_grief_phi call into a Phi between guard blocks of PHI_SLACK rows
    (of either orientation); misalign: Phi starts one double past 16 bytes."""
    Ut, d = Lt.shape[1], cidx.shape[1]
    lb, cb, gb = Buf(Lt), Buf(cidx), Buf(log_lam)
    sb = Buf(St) if St is not None else None
    ob = Buf(nans(p, n) if transposed else nans(n, p), guard=PHI_SLACK * max(n, p),
             off=1 if misalign else 0)
    assert (ob.ptr().value % 16 == 8) == bool(misalign)
    st = nat.lib().gg_grief_phi(lb.ptr(), sb.ptr() if sb else None, Ut, n, cb.ptr(), d, gb.ptr(), p,
                                int(transposed), ob.ptr(), nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    for b in (lb, cb, gb) + ((sb,) if sb else ()):
        b.untouched()
    got = ob.read()
    return np.ascontiguousarray(got.T) if transposed else got


def phi_all_routes(nat, d, Ut, p, n, T, cidx, log_lam, what):
    """Both table forms through the four routes: each within the bound of its
    own tables, and the routes of one form bit for bit equal (every kernel
    multiplies scale, factor 0, factor 1, ... in that order)."""
    L, S = R.log_tables(T)
    for form, Lt, St, Tv in (("value", T, None, T), ("log", L, S, R.log_tables_value(L, S))):
        ref = R.phi_ref(Tv, cidx, log_lam)
        bound = R.phi_bound(d, ref)
        outs = {}
        with knob(nat, "GG_PHI_PAIR", None):
            outs[phi_route(d, p, True, True, False, Ut)] = run_phi(nat, Lt, St, cidx, log_lam, n, p, 0, 0)
            outs["cols_misaligned"] = run_phi(nat, Lt, St, cidx, log_lam, n, p, 0, 1)
            outs["T"] = run_phi(nat, Lt, St, cidx, log_lam, n, p, 1, 0)
        with knob(nat, "GG_PHI_PAIR", "0"):
            outs["cols_knob"] = run_phi(nat, Lt, St, cidx, log_lam, n, p, 0, 0)
        first = None
        for route, got in sorted(outs.items()):
            check("gg_grief_phi " + form, got, ref, bound, "%s %s %s" % (what, form, route))
            if first is None:
                first = got
            assert np.array_equal(got.view(np.uint64), first.view(np.uint64)), \
                "%s %s: route %s differs bitwise" % (what, form, route)


@pytest.mark.parametrize("case", PHI_CASES, ids=lambda c: "d%d_U%d_p%d" % c)
def test_phi_routes(nat, case):
    d, Ut, p = case
    pair = d <= 8 and p % 2 == 0
    assert phi_route(d, p, True, True, False, Ut) == ("pair" if pair else "cols")
    assert phi_route(d, p, False, True, False, Ut) == "cols"
    assert phi_route(d, p, True, False, False, Ut) == "cols"
    for n in PHI_NS:
        T, cidx, log_lam = R.phi_problem(d, Ut, p, n)
        phi_all_routes(nat, d, Ut, p, n, T, cidx, log_lam, "d %d U %d p %d n %d" % (d, Ut, p, n))


@pytest.mark.parametrize("transposed", [0, 1], ids=["row_major", "transposed"])
def test_phi_u_cap(nat, transposed):
    """The largest U whose rows fit the LDS cap runs and meets the bound
    (row-major: the pair kernel and, misaligned, the 256-column kernel at
    exactly the cap); U + 1 is GG_ERR_VALUE with Phi untouched.  The caps of
    the two layouts differ."""
    d, n, p = 1, 65, 4
    cap = phi_u_cap(d, transposed)
    assert phi_u_cap(d, 0) != phi_u_cap(d, 1)
    T, cidx, log_lam = R.phi_problem(d, cap, p, n)
    ref = R.phi_ref(T, cidx, log_lam)
    with knob(nat, "GG_PHI_PAIR", None):
        for mis in ((0,) if transposed else (0, 1)):
            got = run_phi(nat, T, None, cidx, log_lam, n, p, transposed, mis)
            check("gg_grief_phi value", got, ref, R.phi_bound(d, ref), "U = cap = %d" % cap)
        T1 = np.concatenate([T, nans(n, 1)], axis=1)
        lb, cb, gb, ob = Buf(T1), Buf(cidx), Buf(log_lam), Buf(nans(n, p))
        st = nat.lib().gg_grief_phi(lb.ptr(), None, cap + 1, n, cb.ptr(), d, gb.ptr(), p,
                                    transposed, ob.ptr(), nat.stream_ptr())
        assert st == GG_ERR_VALUE
        assert "too many selected eigenvector rows" in nat.last_error()
        ob.untouched()


def test_phi_empty_and_errors(nat):
    """Every refusal precedes the launch (the two GG_REQUIREs and the LDS cap
    come first in gg_grief_phi); n == 0 writes nothing."""
    L, s = nat.lib(), nat.stream_ptr()
    n, Ut, d, p = 4, 70, 2, 6
    T, cidx, log_lam = R.phi_problem(d, Ut, p, n)
    wide = np.zeros((p, C["max_dim"] + 1), dtype=np.int32)
    lb, cb, wb, gb, ob = Buf(T), Buf(cidx), Buf(wide), Buf(log_lam), Buf(nans(n, p))

    def one(l=lb.ptr(), U_=Ut, n_=n, c=cb.ptr(), d_=d, g=gb.ptr(), p_=p, o=ob.ptr(), tr=0):
        return L.gg_grief_phi(l, None, U_, n_, c, d_, g, p_, tr, o, s)
    for tr in (0, 1):
        assert one(n_=0, tr=tr) == GG_OK
        for kw in [dict(d_=0), dict(d_=C["max_dim"] + 1, c=wb.ptr()), dict(p_=0), dict(U_=0),
                   dict(l=None), dict(c=None), dict(g=None), dict(o=None), dict(n_=-1)]:
            assert one(tr=tr, **kw) == GG_ERR_VALUE, kw
    ob.untouched()


# ----------------------------------------------------------- gg_expand_skc
SKC_CASES = [(1, 1, 1), (3, 40, 255), (3, 40, 257), (8, 7, 1000), (20, 5, 33), (2, 65536, 3)]


def run_skc(nat, X, cidx, logged):
    (Ux, n), (p, d) = X.shape, cidx.shape
    xb, cb = Buf(X), Buf(cidx)
    ob = Buf(nans(p, n), guard=256)
    sb = Buf(np.full((p, n), 7, dtype=np.int32), guard=256) if logged else None
    st = nat.lib().gg_expand_skc(xb.ptr(), Ux, n, cb.ptr(), d, p, int(logged), ob.ptr(),
                                 sb.ptr() if logged else None, nat.stream_ptr())
    assert st == GG_OK, nat.last_error()
    xb.untouched()
    cb.untouched()
    return ob.read(), (sb.read() if logged else None)


@pytest.mark.parametrize("case", SKC_CASES, ids=lambda c: "d%d_p%d_n%d" % c)
def test_expand_skc(nat, case):
    """Plain and logged; (2, 65536, 3): more eigenfunctions than gridDim.y
    holds (blockIdx.y strides over j)."""
    d, p, n = case
    X, cidx = R.expand_problem(d, p, n)
    got, _ = run_skc(nat, X, cidx, False)
    ref = R.expand_skc_ref(X, cidx, False)
    check("gg_expand_skc", got, ref, R.expand_bound(d, ref=ref), "d %d p %d n %d" % case)
    got, sg = run_skc(nat, X, cidx, True)
    ref, sref, B = R.expand_skc_ref(X, cidx, True)
    assert sg.dtype == np.int32 and np.array_equal(sg, sref)
    assert np.all(sg[:, n // 2] == 0) and np.all(got[:, n // 2] == 0.0)
    check("gg_expand_skc logged", got, ref, R.expand_bound(d, B=B), "d %d p %d n %d" % case)


def test_expand_skc_empty_and_errors(nat):
    L, s = nat.lib(), nat.stream_ptr()
    X, cidx = R.expand_problem(3, 40, 255)
    xb, cb, ob = Buf(X), Buf(cidx), Buf(nans(40, 255))
    sb = Buf(np.full((40, 255), 7, dtype=np.int32))
    assert L.gg_expand_skc(xb.ptr(), 9, 255, cb.ptr(), 3, 0, 1, ob.ptr(), sb.ptr(), s) == GG_OK
    assert L.gg_expand_skc(xb.ptr(), 9, 0, cb.ptr(), 3, 40, 1, ob.ptr(), sb.ptr(), s) == GG_OK
    assert L.gg_expand_skc(xb.ptr(), 9, 255, cb.ptr(), 3, 40, 1, ob.ptr(), None, s) == GG_ERR_VALUE
    for kw in [dict(x=None), dict(c=None), dict(o=None), dict(U_=0), dict(d_=0), dict(p_=-1),
               dict(n_=-1)]:
        a = dict(x=xb.ptr(), U_=9, n_=255, c=cb.ptr(), d_=3, p_=40, o=ob.ptr())
        a.update(kw)
        assert L.gg_expand_skc(a["x"], a["U_"], a["n_"], a["c"], a["d_"], a["p_"], 0, a["o"],
                               None, s) == GG_ERR_VALUE, kw
    ob.untouched()
    sb.untouched()


def test_report_worst_ratios():
    """Prints the worst |got - ref| / bound seen per entry point in this run."""
    for k in sorted(WORST):
        print("worst err / bound  %-36s %.4f" % (k, WORST[k]))
        assert WORST[k] <= 1.0
