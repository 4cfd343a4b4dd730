"""The Laplace likelihood C ABI (gg_lik_newton, gg_lik_response_accumulate) and
linalg.LaplaceNewton at their edges on the MI355X: the clamp at |f| = 700 and
the saturation branches, overflowed sums, every lane / alignment / argument
combination, the workspace, the refusals, and the driver paths that
test_gpu_laplace.py never walks (halving, an overflowed trial, a stall, the
cut-offs, warm starts, set_operator, precond='kron').

Reference: laplace_abi_ref.py, laplace_ref's arithmetic in long double rounded
once (held to itself on the CPU by test_laplace_abi_ref.py, which also
conditions the driver cases).  Tolerances are those of test_gpu_laplace.py:
noise 1e-14 relative; b 1e-14 (|f| + (|y| + w) / w); finite sums 1e-12 of the sum
of the absolute terms; response moments 1e-13 relative; modes 1e-6 of dense
Newton; Newton steps +-1; CG iterations 5 %.  Non-finite reference values are
matched exactly in class and sign, and no output is ever NaN.

b at the binomial rows with y = 0 and f >= 36: b = f - 1 - exp(f), while the
stated bound there is 1e-14 (f + 1) -- below half the spacing of the doubles
at b from f = 36 on (spacing 0.5, bound 3.7e-13), so only the correctly rounded
value meets it.  The kernel forms exp(f) there to 2^-64 (exp_dd) and meets it;
a reciprocal of the rounded exp(-f) was one spacing, 1.35e12 bounds, off at f
= 36, as the double-precision restatement is.
"""
import ctypes

import numpy as np
import pytest

import oracle
import laplace_ref as lr
import laplace_abi_ref as ar
from test_gpu_laplace import (SENTINEL, dev_vec, gg, host, laplace_model,  # noqa: F401
                              pass_data, rel)

pytestmark = pytest.mark.gpu

VECS = ("y", "aux", "f", "a", "noise", "b")
BIG = 1048579
CASE = ((7, 5, 3), 0.2, 1.0)


def intact(v, off, written):
    """The sentinels around a dev_vec slice (and in it, unless written)."""
    base = host(v._base)
    n = v.numel()
    keep = np.ones(base.size, dtype=bool)
    if written:
        keep[off:off + n] = False
    return bool(np.all(base[keep] == SENTINEL))


def run(gg, kind, y, aux, f, a, mask, write=True, off=(), part=np.nan):
    """gg_lik_newton on a workspace pre-filled with `part`: (status, noise, b,
    sums) on the host; the vectors named in `off` lie one double into their
    allocation.  Asserts that every sentinel around (read-only form: and in)
    the two outputs is intact."""
    import torch
    from gp_grief_amd import native
    n = f.size
    o = lambda k: 1 if k in off else 0   # noqa: E731
    yd, fd, ad = dev_vec(y, o("y")), dev_vec(f, o("f")), dev_vec(a, o("a"))
    ed = None if aux is None else dev_vec(aux, o("aux"))
    md = None if mask is None else torch.from_numpy(
        np.ascontiguousarray(mask, dtype=np.uint8)).cuda()
    nd = dev_vec(np.full(n, SENTINEL), o("noise"))
    bd = dev_vec(np.full(n, SENTINEL), o("b"))
    sums = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    parts = torch.full((native.GG_LIK_PARTIALS,), part, dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = gg.native.lib().gg_lik_newton(kind, p(yd), p(ed), p(fd), p(ad), p(md),
                                       p(nd) if write else None, p(bd) if write else None,
                                       p(sums), p(parts), n, native.stream_ptr())
    torch.cuda.synchronize()
    assert intact(nd, o("noise"), write and st == 0) and intact(bd, o("b"), write and st == 0)
    return st, host(nd).copy(), host(bd).copy(), host(sums).copy()


def bits(x, y):
    """Equal bit for bit up to the sign of NaN; here no output is NaN at all."""
    x, y = np.asarray(x), np.asarray(y)
    return bool(not np.isnan(x).any() and np.array_equal(x, y)
                and np.array_equal(np.signbit(x), np.signbit(y)))


def check(R, noise, b, sums, what, elements=True):
    """The tolerances of the module docstring against pass_ref's R; the
    figures are printed before they are asserted."""
    err = ar.pass_errors(R, noise, b, sums) if elements else \
        ar.pass_errors(R, R["noise"], R["b"], sums)
    print(what, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in err.items()})
    assert not err["nan"] and err["classes"], what
    assert err["noise"] <= ar.NOISE_RTOL, what
    assert err["b"] <= 1.0, what
    assert np.all(err["sums"] <= ar.SUM_TOL), what
    if elements:
        m = R["m"]
        assert np.all(noise[~m] == 1.0) and np.all(b[~m] == 0.0), what
    return err


# ------------------------------------------------------------ edge values
def edge_calls(kind):
    """The edge rows as the two calls they need: aux given, aux NULL."""
    E = ar.edge_points(kind)
    for given in (True, False):
        r = E["given"] == given
        yield given, E["y"][r], (E["e"][r] if given else None), E["f"][r], E["a"][r], \
            E["designated"][r]


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_edge_values(gg, lik):
    kind = lr.KINDS[lik]
    for given, y, e, f, a, des in edge_calls(kind):
        st, noise, b, sums = run(gg, kind, y, e, f, a, None)
        assert st == 0
        R = ar.pass_ref(kind, y, e, f, a)
        err = ar.pass_errors(R, noise, b, sums)
        print(lik, "aux given" if given else "aux NULL", "rows", f.size, "noise", err["noise"],
              "b over bound", err["b_reach"], "b ulps where the bound is below the spacing",
              err["b_ulps"], "on", err["below"], "rows; over the stated bound everywhere", err["b"])
        assert not np.isnan(noise).any() and not np.isnan(b).any() and not np.isnan(sums).any()
        assert ar.same_class(noise, R["noise"]) and ar.same_class(b, R["b"])
        assert err["noise"] <= ar.NOISE_RTOL
        assert err["b"] <= 1.0
        # the one non-finite reference value, matched in class and sign
        assert np.array_equal(~np.isfinite(b), des) and np.all(b[des] == np.inf)
        # the header's promise (and beyond the clamp, the noise of +-700)
        assert np.all(np.isfinite(noise)) and np.all(noise > 0)
        # |f| > 700: w and what derives from it are those of +-700, bit for bit
        fc = ar.clamped(f)
        st, nc, bc, sc = run(gg, kind, y, e, fc, a, None)
        assert st == 0
        assert bits(nc, noise) and bits(sc[2:3], sums[2:3])
        inside = np.abs(f) <= ar.CLAMP
        assert bits(bc[inside], b[inside])
        # the g / w part of b: b(f) - f = b(+-700) - (+-700) up to the two roundings
        # of each side (eps of the terms of b, of which y noise is the largest)
        fin = ~des
        eps = np.finfo(np.float64).eps
        with np.errstate(over="ignore"):
            scale = np.abs(f) + np.abs(b) + np.abs(bc) + y * noise
        gap = np.abs((b[fin] - bc[fin]) - (f[fin] - fc[fin]))
        assert np.all(gap <= 8 * eps * scale[fin])
        # ... while g and log p use f as given: the sums per value of f, both forms
        for v in np.unique(f):
            for neg in (False, True):
                r = (f == v) & (np.signbit(f) == neg)
                if not r.any():
                    continue
                ev = None if e is None else e[r]
                Rv = ar.pass_ref(kind, y[r], ev, f[r], a[r])
                st, _, _, s1 = run(gg, kind, y[r], ev, f[r], a[r], None)
                assert st == 0
                check(Rv, None, None, s1, "%s f %r rows %d" % (lik, float(f[r][0]), r.sum()),
                      elements=False)
                st, n0, b0, s0 = run(gg, kind, y[r], ev, f[r], a[r], None, write=False)
                assert st == 0 and bits(s0, s1)


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_edge_b_within_the_stated_bound(gg, lik):
    """b within 1e-14 (|f| + (|y| + w) / w) of the long-double value at every
    edge row, the 32 binomial rows included where that asks for the correctly
    rounded b (y = 0, f >= 36; module docstring)."""
    kind = lr.KINDS[lik]
    worst = 0.0
    for given, y, e, f, a, des in edge_calls(kind):
        st, noise, b, sums = run(gg, kind, y, e, f, a, None)
        assert st == 0
        err = ar.pass_errors(ar.pass_ref(kind, y, e, f, a), noise, b, sums)
        print(lik, "aux given" if given else "aux NULL", "b over the stated bound", err["b"],
              "in spacings of b on the rows below the spacing", err["b_ulps"])
        worst = max(worst, err["b"])
    assert worst <= 1.0


# ------------------------------------------------------------ overflow in the sums
@pytest.mark.parametrize("at", [0, 513, 960])
def test_overflowed_point_in_the_sums(gg, at):
    kind = lr.POISSON
    y0, e0, f0, a0, m0 = pass_data(kind, 960)
    ins = lambda v, x: np.insert(v, at, x)   # noqa: E731
    y, e, a, mask = ins(y0, 3.0), ins(e0, 1.0), ins(a0, 0.25), ins(m0, True)
    f = ins(f0, 720.0)
    st, noise, b, sums = run(gg, kind, y, e, f, a, mask)
    assert st == 0
    R = ar.pass_ref(kind, y, e, f, a, mask)
    assert R["sums"][0] == -np.inf and R["sums"][3] == np.inf and R["sums"][4] == np.inf
    check(R, noise, b, sums, "overflowed point at %d" % at)
    assert sums[0] == -np.inf and sums[3] == np.inf and sums[4] == np.inf
    assert np.isfinite(sums[1]) and np.isfinite(sums[2])
    assert np.all(np.isfinite(noise)) and np.all(np.isfinite(b))
    st, _, _, s0 = run(gg, kind, y, e, f, a, mask, write=False)
    assert st == 0 and np.array_equal(s0, sums) and not np.isnan(s0).any()
    # under a zero mask byte the point is not there: the ordinary one's outputs
    mask0 = mask.copy()
    mask0[at] = False
    out_inf = run(gg, kind, y, e, f, a, mask0)
    out_ord = run(gg, kind, y, e, ins(f0, 0.5), a, mask0)
    assert out_inf[0] == 0 and out_ord[0] == 0
    for u, v in zip(out_inf[1:], out_ord[1:]):
        assert bits(u, v)
    assert np.all(np.isfinite(out_inf[3]))


# ------------------------------------------------------------ lanes
def lane_data(kind, n):
    y, e, f, a, mask = (v[:n] for v in pass_data(kind, 960))
    return y, e, f, a, mask


@pytest.mark.parametrize("n", [1, 2, 3, 513, 514, 960])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_lanes(gg, lik, n):
    kind = lr.KINDS[lik]
    y, e, f, a, mask = lane_data(kind, n)
    R = ar.pass_ref(kind, y, e, f, a, mask)
    st, noise, b, wide = run(gg, kind, y, e, f, a, mask)
    assert st == 0
    check(R, noise, b, wide, "%s n %d aligned" % (lik, n))
    st, _, _, s0 = run(gg, kind, y, e, f, a, mask, write=False)
    assert st == 0 and bits(s0, wide)
    for off in [(v,) for v in VECS] + [VECS]:
        st, n1, b1, s1 = run(gg, kind, y, e, f, a, mask, off=off)
        assert st == 0, off
        # 8-byte lanes: the element outputs bit for bit, the sums to tolerance
        assert bits(n1, noise) and bits(b1, b), off
        check(R, n1, b1, s1, "%s n %d off %s" % (lik, n, "+".join(off)))
        # read-only: the outputs do not count towards the lane width
        st, _, _, s2 = run(gg, kind, y, e, f, a, mask, write=False, off=off)
        narrow = bool(set(off) & {"y", "aux", "f", "a"})
        assert st == 0 and bits(s2, s1 if narrow else wide), off


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_scalar_path_grid_stride(gg, lik):
    """n = 1048579 on 8-byte lanes: 2048 workgroups, each thread several points."""
    kind = lr.KINDS[lik]
    y, e, f, a, mask = pass_data(kind, BIG)
    R = ar.pass_ref(kind, y, e, f, a, mask)
    st, noise, b, sums = run(gg, kind, y, e, f, a, mask, off=("f",))
    assert st == 0
    check(R, noise, b, sums, "%s n %d off f" % (lik, BIG))
    st, _, _, s0 = run(gg, kind, y, e, f, a, mask, write=False, off=("f",))
    assert st == 0 and bits(s0, sums)


# ------------------------------------------------------------ combinations
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_mask_and_aux_combinations(gg, lik):
    kind = lr.KINDS[lik]
    y, e, f, a, mask = lane_data(kind, 105)
    y1 = np.minimum(y, 1.0) if kind == lr.BINOMIAL else y     # aux NULL: one trial
    for what, yy, ee, mm in (("mask, aux NULL", y1, None, mask), ("aux, mask NULL", y, e, None)):
        st, noise, b, sums = run(gg, kind, yy, ee, f, a, mm)
        assert st == 0
        check(ar.pass_ref(kind, yy, ee, f, a, mm), noise, b, sums, lik + " " + what)
        st, _, _, s0 = run(gg, kind, yy, ee, f, a, mm, write=False)
        assert st == 0 and bits(s0, sums)
    # nothing observed
    none = np.zeros(105, dtype=bool)
    for write in (True, False):
        st, noise, b, sums = run(gg, kind, y, e, f, a, none, write=write)
        assert st == 0 and np.all(sums == 0.0) and not np.signbit(sums).any()
        if write:
            assert np.all(noise == 1.0) and np.all(b == 0.0)
    # NaN in every input at the missing points changes no bit of any output
    ref = run(gg, kind, y, e, f, a, mask)
    nan = lambda v: np.where(mask, v, np.nan)   # noqa: E731
    for off in ((), ("b",)):
        out = run(gg, kind, nan(y), nan(e), nan(f), nan(a), mask, off=off)
        assert out[0] == 0 and bits(out[1], ref[1]) and bits(out[2], ref[2])
        if not off:
            assert bits(out[3], ref[3])
        ro = run(gg, kind, nan(y), nan(e), nan(f), nan(a), mask, write=False, off=off)
        assert ro[0] == 0 and bits(ro[3], ref[3])    # b's offset does not narrow the lanes


@pytest.mark.parametrize("n", [1, 960])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_workspace_contents_do_not_matter(gg, lik, n):
    kind = lr.KINDS[lik]
    y, e, f, a, mask = lane_data(kind, n)
    R = ar.pass_ref(kind, y, e, f, a, mask)
    outs = [run(gg, kind, y, e, f, a, mask, part=part) for part in (np.nan, np.nan, 1e300, 0.0)]
    check(R, outs[0][1], outs[0][2], outs[0][3], "%s n %d, NaN workspace" % (lik, n))
    for o in outs[1:]:
        assert o[0] == 0 and bits(o[3], outs[0][3])


def test_alignment_and_workspace_refusals(gg):
    import torch
    from gp_grief_amd import native
    L = gg.native.lib()
    n = 105
    y, e, f, a, mask = lane_data(lr.POISSON, n)
    yd, ed, fd, ad = dev_vec(y), dev_vec(e), dev_vec(f), dev_vec(a)
    md = torch.from_numpy(mask.astype(np.uint8)).cuda()
    nd, bd = dev_vec(np.full(n, SENTINEL)), dev_vec(np.full(n, SENTINEL))
    sums = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    part = torch.full((native.GG_LIK_PARTIALS + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    names = ["kind", "y", "aux", "f", "a", "mask", "noise", "b", "sums", "part", "n"]
    tens = dict(y=yd, aux=ed, f=fd, a=ad, mask=md, noise=nd, b=bd, sums=sums, part=part)
    good = dict(kind=0, n=n)
    good.update({k: ctypes.c_void_p(t.data_ptr()) for k, t in tens.items()})

    def call(**kw):
        args = dict(good)
        args.update(kw)
        return L.gg_lik_newton(*([args[k] for k in names] + [native.stream_ptr()]))

    def untouched():
        torch.cuda.synchronize()
        return (intact(nd, 0, False) and intact(bd, 0, False)
                and bool(np.all(host(sums) == SENTINEL)) and bool(np.all(host(part) == SENTINEL)))

    # an address that is 4 mod 8 holds no double (refused before any launch)
    for k in ("y", "aux", "f", "a", "noise", "b", "sums", "part"):
        bad = ctypes.c_void_p(tens[k].data_ptr() + 4)
        assert call(**{k: bad}) == native.GG_ERR_VALUE, k
        if k not in ("noise", "b"):
            assert call(**{"noise": None, "b": None, k: bad}) == native.GG_ERR_VALUE, k
    assert call(part=None) == native.GG_ERR_VALUE
    assert call(part=None, noise=None, b=None) == native.GG_ERR_VALUE
    assert untouched()
    # the mask is bytes: any address
    m2 = torch.from_numpy(np.concatenate([[0], mask]).astype(np.uint8)).cuda()
    assert call(mask=ctypes.c_void_p(m2.data_ptr() + 1)) == 0
    torch.cuda.synchronize()
    ref = run(gg, lr.POISSON, y, e, f, a, mask)
    assert bits(host(nd), ref[1]) and bits(host(bd), ref[2]) and bits(host(sums)[:5], ref[3])
    assert np.all(host(sums)[5:] == SENTINEL) and host(part)[-1] == SENTINEL
    # n == 0 needs no workspace: the sums are zeroed, nothing else is written
    nd.fill_(SENTINEL)
    bd.fill_(SENTINEL)
    sums.fill_(SENTINEL)
    assert call(part=None, n=0) == 0
    torch.cuda.synchronize()
    assert np.all(host(sums)[:5] == 0.0) and np.all(host(sums)[5:] == SENTINEL)
    assert intact(nd, 0, False) and intact(bd, 0, False)


# ------------------------------------------------------------ response moments
def accumulate(gg, kind, F, W, off=()):
    """gg_lik_response_accumulate over the draws F[k] + W[k]: (mean, m2) on the
    host, the moments starting as NaN; asserts the sentinels around them."""
    import torch
    from gp_grief_amd import native
    L = gg.native.lib()
    n = F.shape[1]
    o = lambda k: 1 if k in off else 0   # noqa: E731
    mean, m2 = dev_vec(np.full(n, np.nan), o("mean")), dev_vec(np.full(n, np.nan), o("m2"))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for k in range(1, F.shape[0] + 1):
        fd, wd = dev_vec(F[k - 1], o("f")), dev_vec(W[k - 1], o("w"))
        assert L.gg_lik_response_accumulate(kind, p(fd), p(wd), p(mean), p(m2), k, n,
                                            native.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert intact(mean, o("mean"), True) and intact(m2, o("m2"), True)
    return host(mean).copy(), host(m2).copy()


def check_response(kind, F, W, mean, m2, what):
    rm, rq, same = ar.response_ref(kind, F, W)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(m2)), what
    # one denormal step is the precision of the format at exp(-745)
    em = np.abs(mean - rm) / np.maximum(np.abs(rm), 1e-300)
    em[np.abs(mean - rm) <= 5e-324] = 0.0
    nz = ~same & (rq != 0)
    eq = np.abs(m2 - rq)[nz] / rq[nz]
    print(what, "mean", em.max(), "m2", eq.max() if eq.size else 0.0, "equal points", same.sum())
    assert np.all(em <= 1e-13), what
    assert np.all(eq <= 1e-13), what
    assert np.all(m2[same] == 0.0), what
    # a reference m2 that underflowed (responses near exp(-700), squared)
    assert np.all(m2[~same & (rq == 0)] <= 5e-324), what


@pytest.mark.parametrize("n", [1, 2, 3, 513, 514])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_response_lanes_and_values(gg, lik, n):
    kind = lr.KINDS[lik]
    F, W = ar.response_values(kind, n)
    mean, m2 = accumulate(gg, kind, F, W)
    check_response(kind, F, W, mean, m2, "%s n %d" % (lik, n))
    for v in ("f", "w", "mean", "m2"):
        m1, q1 = accumulate(gg, kind, F, W, off=(v,))
        assert bits(m1, mean) and bits(q1, m2), v


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_response_grid_stride(gg, lik):
    kind = lr.KINDS[lik]
    F, W = ar.response_values(kind, BIG)
    mean, m2 = accumulate(gg, kind, F, W)
    check_response(kind, F, W, mean, m2, "%s n %d" % (lik, BIG))
    m1, q1 = accumulate(gg, kind, F, W, off=("mean",))
    assert bits(m1, mean) and bits(q1, m2)


# ------------------------------------------------------------ the driver
def driver(gg, C, F=None, **kw):
    """linalg.LaplaceNewton on a case (cg_rtol 1e-11 unless given)."""
    K = gg.tensors.KronMatrix(list(C["F"] if F is None else F), sym=True)
    kw.setdefault("cg_rtol", 1e-11)
    lik = "poisson" if C["kind"] == lr.POISSON else "binomial"
    return gg.linalg.LaplaceNewton(K, C["y"].copy(), lik, aux=C["aux"], mask=C["mask"],
                                   const=lr.log_norm(C["kind"], C["y"], C["aux"], C["mask"]), **kw)


def test_driver_halves_the_step(gg):
    C = ar.driver_case("halving")
    D, R = ar.driver_run("halving", solve="dense"), ar.driver_run("halving")
    nt = driver(gg, C)
    nt.mode()
    print("halvings device", nt.halvings, "reference", R["halvings"], "newton", nt.newton_iters,
          R["iters"], "a err", rel(host(nt.a), D["a"]))
    assert R["converged"] and max(R["halvings"]) >= 1
    assert nt.newton_converged and not nt.newton_stalled
    for i, h in enumerate(R["halvings"]):
        if h >= 1:
            assert nt.halvings[i] == h
    assert abs(nt.newton_iters - R["iters"]) <= 1 and len(nt.halvings) == nt.newton_iters
    assert rel(host(nt.a), D["a"]) < 1e-6 and rel(host(nt.f), D["f"]) < 1e-6


def test_driver_rejects_an_overflowed_trial(gg):
    C = ar.driver_case("overflow")
    D, R = ar.driver_run("overflow", solve="dense"), ar.driver_run("overflow")
    assert not np.all(np.isfinite(ar.first_trial_sums("overflow"))) and R["converged"]
    nt = driver(gg, C)
    nt.mode()
    print("halvings device", nt.halvings, "reference", R["halvings"], "dense", D["halvings"],
          "converged", nt.newton_converged, "stalled", nt.newton_stalled,
          "a err", rel(host(nt.a), D["a"]))
    assert nt.halvings[0] == R["halvings"][0] >= 1
    for v in (nt.a, nt.f, nt.noise, nt.b):
        assert np.all(np.isfinite(host(v)))
    assert np.isfinite(nt.psi) and np.all(np.isfinite(nt.sums))
    assert rel(host(nt.a), D["a"]) < 1e-6


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_driver_stalls_below_the_resolution_of_psi(gg, lik):
    ms, frac, amp = CASE
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    S = lr.mode(ms, frac, amp, lik, solve="cg", cg_rtol=1e-11, newton_tol=1e-14)
    assert S["stalled"] and not S["converged"] and S["iters"] < 50
    nt = driver(gg, C, newton_tol=1e-14)
    nt.mode()
    print(lik, "device steps", nt.newton_iters, "halvings", nt.halvings, "reference", S["iters"],
          S["halvings"], "a err", rel(host(nt.a), D["a"]))
    assert nt.newton_stalled and not nt.newton_converged and nt.newton_iters < nt.max_newton
    assert rel(host(nt.a), D["a"]) < 1e-6
    m = laplace_model(gg, ms, amp, lik, C, newton_tol=1e-14)
    m.fit()
    assert m.newton_stalled and not m.newton_converged
    assert rel(host(m._alpha), D["a"]) < 1e-6


def test_driver_cut_offs(gg):
    C = ar.driver_case("halving")
    D = ar.driver_run("halving", solve="dense")
    nt = driver(gg, C, max_newton=2)
    nt.mode()
    assert nt.newton_iters == 2 and len(nt.cg_iters) == 2 and len(nt.halvings) == 2
    assert not nt.newton_converged and not nt.newton_stalled
    nt.max_newton = 50
    nt.mode(a0=nt.a)
    assert nt.newton_converged and rel(host(nt.a), D["a"]) < 1e-6
    h0 = driver(gg, C, max_halvings=0)
    h0.mode()
    assert h0.newton_stalled and not h0.newton_converged and h0.newton_iters == 0
    assert h0.halvings == [] and len(h0.cg_iters) == 1
    assert np.all(host(h0.a) == 0.0)


def test_driver_warm_start_hygiene(gg):
    C = ar.driver_case("halving")
    m = C["mask"]
    a0 = ar.driver_run("halving", max_newton=2)["a"]
    nt = driver(gg, C)
    modes = []
    for fill in (0.0, np.nan, 7.0):
        nt.mode(a0=np.where(m, a0, fill))
        assert nt.newton_converged
        a = host(nt.a).copy()
        assert np.all(a[~m] == 0.0) and not np.signbit(a[~m]).any()
        modes.append((a, nt.newton_iters, list(nt.halvings)))
    for a, iters, halvings in modes[1:]:
        assert bits(a, modes[0][0]) and iters == modes[0][1] and halvings == modes[0][2]
    with pytest.raises(ValueError):
        nt.mode(a0=np.zeros(104))


def test_driver_set_operator(gg):
    C = ar.driver_case("halving")
    F2 = lr.factors(ar.GRID, 1.0, ls=0.15)
    D2 = lr.newton(F2, C["kind"], C["y"], C["aux"], C["mask"], solve="dense")
    assert D2["converged"]
    nt = driver(gg, C)
    nt.mode()
    first = host(nt.a).copy()
    nt.set_operator(gg.tensors.KronMatrix(list(F2), sym=True))
    nt.mode(a0=nt.a)
    fresh = driver(gg, C, F=F2)
    fresh.mode()
    print("other lengthscales: moved", rel(first, D2["a"]), "warm", rel(host(nt.a), D2["a"]),
          "fresh", rel(host(fresh.a), D2["a"]))
    assert nt.newton_converged and fresh.newton_converged
    assert rel(first, D2["a"]) > 1e-3          # the operators do differ
    assert rel(host(nt.a), host(fresh.a)) < 1e-6 and rel(host(nt.a), D2["a"]) < 1e-6
    assert rel(host(nt.f), oracle.kron_matvec(F2, host(nt.a))) < 1e-12
    with pytest.raises(ValueError):
        nt.set_operator(gg.tensors.KronMatrix(list(lr.factors((7, 5, 2))), sym=True))


@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_driver_with_the_kron_preconditioner(gg, lik):
    ms, frac, amp = CASE
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    P = lr.mode(ms, frac, amp, lik, solve="cg", cg_rtol=1e-11, precond="kron")
    nt = driver(gg, C, precond="kron")
    nt.mode()
    print(lik, "cg", nt.cg_iters, "reference", P["cg_iters"], "a err", rel(host(nt.a), D["a"]))
    assert nt.newton_converged and rel(host(nt.a), D["a"]) < 1e-6
    assert abs(nt.newton_iters - P["iters"]) <= 1
    for it, itref in zip(nt.cg_iters, P["cg_iters"]):
        assert abs(it - itref) <= 0.05 * itref, (nt.cg_iters, P["cg_iters"])


def test_model_warns_outside_the_documented_exposure_range(gg, caplog):
    import logging
    ms, frac, amp = CASE
    C = lr.case(ms, frac, amp, "poisson")
    io = int(np.nonzero(C["mask"])[0][0])
    with caplog.at_level(logging.WARNING, logger="gp_grief_amd.models"):
        laplace_model(gg, ms, amp, "poisson", C)
        assert not [r for r in caplog.records if "outside [1e-4, 1e4]" in r.getMessage()]
        for bad in (5e-5, 2e4):
            caplog.clear()
            aux = C["aux"].copy()
            aux[io] = bad
            out = np.where(C["mask"], 1.0, bad)      # a missing point's value is not looked at
            laplace_model(gg, ms, amp, "poisson", dict(C, aux=C["aux"] * out))
            assert not caplog.records
            laplace_model(gg, ms, amp, "poisson", dict(C, aux=aux))
            assert [r for r in caplog.records if "outside [1e-4, 1e4]" in r.getMessage()], bad
