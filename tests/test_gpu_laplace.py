"""Poisson / binomial likelihoods on the MI355X: the fused Newton pass
(gg_lik_newton), the response moments (gg_lik_response_accumulate), the
Newton driver and GPGridLaplaceModel against the NumPy restatement in
laplace_ref.py (itself held to dense Newton on the CPU, test_laplace_ref.py)
and dense algebra.

Pass tolerances (device exp / log1p within an ulp of NumPy's): noise 1e-14
relative; b 1e-14 (|f| + (|y| + w) / w) per element; each sum 1e-12 of the sum of
its absolute terms.  The element outputs are compared with laplace_ref's
long-double evaluation rounded once, so the reference's own rounding does not
use up the bound (measured at n = 1048579: noise 7e-16, b 0.87 of its bound
for the binomial -- where y = 0 and f is near 6, b = f - 1 - exp(f) and the bound
is 1.2 ulp of b -- and 0.04 for the Poisson; sums 4e-16).  Mode 1e-6 of dense Newton at newton_tol 1e-8, cg_rtol
1e-11; Newton steps +-1 and CG iterations 5 % of the restatement's; psi and sum
log w 1e-8; per-probe SLQ estimates 1e-5 |log det| (test_gpu_noise.py) and the
SLQ mean within 4 standard errors of the dense log det; sampled means within
6 standard errors of the dense Laplace posterior's law
(test_gpu_posterior_sample.py).
"""
import ctypes

import numpy as np
import pytest

import laplace_ref as lr
import noise_ref as nr

pytestmark = pytest.mark.gpu

ALL = [(ms, frac, amp, lik) for (ms, frac, amp) in lr.CASES for lik in lr.LIKELIHOODS]
SIZES = [1, 2, 105, 960, 1048579]
SENTINEL = -12345.678


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    return gp_grief_amd


# ------------------------------------------------------------ the pass
_data = {}


def pass_data(kind, n):
    """(y, aux, f, a, mask): f uniform in [-6, 6], a normal; Poisson counts
    with exposure exp(U(log .5, log 4)), binomial y uniform on 0..t with t in
    1..5; about a fifth of the points missing.  Once per (kind, n)."""
    if (kind, n) not in _data:
        rng = np.random.default_rng(100 + kind)
        f = rng.uniform(-6.0, 6.0, n)
        a = rng.standard_normal(n)
        if kind == lr.POISSON:
            aux = np.exp(rng.uniform(np.log(0.5), np.log(4.0), n))
            y = rng.poisson(3.0, n).astype(np.float64)
        else:
            aux = rng.integers(1, 6, n).astype(np.float64)
            y = np.floor(rng.uniform(0, 1, n) * (aux + 1))
        mask = rng.uniform(0, 1, n) > 0.2
        mask[0] = True
        _data[(kind, n)] = (y, aux, f, a, mask)
    return _data[(kind, n)]


def dev_vec(x, off=0):
    """x on the device, `off` doubles into a 16-byte aligned allocation."""
    import torch
    buf = torch.full((x.size + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + x.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
    return v


def run_pass(gg, kind, y, aux, f, a, mask, write=True, off=()):
    """gg_lik_newton: (status, noise, b, sums) on the host; the vectors named
    in `off` lie one double into their allocation."""
    import torch
    from gp_grief_amd import native
    n = f.size
    o = lambda k: 1 if k in off else 0   # noqa: E731
    yd, fd, ad = dev_vec(y, o("y")), dev_vec(f, o("f")), dev_vec(a, o("a"))
    ed = None if aux is None else dev_vec(aux, o("aux"))
    md = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda()
    nd = dev_vec(np.full(n, SENTINEL), o("noise"))
    bd = dev_vec(np.full(n, SENTINEL), o("b"))
    sums = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    part = torch.empty(native.GG_LIK_PARTIALS, dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    st = gg.native.lib().gg_lik_newton(kind, p(yd), p(ed), p(fd), p(ad), p(md),
                                       p(nd) if write else None, p(bd) if write else None,
                                       p(sums), p(part), n, native.stream_ptr())
    torch.cuda.synchronize()
    return st, host(nd).copy(), host(bd).copy(), host(sums).copy()


def check_pass(kind, y, aux, f, a, mask, noise, b, sums):
    n = f.size
    rn, rb, rs, rabs = lr.newton_pass(kind, y, aux, f, a, mask, precise=True)
    m = np.ones(n, dtype=bool) if mask is None else mask
    e = np.ones(n) if aux is None else aux
    _, _, w, _, _ = lr.point(kind, np.where(m, y, 0.0), np.where(m, e, 1.0), f)
    en = np.max(np.abs(noise[m] - rn[m]) / rn[m])
    bound = 1e-14 * (np.abs(f) + (np.abs(y) + w) / w)
    eb = np.max((np.abs(b - rb) / bound)[m])
    es = np.abs(sums - rs) / np.maximum(rabs, 1e-300)
    print("kind", kind, "n", n, "noise rel", en, "b err / bound", eb, "sums", es)
    assert en <= 1e-14
    assert eb <= 1.0
    assert np.all(es <= 1e-12)
    assert np.all(noise[~m] == 1.0) and np.all(b[~m] == 0.0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("full", [False, True], ids=["mask-aux", "plain"])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_pass_matches_restatement(gg, lik, full, n):
    kind = lr.KINDS[lik]
    y, aux, f, a, mask = pass_data(kind, n)
    if full:
        aux, mask = None, None
        if kind == lr.BINOMIAL:
            y = np.minimum(y, 1.0)
    st, noise, b, sums = run_pass(gg, kind, y, aux, f, a, mask)
    assert st == 0
    check_pass(kind, y, aux, f, a, mask, noise, b, sums)
    # the read-only form: the same sums bit for bit, nothing written
    st, n2, b2, s2 = run_pass(gg, kind, y, aux, f, a, mask, write=False)
    assert st == 0
    assert np.array_equal(s2, sums)
    assert np.all(n2 == SENTINEL) and np.all(b2 == SENTINEL)


@pytest.mark.parametrize("n", [105, 960])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_pass_unaligned_streams_and_nan_at_missing_points(gg, lik, n):
    kind = lr.KINDS[lik]
    y, aux, f, a, mask = pass_data(kind, n)
    st, noise, b, sums = run_pass(gg, kind, y, aux, f, a, mask)
    assert st == 0
    for name in ("y", "f", "noise"):
        st, n1, b1, s1 = run_pass(gg, kind, y, aux, f, a, mask, off=(name,))
        assert st == 0
        # 8-byte lanes: the element outputs bit for bit, the sums as the pass
        assert np.array_equal(n1, noise) and np.array_equal(b1, b)
        check_pass(kind, y, aux, f, a, mask, n1, b1, s1)
    # NaN in y / aux at the missing points changes no bit of any output
    st, n2, b2, s2 = run_pass(gg, kind, np.where(mask, y, np.nan), np.where(mask, aux, np.nan),
                              f, a, mask)
    assert st == 0
    assert np.array_equal(n2, noise) and np.array_equal(b2, b) and np.array_equal(s2, sums)


def test_pass_refusals_leave_outputs_untouched(gg):
    import torch
    from gp_grief_amd import native
    L = gg.native.lib()
    n = 105
    y, aux, f, a, mask = pass_data(lr.POISSON, n)
    yd, ed, fd, ad = dev_vec(y), dev_vec(aux), dev_vec(f), dev_vec(a)
    md = torch.from_numpy(mask.astype(np.uint8)).cuda()
    nd, bd = dev_vec(np.full(n, SENTINEL)), dev_vec(np.full(n, SENTINEL))
    sums = torch.full((5,), SENTINEL, dtype=torch.float64, device="cuda")
    part = torch.empty(native.GG_LIK_PARTIALS, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    sp = native.stream_ptr()
    good = [0, p(yd), p(ed), p(fd), p(ad), p(md), p(nd), p(bd), p(sums), p(part), n, sp]

    def call(**kw):
        args = list(good)
        names = ["kind", "y", "aux", "f", "a", "mask", "noise", "b", "sums", "part", "n"]
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.gg_lik_newton(*args)

    for bad in (dict(kind=2), dict(kind=-1), dict(y=None), dict(f=None), dict(a=None),
                dict(sums=None), dict(n=-1), dict(noise=None), dict(b=None)):
        assert call(**bad) == native.GG_ERR_VALUE, bad
    torch.cuda.synchronize()
    assert np.all(host(nd) == SENTINEL) and np.all(host(bd) == SENTINEL)
    assert np.all(host(sums) == SENTINEL)
    # n == 0 zeroes the sums and writes nothing else
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert np.all(host(sums) == 0.0)
    assert np.all(host(nd) == SENTINEL) and np.all(host(bd) == SENTINEL)


# ------------------------------------------------------------ response moments
@pytest.mark.parametrize("n", [105, 960])
@pytest.mark.parametrize("lik", lr.LIKELIHOODS)
def test_response_accumulate(gg, lik, n):
    import torch
    from gp_grief_amd import native
    L = gg.native.lib()
    kind = lr.KINDS[lik]
    rng = np.random.default_rng(7)
    S = 5
    F, W = rng.standard_normal((S, n)), rng.standard_normal((S, n))
    mean = dev_vec(np.full(n, np.nan))        # k == 1 overwrites garbage
    m2 = dev_vec(np.full(n, np.nan))
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rm, rq = np.zeros(n), np.zeros(n)
    for k in range(1, S + 1):
        fd, wd = dev_vec(F[k - 1]), dev_vec(W[k - 1])
        assert L.gg_lik_response_accumulate(kind, p(fd), p(wd), p(mean), p(m2), k, n,
                                            native.stream_ptr()) == 0
        x = F[k - 1] + W[k - 1]
        r = np.exp(x) if kind == lr.POISSON else 1.0 / (1.0 + np.exp(-x))
        d = r - rm
        rm = rm + d / k
        rq = rq + d * (r - rm)
    torch.cuda.synchronize()
    assert np.max(np.abs(host(mean) - rm) / np.abs(rm)) <= 1e-13
    assert np.max(np.abs(host(m2) - rq) / np.abs(rq)) <= 1e-13
    before = (host(mean).copy(), host(m2).copy())
    fd, wd = dev_vec(F[0]), dev_vec(W[0])
    for args in ((2, p(fd), p(wd), p(mean), p(m2), 1, n), (kind, None, p(wd), p(mean), p(m2), 1, n),
                 (kind, p(fd), None, p(mean), p(m2), 1, n), (kind, p(fd), p(wd), None, p(m2), 1, n),
                 (kind, p(fd), p(wd), p(mean), None, 1, n), (kind, p(fd), p(wd), p(mean), p(m2), 0, n),
                 (kind, p(fd), p(wd), p(mean), p(m2), 1, -1)):
        assert L.gg_lik_response_accumulate(*args, native.stream_ptr()) == native.GG_ERR_VALUE
    torch.cuda.synchronize()
    assert np.array_equal(host(mean), before[0]) and np.array_equal(host(m2), before[1])


# ------------------------------------------------------------ the model
def laplace_model(gg, ms, amp, lik, C, dev_y=False, **kw):
    """GPGridLaplaceModel whose operator has laplace_ref.factors(ms, amp)
    (cov_grid reverses the input dimensions: input j is factor d - 1 - j)."""
    d = len(ms)
    ls = [0.1 * (1 + 0.05 * i) for i in range(d)]
    var = [float(amp) ** 2 if i == 0 else 1.0 for i in range(d)]
    kerns = [gg.kern.RBF(1, variance=var[d - 1 - j], lengthscale=ls[d - 1 - j])
             for j in range(d)]
    xg = [np.linspace(0, 1, ms[d - 1 - j]).reshape(-1, 1) for j in range(d)]
    Y = C["y"].reshape(-1, 1).copy()
    if dev_y:
        import torch
        Y = torch.from_numpy(Y).cuda()
    aux = {"exposure" if lik == "poisson" else "trials": C["aux"]}
    kw.setdefault("cg_rtol", 1e-11)
    kw.setdefault("newton_tol", 1e-8)
    mask = None if C["mask"].all() else C["mask"]
    return gg.models.GPGridLaplaceModel(xg, Y, gg.kern.GridKernel(kerns), lik, mask=mask,
                                        **aux, **kw)


_models = {}


def fitted(gg, ms, frac, amp, lik):
    key = (tuple(ms), frac, amp, lik)
    if key not in _models:
        m = laplace_model(gg, ms, amp, lik, lr.case(ms, frac, amp, lik))
        m.fit()
        _models[key] = m
    return _models[key]


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_mode_matches_dense_newton(gg, ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    R = lr.mode(ms, frac, amp, lik, solve="cg", cg_rtol=1e-11)
    m = fitted(gg, ms, frac, amp, lik)
    a = host(m._alpha)
    fhat = m.predict_grid(compute_var=False)[0][:, 0]
    print(lik, ms, frac, "newton", m.newton_iters, "ref", R["iters"], "cg", m.cg_iters, "ref",
          R["cg_iters"], "a err", rel(a, D["a"]), "f err", rel(fhat, D["f"]))
    assert m.newton_converged and not m.newton_stalled
    assert rel(a, D["a"]) < 1e-6 and rel(fhat, D["f"]) < 1e-6
    assert np.all(a[~C["mask"]] == 0)
    assert abs(m.newton_iters - R["iters"]) <= 1
    assert len(m.cg_iters) == m.newton_iters
    for it, itref in zip(m.cg_iters, R["cg_iters"]):
        assert abs(it - itref) <= 0.05 * itref, (m.cg_iters, R["cg_iters"])
    # predict_grid(compute_var=False) is K a^
    assert rel(fhat, lr.oracle.kron_matvec(C["F"], a)) < 1e-12
    # a warm start from the mode takes no Newton step
    nt = m._newton
    nt.mode(a0=nt.a)
    assert nt.newton_iters == 0 and nt.newton_converged and nt.cg_iters == []


@pytest.mark.parametrize("ms,frac,amp,lik", ALL)
def test_laplace_lml(gg, ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    m = fitted(gg, ms, frac, amp, lik)
    ll = float(np.squeeze(m.log_likelihood()))
    dense_ld = nr.dense_logdet(C["F"], C["mask"], D["noise"])
    _, ref_ests = nr.weighted_slq(C["F"], C["mask"], D["noise"], probes=8, steps=50, seed=0)
    ests = m.slq_estimates
    se = ests.std(ddof=1) / np.sqrt(ests.size)
    print(lik, ms, frac, "psi", m.psi, D["psi"], "sum log w", m._sum_log_w, D["sums"][2],
          "log det", ests.mean(), "dense", dense_ld, "se", se)
    assert abs(m.psi - D["psi"]) <= 1e-8 * abs(D["psi"])
    assert abs(m._sum_log_w - D["sums"][2]) <= 1e-8 * abs(D["sums"][2])
    assert np.max(np.abs(ests - ref_ests)) <= 1e-5 * abs(dense_ld)
    assert abs(ests.mean() - dense_ld) <= 4 * se
    assert abs(ll - lr.laplace_lml(m.psi, ests.mean(), m._sum_log_w)) <= 1e-12 * abs(ll)


@pytest.mark.parametrize("ms,frac,amp,lik", [((7, 5, 3), 0.2, 1.0, "poisson"),
                                             ((12, 10, 8), 0.0, 2.0, "binomial")])
def test_posterior_and_response_moments(gg, ms, frac, amp, lik):
    C = lr.case(ms, frac, amp, lik)
    D = lr.mode(ms, frac, amp, lik, solve="dense")
    m = fitted(gg, ms, frac, amp, lik)
    S = 256
    cov = lr.dense_cov(C["F"], C["mask"], D["noise"])
    sd = np.sqrt(np.diag(cov))
    mean, var = m.posterior_moments(S)
    z = np.max(np.abs(mean[:, 0] - D["f"]) / (sd / np.sqrt(S)))
    rmean, rvar = m.response_moments(S)
    lm, lv = lr.response_law(C["kind"], D["f"], np.diag(cov))
    zr = np.max(np.abs(rmean[:, 0] - lm) / np.sqrt(lv / S))
    print(lik, ms, "latent mean worst z %.2f, response mean worst z %.2f" % (z, zr))
    assert z <= 6
    assert zr <= 6
    assert rmean.shape == (C["y"].size, 1) and np.all(rvar >= 0)


def test_model_plumbing(gg):
    ms, frac, amp = (7, 5, 3), 0.2, 1.0
    C = lr.case(ms, frac, amp, "poisson")
    B = lr.case(ms, frac, amp, "binomial")
    mask = C["mask"]
    io = int(np.nonzero(mask)[0][0])     # an observed point

    def with_(case, **repl):
        c = dict(case)
        c.update(repl)
        return c

    with pytest.raises(ValueError):
        laplace_model(gg, ms, amp, "gaussian", C)
    with pytest.raises(ValueError):
        laplace_model(gg, ms, amp, "poisson", C, trials=np.ones(105))
    with pytest.raises(ValueError):
        laplace_model(gg, ms, amp, "binomial", B, exposure=np.ones(105))
    for bad in (0.0, -1.0, np.inf, np.nan):
        aux = C["aux"].copy()
        aux[io] = bad
        with pytest.raises(ValueError):
            laplace_model(gg, ms, amp, "poisson", with_(C, aux=aux))
    for bad in (-1.0, np.inf, np.nan):
        y = C["y"].copy()
        y[io] = bad
        with pytest.raises(ValueError):
            laplace_model(gg, ms, amp, "poisson", with_(C, y=y))
    y = B["y"].copy()
    y[io] = B["aux"][io] + 1
    with pytest.raises(ValueError):
        laplace_model(gg, ms, amp, "binomial", with_(B, y=y))
    with pytest.raises(ValueError):
        laplace_model(gg, ms, amp, "poisson", C, grad_method="adjoint")
    assert not mask[0]
    # NaN at the missing points is allowed everywhere; fractional y too
    y = np.where(mask, C["y"], np.nan)
    y[io] += 0.5
    aux = np.where(mask, C["aux"], np.nan)
    m = laplace_model(gg, ms, amp, "poisson", with_(C, y=y, aux=aux), dev_y=True)
    m.fit()
    assert m.newton_converged
    mean, none = m.predict_grid(compute_var=False)
    assert hasattr(mean, "is_cuda") and mean.is_cuda and none is None
    assert bool(np.all(np.isfinite(host(mean))))
    rm, rv = m.response_moments(4)
    assert rm.is_cuda and rv.is_cuda and tuple(rm.shape) == (105, 1)
    assert np.array_equal(m.constraints[:1], ["fixed"])
    # optimize() through BaseModel does not lower the LML
    ll0 = float(np.squeeze(m.log_likelihood()))
    m.optimize(max_iters=2)
    ll1 = float(np.squeeze(m.log_likelihood()))
    print("LML before / after two L-BFGS iterations", ll0, ll1)
    assert ll1 >= ll0
    # off-grid prediction: the latent variance, below the prior's
    mu, v = m.predict(np.array([[0.5, 0.5, 0.5]]))
    assert mu.shape == (1, 1) and 0.0 < float(v[0, 0]) <= float(m.kern.diag_val)
