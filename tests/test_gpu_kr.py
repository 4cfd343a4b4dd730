"""Off-grid P1: the device Khatri-Rao contraction (gg_kr_contract) and
GPGridModel.predict against the oracle (oracle.kr_contract,
oracle.grid_offgrid_predict) and the reference-generated fixture
grid_offgrid.npz (GridKernel.cov_kr KhatriRaoMatrix * alpha; dense variance)."""
import numpy as np
import pytest

import oracle
from conftest import golden

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def gg(gpu):
    import gp_grief_amd
    import gp_grief_amd.kern  # noqa: F401
    import gp_grief_amd.models  # noqa: F401
    return gp_grief_amd


@pytest.mark.parametrize("ms,M", [([13], 5), ([7, 9], 37), ([5, 6, 7], 300),
                                  ([4, 3, 5, 6], 1), ([3, 4, 2, 5, 3], 129),
                                  ([2, 3, 2, 2, 3, 2, 2, 3], 65),        # d = 8: fused, NF = 7
                                  ([2, 3, 2, 2, 3, 2, 2, 2, 3], 70),     # d = 9: two-pass path
                                  ([300, 1, 130], 200)])
def test_kr_contract_vs_oracle(gg, ms, M):
    rng = np.random.default_rng(len(ms) * 100 + M)
    blocks = [rng.standard_normal((M, m)) for m in ms]
    c = rng.standard_normal(int(np.prod(ms)))
    KR = gg.tensors.KhatriRaoMatrix(blocks, partition=0)
    assert KR.shape == (M, int(np.prod(ms)))
    y = KR * c.reshape(-1, 1)
    assert y.shape == (M, 1)
    assert rel(y, oracle.kr_contract(blocks, c)) < 1e-13


def test_kr_contract_chunked_equals_single(gg):
    """A scratch of the minimum size forces several GEMM chunks on the
    two-pass path (d > 8); results agree and repeated runs are bitwise
    identical (fixed-order reductions)."""
    import torch
    rng = np.random.default_rng(5)
    ms, M = [3, 3, 3, 3, 3, 3, 3, 3, 2], 70      # d = 9: the chunked two-pass path
    blocks = [rng.standard_normal((M, m)) for m in ms]
    c = rng.standard_normal(int(np.prod(ms)))
    KR = gg.tensors.KhatriRaoMatrix(blocks, partition=0)
    cd = torch.from_numpy(c).cuda()
    a = KR.contract(cd).cpu().numpy()
    b = KR.contract(cd, work_elems=1).cpu().numpy()
    b2 = KR.contract(cd, work_elems=1).cpu().numpy()
    assert np.array_equal(b, b2)
    assert rel(a, b) < 1e-14
    f1 = KR.contract(cd).cpu().numpy()
    assert np.array_equal(a, f1)


def test_kr_contract_fused_deterministic(gg):
    import torch
    rng = np.random.default_rng(6)
    ms, M = [37, 41, 29], 333
    blocks = [rng.standard_normal((M, m)) for m in ms]
    c = torch.from_numpy(rng.standard_normal(int(np.prod(ms)))).cuda()
    KR = gg.tensors.KhatriRaoMatrix(blocks, partition=0)
    a = KR.contract(c).cpu().numpy()
    assert np.array_equal(a, KR.contract(c).cpu().numpy())
    assert rel(a, oracle.kr_contract(blocks, c.cpu().numpy())) < 1e-13


def test_kr_wrong_shape_raises(gg):
    KR = gg.tensors.KhatriRaoMatrix([np.ones((3, 4)), np.ones((3, 5))], partition=0)
    with pytest.raises(ValueError):
        KR * np.ones((21, 1))
    with pytest.raises(NotImplementedError):
        gg.tensors.KhatriRaoMatrix([np.ones((3, 4))], partition=1)


def _grid_model(gg, z, tag, solver):
    ms, ls = z[tag + "_m"], z[tag + "_ls"]
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=float(l)) for l in ls]
    xg = [np.linspace(0.0, 1.0, int(m)).reshape(-1, 1) for m in ms]
    gk = gg.kern.GridKernel(kerns)
    return gg.models.GPGridModel(xg, z[tag + "_y"].reshape(-1, 1), gk,
                                 noise_var=float(z[tag + "_sigma2"]), solver=solver)


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("solver", ["exact", "cg"])
def test_grid_predict_offgrid_fixture(gg, tag, solver):
    z = golden("grid_offgrid.npz")
    m = _grid_model(gg, z, tag, solver)
    mean, var = m.predict(z[tag + "_xs"])
    assert mean.shape == var.shape == (len(z[tag + "_xs"]), 1)
    tol = 1e-11 if solver == "exact" else 1e-7
    assert rel(mean, z[tag + "_mean"]) < tol
    s = float(z[tag + "_sigma2"])
    assert rel(var - s, z[tag + "_var_latent"]) < 1e-9
    mean2, none = m.predict(z[tag + "_xs"], compute_var=False)
    assert none is None and rel(mean2, mean) < 1e-15


def test_grid_predict_on_grid_points_matches_predict_grid(gg):
    """At the grid nodes the off-grid path equals predict_grid (K alpha and the
    eigen-streamed variance)."""
    z = golden("grid_offgrid.npz")
    m = _grid_model(gg, z, "a", "exact")
    ms = [int(v) for v in z["a_m"]]
    xg = [np.linspace(0.0, 1.0, k) for k in ms]
    idx = np.random.default_rng(0).integers(0, int(np.prod(ms)), 40)
    # flat index -> per-dimension grid coordinates, input dim 0 fastest
    coords = np.stack([xg[i][(idx // int(np.prod(ms[:i]))) % ms[i]] for i in range(len(ms))], 1)
    mean, var = m.predict(coords)
    gm, gv = m.predict_grid()
    assert rel(mean[:, 0], gm[idx, 0]) < 1e-10
    assert rel(var[:, 0], gv[idx, 0]) < 1e-8


def test_grid_predict_offgrid_larger(gg):
    """48^4 grid (5.3M points), 64 test points: mean and variance vs the oracle."""
    rng = np.random.default_rng(9)
    m, d, s = 48, 4, 0.01
    ls = [0.15 * (1 + 0.05 * i) for i in range(d)]
    g = np.linspace(0.0, 1.0, m)
    kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=l) for l in ls]
    gk = gg.kern.GridKernel(kerns)
    y = rng.standard_normal((m ** d, 1))
    model = gg.models.GPGridModel([g.reshape(-1, 1)] * d, y, gk, noise_var=s)
    xs = rng.uniform(0, 1, (64, d))
    mean, var = model.predict(xs)
    factors = [oracle.cov_1d("RBF", g, g, 1.0, ls[d - 1 - f]) + 1e-12 * np.eye(m)
               for f in range(d)]
    blocks = [oracle.cov_1d("RBF", xs[:, d - 1 - f], g, 1.0, ls[d - 1 - f]) for f in range(d)]
    Q, t = oracle.factor_eigh(factors)
    lam = t[0]
    for ti in t[1:]:
        lam = np.multiply.outer(lam, ti).reshape(-1)
    alpha = oracle.solve_schur(Q, lam, y[:, 0], s)
    mo, vo = oracle.grid_offgrid_predict(factors, blocks, np.ones(64), alpha, s)
    assert rel(mean, mo) < 1e-9
    assert rel(var - s, vo) < 1e-8


# ---- gg_kr_contract through ctypes at the NT switch points, deep d and its
# scratch boundary.  Bound (elementwise, u = 2^-53): K = m_{d-1} products
# accumulated per outer row, the rows of a column summed in any order (outer =
# prod m_f, f < d - 1, of them), d - 1 weight multiplies:
#   |got - ref| <= (K + outer + d) u sum_g |c_g| prod_f |U_f[j][g_f]|
# against the contraction accumulated in long double.
def _kr_consts():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "gp_grief_amd", "csrc", "gg_kr.hip")).read()
    return {k: int(re.search(r"\b%s\s*=\s*(\d+)" % k, src).group(1))
            for k in ("kSMaxWG", "kKrMaxSplits", "kKrThreads", "kKrMaxD")}


def _kr_need(ms, M):
    """The scratch the path gg_kr_contract takes requires (its GG_REQUIREs)."""
    k = _kr_consts()
    outer = int(np.prod(ms[:-1])) if len(ms) > 1 else 1
    if len(ms) - 1 <= 7:                      # fused streaming kernel: gy partial rows
        nt = 1 if M <= 16 else (4 if M <= 64 else 8)
        groups = -(-(-(-outer // 16)) // 4)
        gx = -(-M // (16 * nt))
        return max(1, min(groups, max(1, k["kSMaxWG"] // gx))) * M
    bx = -(-M // k["kKrThreads"])             # two-pass: S partial rows + one row of T
    return (max(1, min(k["kKrMaxSplits"], -(-4096 // bx))) + 1) * M


def _kr_call(ms, M, work_elems=None, d=None, seed=0):
    """(status, out with its guards checked, blocks, c) of one gg_kr_contract
    call with exactly work_elems (default: what the path requires) of scratch."""
    import ctypes
    import torch
    from gp_grief_amd import native
    rng = np.random.default_rng(1000 * len(ms) + M + seed)
    blocks = [rng.standard_normal((M, m)) for m in ms]
    c = rng.standard_normal(int(np.prod(ms)))
    need = _kr_need(ms, max(M, 1)) if work_elems is None else work_elems
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    uts = [dev(b.T) for b in blocks[:-1]]
    ulast, cd = dev(blocks[-1]), dev(c)
    guard = np.full(64, np.nan)
    out = dev(np.concatenate([guard, np.full(M, np.nan), guard]))
    work = dev(np.full(max(need, 1) + 64, np.nan))
    ptrs = (ctypes.c_void_p * max(1, len(uts)))(*[native.dptr(u) for u in uts])
    st = native.lib().gg_kr_contract(
        len(ms) if d is None else d, native.i64_array(ms), native.dptr(cd), native.dptr(ulast),
        ptrs, M, ctypes.c_void_p(out.data_ptr() + 8 * 64), native.dptr(work), need,
        native.stream_ptr())
    o = out.cpu().numpy()
    assert np.all(np.isnan(o[:64])) and np.all(np.isnan(o[64 + M:])), "out guard written"
    assert np.all(np.isnan(work.cpu().numpy()[max(need, 1):])), "written past work_elems"
    return st, o[64:64 + M], blocks, c


def _kr_check(ms, M):
    from grief_abi_ref import kr_ref
    st, got, blocks, c = _kr_call(ms, M)
    assert st == 0
    ref, mag = kr_ref(blocks, c)
    outer = int(np.prod(ms[:-1])) if len(ms) > 1 else 1
    bound = (ms[-1] + outer + len(ms)) * 2.0 ** -53 * mag
    err = np.abs(got.astype(np.longdouble) - ref)
    print("gg_kr_contract ms %s M %d: worst err / bound %.4f" % (ms, M, float((err / bound).max())))
    assert not np.any(np.isnan(got)) and np.all(err <= bound), (ms, M, float((err / bound).max()))
    assert rel(ref, oracle.kr_contract(blocks, c)) < 1e-13
    return st


@pytest.mark.parametrize("M", [16, 17, 64, 65, 128])
def test_kr_contract_nt_switch_points(gg, M):
    """M = 16 | 17 and 64 | 65: the streaming kernel's NT = 1 | 4 | 8 tiles per
    pass; 128: one full pass of NT = 8."""
    _kr_check([5, 6, 7], M)


@pytest.mark.parametrize("K", [1, 15, 16, 17])
def test_kr_contract_single_factor(gg, K):
    """d = 1 (no weights, NF = 0) around the 16-deep staged k chunk."""
    _kr_check([K], 19)


@pytest.mark.parametrize("ms", [[2] * 11 + [3], [1] * 28 + [2, 2, 2, 3]],
                         ids=["d12", "d32"])
def test_kr_contract_deep(gg, ms):
    """The two-pass path (GEMM + odometer column sum) beyond d = 9."""
    _kr_check(ms, 19)


def test_kr_contract_limits(gg):
    """d = 33 and a scratch one element short of what the taken path needs are
    refused before any launch (out untouched); M = 0 is a no-op."""
    k = _kr_consts()
    st, out, _, _ = _kr_call([1] * k["kKrMaxD"] + [2], 3, d=k["kKrMaxD"] + 1)
    assert st == -1 and np.all(np.isnan(out))
    assert _kr_call([5, 6, 7], 0)[0] == 0
    for ms, M in [([5, 6, 7], 17), ([40, 41, 7], 65), ([2] * 11 + [3], 19)]:
        need = _kr_need(ms, M)
        st, out, _, _ = _kr_call(ms, M, work_elems=need - 1)
        assert st == -1 and np.all(np.isnan(out)), (ms, M)
        assert _kr_check(ms, M) == 0          # exactly `need` runs and meets the bound
