"""Pins tests/grief_abi_ref.py (the long-double reference of the GRIEF basis C
ABI) against the code that already exists, and checks on the host that NumPy's
own float64 evaluation meets every bound tests/test_gpu_grief_abi.py asserts
on the device, for every parametrised case of that module: the bounds are
neither vacuous nor too tight.  No GPU."""
import types

import numpy as np
import pytest

import grief_abi_ref as R
import oracle
import test_gpu_compat
import test_gpu_grief_abi as G

LD = np.longdouble


def close(a, b, tol=1e-13):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return bool(np.all(np.abs(a - b) <= tol * np.abs(b)))


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2.0 ** -60


@pytest.mark.parametrize("kind", R.KINDS)
def test_cov_ref_vs_oracle(kind):
    rng = np.random.default_rng(0)
    x, z = rng.random(41), rng.random(29)
    x[:5] = z[:5]
    # (the delta rule is the RBF's; elsewhere l = 1e-7 only underflows)
    for ls in (0.05, 0.3, 2.0) + ((1e-7,) if kind == "RBF" else ()):
        k, t = R.cov_ref(kind, 1.3, ls, x.reshape(-1, 1), z.reshape(-1, 1))
        assert k.dtype == LD and k.shape == t.shape == (41, 29)
        assert close(k, oracle.cov_1d(kind, x, z, 1.3, ls)), ls
        assert close(R.cov_ref(R.KINDS.index(kind), 1.3, ls, x, z)[0], k, 0)
    d2 = (x[:, None] - z[None, :]) ** 2
    want = {"RBF": d2 / (2 * 0.3 ** 2), "Exponential": np.sqrt(d2) / 0.3,
            "Matern32": np.sqrt(3 * d2) / 0.3, "Matern52": np.sqrt(5 * d2) / 0.3}[kind]
    assert close(R.cov_ref(kind, 1.3, 0.3, x, z)[1], want)


def test_phi_of_tables_vs_oracle():
    """phi_ref(tables_ref(...)) is oracle.grief_phi on oracle.grief_inducing's
    selection (d = 3, m = 16, p = 30, n = 200)."""
    d, m, p, n = 3, 16, 30, 200
    rng = np.random.default_rng(2)
    specs = [("RBF", 1.0, 0.2), ("Matern52", 1.2, 0.3), ("Exponential", 0.8, 0.25)]
    xg = [np.linspace(0, 1, m) for _ in range(d)]
    x = rng.random((n, d))
    ind = oracle.grief_inducing(specs, xg, p)
    cols, cidx, col0 = [], np.zeros((p, d), dtype=np.int32), 0
    for f in range(d):
        i = d - 1 - f                                   # factor f <-> input dim d - 1 - f
        uniq, inv = np.unique(ind["eig_pos"][:, f], return_inverse=True)
        kind, var, ls = specs[i]
        X, A = R.tables_ref(kind, var, ls, x[:, i], xg[i], ind["Q"][f].T[uniq, :])
        assert X.shape == A.shape == (uniq.size, n) and np.all(A >= np.abs(X))
        cols.append(X.T)
        cidx[:, f] = col0 + inv.reshape(-1)
        col0 += uniq.size
    Phi = R.phi_ref(np.concatenate(cols, axis=1), cidx, ind["log_lam"])
    assert Phi.dtype == LD and Phi.shape == (n, p)
    assert rel(Phi, oracle.grief_phi(x, specs, xg, ind)) < 1e-13


@pytest.mark.parametrize("logged", [True, False])
def test_expand_skc_ref_vs_restatement(logged):
    rng = np.random.default_rng(1)
    n, p, ms = 100, 40, [7, 9, 5]
    S, K, Cs, rows, cidx, row0 = [], [], [], [], np.zeros((p, 3), dtype=np.int32), 0
    for f, m in enumerate(ms):
        uniq, inv = np.unique(rng.integers(0, m, p), return_inverse=True)
        S.append(types.SimpleNamespace(unique=uniq, unique_inverse=inv.reshape(-1)))
        K.append(rng.standard_normal((m, m)))
        c = rng.standard_normal((m, n))
        c[:, 3] = 0.0
        Cs.append(c)
        rows.append(K[-1][uniq, :].dot(c))
        cidx[:, f] = row0 + inv.reshape(-1)
        row0 += uniq.size
    X = np.concatenate(rows, axis=0)
    want = test_gpu_compat.expand_skc_ref(S, K, Cs, logged)
    got = R.expand_skc_ref(X, cidx, logged)
    if logged:
        assert rel(got[0], want[0]) < 1e-13
        assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
        assert np.all(got[1][:, 3] == 0) and np.all(got[0][:, 3] == 0)
        assert np.all(got[2] >= np.abs(got[0]))
    else:
        assert rel(got, want) < 1e-13


# ------------------------------ NumPy float64 against the device tests' bounds
def test_numpy_meets_cov_bounds():
    cases = [(k, D, ls, nx, nz) for k in G.KINDS for D in G.COV_DS for ls in G.COV_LS
             for nx, nz in G.COV_SHAPES] + [G.COV_WRAP]
    for kind, D, ls, nx, nz in cases:
        x, z, out0, k, t = R.cov_problem(kind, D, ls, nx, nz, G.COV_VAR)
        f = R.cov_f64(kind, G.COV_VAR, ls, x, z)
        G.check("numpy cov", f, k, R.cov_bound(D, k, t), str((kind, D, ls, nx, nz)))
        if (nx, nz) == G.COV_SHAPES[1]:
            for mode, g in ((1, out0 * f), (2, out0 + f)):
                ref, bound = G.cov_mode_bound(mode, D, out0, k, t)
                G.check("numpy cov mode %d" % mode, g, ref, bound)
    for D in G.COV_DS:
        x, z = G.cov_delta_problem(D)
        k, t = R.cov_ref(0, G.COV_VAR, 1e-7, x, z)
        assert np.all(t == 0) and set(np.unique(k)) == {0, LD(G.COV_VAR)}
    print("numpy / bound, cov: %.3f" % G.WORST["numpy cov"])
    assert 0.01 < G.WORST["numpy cov"] <= 1.0


def test_numpy_meets_tables_bounds():
    for m, u in G.TAB_SHAPES:
        for n in G.TAB_NS:
            for kind in G.KINDS:
                for ls in G.TAB_LS:
                    x, xg, q, X, A = R.tables_problem(kind, ls, m, u, n, G.TAB_VAR)
                    G.check("numpy tables", R.tables_f64(kind, G.TAB_VAR, ls, x, xg, q), X,
                            R.tables_bound(m, A), str((m, u, n, kind, ls)))
                    if n in (1, 17, 83):
                        zr = u - 1 if u >= 2 else None
                        x, xg, q, X, A = R.tables_problem(kind, ls, m, u, n, G.TAB_VAR, zr)
                        L, S = R.log_tables(R.tables_f64(kind, G.TAB_VAR, ls, x, xg, q))
                        G.check_log_sign("numpy tables log/sign", L, S, X, R.tables_bound(m, A), q,
                                         str((m, u, n, kind, ls)))
    for name in sorted(G.ALL_CASES):
        c = G.ALL_CASES[name]
        for n in (1, 17, 83):
            x, xgs, qs, col0s, Ut = G.all_problem(name, n)
            assert Ut == sum(c["us"]) + 5 and col0s[0] > 0
            for f in range(len(qs)):
                a = (c["kinds"][f], G.TAB_VAR, c["ls"][f], x[:, f], xgs[f], qs[f])
                X, A = R.tables_ref(*a)
                G.check("numpy tables", R.tables_f64(*a), X, R.tables_bound(c["ms"][f], A), name)
    print("numpy / bound, tables: %.3f, log/sign %.3f"
          % (G.WORST["numpy tables"], G.WORST["numpy tables log/sign"]))
    assert 0.001 < G.WORST["numpy tables"] <= 1.0


def test_numpy_meets_phi_bounds():
    cases = [(d, Ut, p, n) for d, Ut, p in G.PHI_CASES for n in G.PHI_NS]
    cases += [(1, G.phi_u_cap(1, tr), 4, 65) for tr in (0, 1)]
    for d, Ut, p, n in cases:
        T, cidx, log_lam = R.phi_problem(d, Ut, p, n)
        assert np.isnan(T).any() or np.unique(cidx).size == Ut
        L, S = R.log_tables(T)
        assert np.array_equal(np.isnan(T), np.isnan(L)) and np.all(L[T == 0] == 0)
        for form, Tf, Tv in (("value", T, T), ("log", S * np.exp(L), R.log_tables_value(L, S))):
            ref = R.phi_ref(Tv, cidx, log_lam)
            G.check("numpy phi " + form, R.phi_f64(Tf, cidx, log_lam), ref, R.phi_bound(d, ref),
                    str((d, Ut, p, n)))
    print("numpy / bound, phi: value %.3f log %.3f"
          % (G.WORST["numpy phi value"], G.WORST["numpy phi log"]))
    assert 0.01 < G.WORST["numpy phi value"] <= 1.0 and G.WORST["numpy phi log"] <= 1.0


def test_numpy_meets_expand_skc_bounds():
    for d, p, n in G.SKC_CASES:
        X, cidx = R.expand_problem(d, p, n)
        ref = R.expand_skc_ref(X, cidx, False)
        G.check("numpy skc", R.expand_skc_f64(X, cidx, False), ref, R.expand_bound(d, ref=ref))
        ref, sref, B = R.expand_skc_ref(X, cidx, True)
        got, sg = R.expand_skc_f64(X, cidx, True)
        assert np.array_equal(sg, sref) and np.all(sref[:, n // 2] == 0)
        G.check("numpy skc logged", got, ref, R.expand_bound(d, B=B))
    print("numpy / bound, expand_skc: %.3f logged %.3f"
          % (G.WORST["numpy skc"], G.WORST["numpy skc logged"]))
    assert 0.01 < G.WORST["numpy skc"] <= 1.0


def test_dispatch_model_matches_branch_shapes():
    """The thresholds parsed from gg_grief.hip put the branch shapes where the
    device tests' docstring says."""
    assert (G.M_MFMA, G.M_QUAD) == (480, 512)
    assert [G.tables_route(1, 0.3, m, False) for m, _ in G.TAB_SHAPES] == G.TAB_ROUTES
    assert G.phi_u_cap(1, 0) == 318 and G.phi_u_cap(1, 1) == 372
