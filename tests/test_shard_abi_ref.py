"""Pins tests/shard_abi_ref.py (the long-double reference of the sharded
section of the C ABI) against the oracle and the library's host helpers, and
checks on the host that the float64 restatement dist_helpers.NumpyEngine meets
every bound tests/test_gpu_shard_abi.py asserts on the device: the bounds are
neither vacuous nor too tight.  The case lists' gates (fold mask, lean_ok) are
asserted here too.  No GPU."""
import numpy as np
import pytest
import torch

import kron_abi_ref as R
import oracle
import shard_abi_ref as S
from dist_helpers import NumpyEngine
from gp_grief_amd import distributed as D

LD = np.longdouble
CASES = S.matvec_cases()


def t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2.0 ** -60


def case_problem(m, G, mask):
    fs = S.case_factors(m, mask)
    x = R.vector(int(np.prod(m)), 5)
    return fs, x, [S.scatter(x, m, G, g) for g in range(G)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matvec_ref_and_numpy_engine(case):
    """The reference's K x, gathered with distributed.gather_global, is the
    oracle's to long-double accuracy (nonsymmetric factors: a transposed
    factor or a swapped axis shows); NumpyEngine's float64 phases lie inside
    the matvec bound, each on the reference's own input."""
    _, m, G, env, mask = case
    fs, x, loc = case_problem(m, G, mask)
    for F in fs:
        assert F.shape[0] == 1 or not np.array_equal(F, F.T)
    for g in range(G):     # the layout is distributed.scatter_global's
        assert np.array_equal(loc[g], D.scatter_global(x, m, G, g))
    assert np.array_equal(S.gather(loc, m), x)
    y = S.matvec_ref(fs, G, loc, mask)
    want = oracle.kron_matvec(fs, x)
    got = D.gather_global([np.asarray(v, dtype=np.float64) for v in y], m)
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    full, _ = R.matvec_ref(fs, x)
    assert float(np.max(np.abs(S.gather(y, m) - full))) <= 1e-17 * len(m) * max(m) * float(
        np.max(np.abs(full))) + 1e-300
    # float64 phases inside the bound
    worst = 0.0
    sends = []
    for g in range(G):
        e = NumpyEngine(fs, G, g)
        send = e.empty()
        e.phase1(t64(loc[g]), send)
        ref, mag = S.phase1_ref(fs, G, loc[g], mask)
        worst = max(worst, R.worst_ratio(send.numpy(), ref, S.phase1_bound(fs, loc[g], mag)))
        sends.append(send.numpy().copy())
    recvs = S.exchange(sends)
    for g in range(G):
        e = NumpyEngine(fs, G, g)
        send = e.empty()
        e.phase2(t64(recvs[g]), send)
        ref, mag = S.phase2_ref(fs, G, recvs[g], mask)
        worst = max(worst, R.worst_ratio(send.numpy(), ref, S.phase2_bound(fs, recvs[g], mag)))
    assert 0.0 <= worst <= 1.0, worst


def test_case_gates():
    """Every folded case passes the restated fold gate with exactly the mask
    it was written for, every dense case has mask 0 with folding off, and the
    fused case list has both values of lean_ok at k = 1, k = 2 and the last
    position."""
    for name, m, G, env, mask in CASES:
        fs = S.case_factors(m, mask)
        if env == ("GG_KRON_FOLD", "0"):
            assert mask == 0 and S.fold_mask(fs, enabled=False) == 0
        else:
            fmin = int(env[1]) if env else 48
            assert S.fold_mask(fs, fmin) == mask != 0, name
        assert m[0] % G == 0 and m[1] % G == 0
    seen = {(pos, v): False for pos in ("k1", "k2", "last") for v in (True, False)}
    for m, G in S.FUSED_SHAPES:
        flags = S.lean_flags(m, G)
        assert flags == S.FUSED_LEAN[m], (m, flags)
        fs = R.toeplitz_factors(m)
        assert S.fold_mask(fs, 8) & ~1 == ((1 << len(m)) - 1) & ~1      # factors 1..d-1 fold
        assert len(m) >= 4 and (int(np.prod(m)) // G) % 2 == 0
        seen[("k1", flags[0])] = seen[("k2", flags[1])] = seen[("last", flags[-1])] = True
    assert all(seen.values()), seen
    assert S.lean_ok(12, 10) and not S.lean_ok(8, 10) and not S.lean_ok(12, 1 << 27)


def test_dot_chain_counts():
    assert S.vec_blocks(0) == S.vec_blocks(3) == 1
    n = 2 * 256 * 2048 + 3
    assert S.vec_blocks(n) == 2048
    # past the wrap: thread 0 takes two 16-byte lanes and the tail
    assert S.dot_chain(n, 2) == 5 + 6 + 4 + 2 + 6 + 16
    assert S.dot_chain(n, 1) == 3 + 6 + 4 + 2 + 6 + 16
    assert S.dot_chain(3, 2) == 3 + 6 + 4 + 1 + 6 + 16
    x, y = R.vector(n, 1), R.vector(n, 2)
    ref, mag = S.dot_ref(x, y)
    assert abs(LD(float(np.dot(x, y))) - ref) <= n * S.U53 * mag   # pairwise float64: far inside


def textbook_problem(m, G):
    fs = R.toeplitz_factors(m)
    b = R.vector(int(np.prod(m)), 9)
    return fs, b, [S.scatter(b, m, G, g) for g in range(G)]


@pytest.mark.parametrize("m,G", S.TEXTBOOK_SHAPES)
def test_textbook_steps_numpy_engine(m, G):
    """Four textbook iterations in lockstep: every NumpyEngine float64 step
    lies inside the scalar bounds of the reference step applied to the
    engine's own state, and the iterates approach the oracle's CG."""
    fs, b, loc = textbook_problem(m, G)
    shift = 0.05
    es = [NumpyEngine(fs, G, g) for g in range(G)]
    nl = es[0].n_local
    r = [t64(v) for v in loc]
    x = [e.zeros() for e in es]
    p = [e.zeros() for e in es]
    q = [e.empty() for e in es]

    def allreduce():
        s = sum(float(e.red[0]) for e in es)
        for e in es:
            e.red[0] = s
        return s

    for g, e in enumerate(es):
        e.local_dot(r[g], r[g])
    rr = allreduce()
    sc = S.init_ref(None, rr, 1e-10, 0.0)
    for e in es:
        e.cg_init(1e-10, 0.0)
        assert e.cg_status()[1] == sc["done"] and e.cg_status()[3] == sc["tol"]
    worst = 0.0
    for it in range(4):
        sends = []
        for g, e in enumerate(es):
            pref, pmag = S.prologue_ref(sc, p[g].numpy(), r[g].numpy())
            send = e.empty()
            e.phase1(p[g], send, r=r[g])
            worst = max(worst, R.worst_ratio(p[g].numpy(), pref, S.AXPY_C * S.U53 * pmag))
            sends.append(send.numpy().copy())
        recvs = S.exchange(sends)
        sends = []
        for g, e in enumerate(es):
            send = e.empty()
            e.phase2(t64(recvs[g]), send)
            sends.append(send.numpy().copy())
        for g, v in enumerate(S.exchange(sends)):
            q[g].numpy()[:] = v
        for g, e in enumerate(es):
            qref, qmag = S.shift_dot_ref(sc, q[g].numpy(), p[g].numpy(), shift)
            e.shift_dot(q[g], p[g], shift)
            worst = max(worst, R.worst_ratio(q[g].numpy(), qref, 2 * S.U53 * qmag))
            ref, mag = S.dot_ref(p[g].numpy(), q[g].numpy())
            assert abs(LD(float(e.red[0])) - ref) <= nl * S.U53 * mag
        pq = allreduce()
        sc = S.alpha_ref(sc, pq)
        for g, e in enumerate(es):
            e.cg_alpha()
            assert abs(LD(e.sc["alpha"]) - sc["alpha"]) <= 2 * S.U53 * abs(sc["alpha"])
            xr, rref, mx, mr = S.update_ref(sc, x[g].numpy(), r[g].numpy(), p[g].numpy(),
                                            q[g].numpy())
            e.cg_update(x[g], r[g], p[g], q[g])
            worst = max(worst, R.worst_ratio(x[g].numpy(), xr, S.AXPY_C * S.U53 * mx),
                        R.worst_ratio(r[g].numpy(), rref, S.AXPY_C * S.U53 * mr))
        rr = allreduce()
        sc = S.rho_ref(sc, rr)
        for e in es:
            e.cg_rho()
            assert e.cg_status()[:2] == (sc["iters"], sc["done"]) and e.cg_status()[2] == sc["rho"]
            assert abs(LD(e.sc["beta"]) - sc["beta"]) <= 2 * S.U53 * abs(sc["beta"])
    assert 0.0 < worst <= 1.0, worst
    xs, _, _ = oracle.cg_solve(lambda v: oracle.kron_matvec(fs, v) + shift * v, b, rtol=1e-30,
                               maxiter=4)
    got = S.gather([v.numpy() for v in x], m)
    assert np.linalg.norm(got - xs) <= 1e-12 * np.linalg.norm(xs)


def test_latch_cases_reference():
    """init's latch: r.r zero, NaN, negative, atol above |b|; rho's mid-run."""
    assert S.init_ref(None, 0.0, 1e-5, 0.0)["done"]
    assert S.init_ref(None, float("nan"), 1e-5, 0.0)["done"]
    assert S.init_ref(None, -1.0, 1e-5, 0.0)["done"]
    assert S.init_ref(None, 4.0, 0.0, 2.5)["done"]
    sc = S.init_ref(None, 4.0, 0.1, 0.0)
    assert not sc["done"] and sc["tol"] == 0.2 and sc["first"]
    sc = S.rho_ref(S.alpha_ref(sc, 8.0), 0.01)
    assert sc["done"] and sc["iters"] == 1 and sc["alpha"] == LD(0.5)
    frozen = S.rho_ref(S.alpha_ref(sc, 1.0), 100.0)
    assert frozen == sc
    e = NumpyEngine(R.toeplitz_factors((2, 2)), 1, 0)
    for rr, rtol, atol in ((0.0, 1e-5, 0.0), (-1.0, 1e-5, 0.0), (4.0, 0.0, 2.5), (4.0, 0.1, 0.0)):
        e.red[0] = rr
        with np.errstate(invalid="ignore"):
            e.cg_init(rtol, atol)
        assert bool(e.cg_status()[1]) == S.init_ref(None, rr, rtol, atol)["done"]


@pytest.mark.parametrize("m,G", S.FUSED_SHAPES)
def test_fused_steps_numpy_engine(m, G):
    """Six fused iterations with a close and a re-entry after the third, the
    reference's scalars against NumpyEngine's float64 ones step by step, and
    the closed state against the textbook recurrence of the same iterations."""
    fs, b, loc = textbook_problem(m, G)
    shift = 0.05
    es = [NumpyEngine(fs, G, g) for g in range(G)]
    nl = es[0].n_local
    r = [t64(v) for v in loc]
    x = [e.zeros() for e in es]
    q = [e.zeros() for e in es]
    pb = [[e.zeros() for _ in range(4)] for e in es]
    ids = [[0, 1, 2, 3] for _ in es]
    for g, e in enumerate(es):
        e.local_dot(r[g], r[g])
    rr = sum(float(e.red[0]) for e in es)
    for e in es:
        e.red[0] = rr
        e.cg_init(1e-12, 0.0)
    sc = S.init_ref(None, rr, 1e-12, 0.0)
    worst = 0.0
    for it in range(6):
        sends = []
        for g, e in enumerate(es):
            vecs = {ids[g][j]: pb[g][j].numpy().copy() for j in range(4)}
            ref = S.fused_prologue_ref(sc, pb[g][0].numpy(), r[g].numpy(), q[g].numpy(),
                                       x[g].numpy(), shift, vecs)
            send = e.empty()
            e.phase1_fused(pb[g][0], pb[g][1], send, r[g], q[g], x[g], shift, False)
            worst = max(worst,
                        R.worst_ratio(r[g].numpy(), ref["r"], ref["b_r"]),
                        R.worst_ratio(pb[g][1].numpy(), ref["p_new"], ref["b_p"]),
                        R.worst_ratio(x[g].numpy(), ref["x"], ref["b_x"]))
            sends.append(send.numpy().copy())
        recvs = S.exchange(sends)
        sends = []
        for g, e in enumerate(es):
            send = e.empty()
            e.phase2(t64(recvs[g]), send)
            sends.append(send.numpy().copy())
        for g, v in enumerate(S.exchange(sends)):
            q[g].numpy()[:] = v
        red = np.zeros(5)
        for g, e in enumerate(es):
            e.fused_post(q[g], pb[g][1], shift)
            pq, qq, mpq, mqq, _ = S.fused_post_ref(q[g].numpy(), pb[g][1].numpy(), shift)
            got = e.red5.numpy()
            assert abs(LD(got[2]) - pq) <= (nl + 2) * S.U53 * mpq
            assert abs(LD(got[4]) - qq) <= (nl + 4) * S.U53 * mqq and got[3] == 0.0
            red += got
        for g, e in enumerate(es):
            e.red5[:] = t64(red)
            e.fused_scalars(pb[g][1])
        sc = S.fused_scalars_ref(sc, red, ids[0][1])
        for g, e in enumerate(es):
            assert abs(LD(e.sc["alpha"]) - sc["alpha"]) <= 2 * S.U53 * abs(sc["alpha"])
            assert abs(LD(e.sc["beta"]) - sc["beta"]) <= sc["beta_err"]
            assert (e.sc["xh"], bool(e.sc["xs"]), bool(e.sc["pending"])) == \
                (sc["xh"], sc["xs"], sc["pending"])
            pb[g][0], pb[g][1], pb[g][2], pb[g][3] = pb[g][1], pb[g][3], pb[g][0], pb[g][2]
            ids[g][0], ids[g][1], ids[g][2], ids[g][3] = ids[g][1], ids[g][3], ids[g][0], ids[g][2]
        if it in (2, 5):
            rr = 0.0
            for g, e in enumerate(es):
                vecs = {ids[g][j]: pb[g][j].numpy().copy() for j in range(4)}
                _, xr, rref, bx, br = S.fused_close_ref(sc, x[g].numpy(), r[g].numpy(),
                                                        q[g].numpy(), pb[g][0].numpy(), shift,
                                                        vecs)
                e.fused_close(x[g], r[g], q[g], pb[g][0], shift)
                worst = max(worst,
                            R.worst_ratio(x[g].numpy(), xr, bx),
                            R.worst_ratio(r[g].numpy(), rref, br))
                rr += float(e.red[0])
            sc = S.fused_close_ref(sc, x[0].numpy(), r[0].numpy(), q[0].numpy(),
                                   pb[0][0].numpy(), shift,
                                   {ids[0][j]: pb[0][j].numpy() for j in range(4)})[0]
            for e in es:
                e.red[0] = rr
                e.fused_close_rho()
            sc = S.fused_close_rho_ref(sc, rr)
            for e in es:
                assert e.cg_status()[:2] == (sc["iters"], sc["done"])
                assert e.cg_status()[2] == sc["rho"] and not e.sc["pending"]
            assert sc["iters"] == it + 1
            xs, _, _ = oracle.cg_solve(lambda v: oracle.kron_matvec(fs, v) + shift * v, b,
                                       rtol=1e-30, maxiter=it + 1)
            got = S.gather([v.numpy() for v in x], m)
            assert np.linalg.norm(got - xs) <= 1e-11 * np.linalg.norm(xs)
    assert 0.0 < worst <= 1.0, worst


# ----------------------------------------------------------------- folds
PARITY_CASES = [((5, 7, 3), 1), ((2, 4), 4), ((2, 6, 3), 2), ((4, 5), 2), ((4, 2, 6, 3), 8),
                ((2,) * 12, 8)]


@pytest.mark.parametrize("m,G", PARITY_CASES)
def test_parity_fold_ref(m, G):
    """parity_fold_ref / parity_unfold_ref agree with distributed.parity_fold
    / parity_unfold inside the fold bound; the ranks' contributions sum to x;
    the per-rank fold matrices, stacked, are orthogonal (small cases)."""
    n = int(np.prod(m))
    x = R.vector(n, 21)
    host = D.parity_fold(x, m, G)
    total = np.zeros(n, dtype=LD)
    locs = []
    for g in range(G):
        ref, bound = S.parity_fold_ref(x, m, G, g)
        assert ref.size == n // G
        assert R.worst_ratio(host[g], ref, bound) <= 1.0
        con, cb = S.parity_unfold_ref(ref, m, G, g)
        assert not np.any(np.isnan(con))          # every element written
        total += con
        locs.append(np.asarray(ref, dtype=np.float64))
    assert float(np.max(np.abs(total - x))) <= 4 * G * S.U53 * float(np.max(np.abs(x)))
    back = D.parity_unfold(locs, m)
    assert np.max(np.abs(back - x)) <= 8 * G * S.U53 * np.max(np.abs(x))
    if n <= 64:
        P = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1.0
            P[:, j] = np.concatenate([np.asarray(S.parity_fold_ref(e, m, G, g)[0], np.float64)
                                      for g in range(G)])
        assert np.max(np.abs(P.dot(P.T) - np.eye(n))) <= 1e-15


def test_shard0_ref():
    for m, G in (((6, 5, 3), 3), ((4, 7), 4), ((5, 3), 1)):
        n = int(np.prod(m))
        x = R.vector(n, 22)
        for g in range(G):
            pos = S.shard0_positions(m, G, g)
            assert np.array_equal(pos, D.local_index_map(m, G, g))
            assert np.array_equal(S.shard0_ref(x, m, G, g), x[pos])
