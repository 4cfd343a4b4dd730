"""Posterior sampling of GPGridModel on one MI355X (linalg.GridPosteriorSampler).

Eigenbasis route (complete grid, solver='exact'; default 4-D RBF 72^4): ms per
draw -- gg_kron_posterior_coeffs plus one Kronecker matvec with Q -- beside, in
the same run and alternated with it, the coefficient pass alone, one
K.matvec_device, one Q.matvec_device and a plain read-plus-write stream of N
doubles (a device copy).  The draw is expected to cost about one matvec plus
one such stream; the line reports the ratio actually measured, and the
coefficient pass's bytes per second beside the copy's, which says whether the
Box-Muller transcendentals leave it stream-bound.
Matheron route (--mask-m^4 grid with --mask missing, default 32^4 and 10 %):
ms per draw, one masked CG solve each, with the iteration counts.

Host clock around work that ends in a device synchronise; every timed shape is
warmed first; best and median of --rounds rounds of --reps calls.  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=72)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--mask-m", type=int, default=32)
    ap.add_argument("--mask", type=float, default=0.1, metavar="FRAC")
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mask-draws", type=int, default=4)
    args = ap.parse_args()
    import torch
    import gp_grief_amd as gg
    import gp_grief_amd.kern  # noqa: F401
    import gp_grief_amd.models  # noqa: F401
    from gp_grief_amd import native
    t = torch
    d, s = args.d, args.noise

    def data(m):
        """y = sum_i sin(6 x_i) + noise on the m^d grid, generated on the device."""
        N = m ** d
        gen = t.Generator(device="cuda").manual_seed(0)
        idx = t.arange(N, device="cuda")
        y = 0.1 * t.randn(N, generator=gen, device="cuda", dtype=t.float64)
        for i in range(d):
            y += t.sin(6.0 * ((idx // m ** i) % m).to(t.float64) / (m - 1))
        return y.reshape(-1, 1), gen

    def model(m, y, **kw):
        xg = [np.linspace(0, 1, m).reshape(-1, 1)] * d
        kl = [gg.kern.RBF(1, variance=1.0, lengthscale=0.2 * (1 + 0.05 * i)) for i in range(d)]
        return gg.models.GPGridModel(xg, y, gg.kern.GridKernel(kl), noise_var=s, **kw)

    def timed(fn, reps):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(reps):
            fn(r)
        t.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    # ---- eigenbasis route
    m = args.m
    N = m ** d
    y, _ = data(m)
    mod = model(m, y, solver='exact')
    smp = mod._sampler(0)
    assert smp.route == 'eigen'
    K, Q = mod._operator(), smp.Q
    a, b = smp.y, t.empty_like(smp.y)
    L, sp = native.lib(), native.stream_ptr

    def coeffs(r):
        native.check(L.gg_kron_posterior_coeffs(
            smp._d, smp._ms, native.dptr(smp._lam), s, native.dptr(smp._yt), 0, 2 * r,
            native.dptr(smp._c), sp()), "gg_kron_posterior_coeffs")

    jobs = {"draw_ms": lambda r: smp._terms(r),
            "coeffs_ms": coeffs,
            "k_matvec_ms": lambda r: K.matvec_device(a, out=b),
            "q_matvec_ms": lambda r: Q.matvec_device(a, out=b),
            "copy_stream_ms": lambda r: b.copy_(a)}
    for fn in jobs.values():
        timed(fn, 3)                                   # warm-up: every shape
    runs = {k: [] for k in jobs}
    for rnd in range(args.rounds):
        for k, fn in jobs.items():
            runs[k].append(timed(fn, args.reps))
    eig = {k: min(v) for k, v in runs.items()}
    eig.update({k.replace("_ms", "_median_ms"): float(np.median(v)) for k, v in runs.items()})
    gb = 16.0 * N / 1e9                                # one read and one write of N doubles
    eig["coeffs_GBps"] = gb / (eig["coeffs_ms"] * 1e-3)
    eig["copy_stream_GBps"] = gb / (eig["copy_stream_ms"] * 1e-3)
    eig["draw_over_k_matvec_plus_stream"] = eig["draw_ms"] / (eig["k_matvec_ms"]
                                                              + eig["copy_stream_ms"])
    eig["draw_over_q_matvec_plus_stream"] = eig["draw_ms"] / (eig["q_matvec_ms"]
                                                              + eig["copy_stream_ms"])
    eig["coeffs_over_stream"] = eig["coeffs_ms"] / eig["copy_stream_ms"]
    del mod, smp, K, Q, a, b, y
    t.cuda.empty_cache()

    # ---- Matheron route on an incomplete grid
    mm = args.mask_m
    ym, gen = data(mm)
    mask = t.rand(mm ** d, generator=gen, device="cuda") >= args.mask
    modm = model(mm, ym, mask=mask, logdet='lanczos')
    smpm = modm._sampler(0)
    smpm._terms(0)                                     # warm-up
    del smpm.cg_iters[:]
    per = [timed(lambda r, k=k: smpm._terms(k), 1) for k in range(1, 1 + args.mask_draws)]
    masked = {"draw_ms": min(per), "draw_median_ms": float(np.median(per)),
              "cg_iters": list(smpm.cg_iters), "N": mm ** d,
              "missing": int(mm ** d - modm.num_observed), "cg_rtol": modm.cg_rtol}

    out = {"metric": "GPGridModel posterior draw, eigenbasis route", "unit": "ms per draw",
           "higher_is_better": False, "n_gpus": 1, "dtype": "f64", "data": "synthetic",
           "value": eig["draw_ms"],
           "config": {"workload": "%d-D %d^%d RBF grid, noise %g" % (d, m, d, s), "N": N,
                      "masked_workload": "%d-D %d^%d RBF grid, %g missing" % (d, mm, d, args.mask),
                      "reps": args.reps, "rounds": args.rounds,
                      "device": torch.cuda.get_device_name(0)},
           "eigenbasis": eig, "masked": masked}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
