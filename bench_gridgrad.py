"""LML gradient of GPGridModel on one MI355X: forward differences (the
default grad_method, d + 3 log-likelihoods for a d-dimensional RBF grid:
noise, kernel 0's variance, d lengthscales and the base point) against
grad_method='adjoint' (one log-likelihood, d + 1 Kronecker matvecs for the
data-fit terms and one streamed trace pass; with --mask FRAC the traces are
Hutchinson estimates, one masked CG solve per probe).  Times one
log_likelihood(return_gradient=True) of a fresh model per method (best of
--reps), and the trace pass gg_kron_trace_ratio at P = d + 2 and P = 1 beside
gg_kron_logdet_shifted on the same grid (host clock around the synchronising
calls, alternated, best of 20).  Prints one JSON line."""
import argparse
import ctypes
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
    ap.add_argument("--mask", type=float, default=None, metavar="FRAC",
                    help="fraction of missing grid points (masked model, logdet='lanczos')")
    ap.add_argument("--noise", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    import gp_grief_amd as gg
    import gp_grief_amd.kern  # noqa: F401
    import gp_grief_amd.models  # noqa: F401
    from gp_grief_amd import native
    d, m, s = args.d, args.m, args.noise
    N = m ** d
    xg = [np.linspace(0, 1, m).reshape(-1, 1)] * d
    # y = sum_i sin(6 x_i) + noise, dimension 0 fastest, generated on the device
    t = torch
    gen = t.Generator(device="cuda").manual_seed(0)
    idx = t.arange(N, device="cuda")
    y = 0.1 * t.randn(N, generator=gen, device="cuda", dtype=t.float64)
    for i in range(d):
        y += t.sin(6.0 * ((idx // m ** i) % m).to(t.float64) / (m - 1))
    y = y.reshape(-1, 1)
    kw = {}
    if args.mask is not None:
        mask = t.rand(N, generator=gen, device="cuda") >= args.mask
        kw = dict(mask=mask, logdet='lanczos')

    def model(method):
        kl = [gg.kern.RBF(1, variance=1.0, lengthscale=0.2 * (1 + 0.05 * i)) for i in range(d)]
        return gg.models.GPGridModel(xg, y, gg.kern.GridKernel(kl), noise_var=s,
                                     grad_method=method, **kw)

    out = {"metric": "GPGridModel log_likelihood(return_gradient=True)",
           "unit": "ms per gradient", "higher_is_better": False, "n_gpus": 1, "dtype": "f64",
           "data": "synthetic",
           "config": {"workload": "%d-D %d^%d RBF grid, noise %g" % (d, m, d, s), "N": N,
                      "mask_fraction": args.mask, "lmls_per_fd_gradient": d + 3,
                      "device": torch.cuda.get_device_name(0)}}
    grads = {}
    for method in ("finite_difference", "adjoint"):
        model(method).log_likelihood(return_gradient=True)        # warm-up: every shape
        times = []
        for rep in range(args.reps):
            mod = model(method)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ll, g = mod.log_likelihood(return_gradient=True)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        out[method + "_ms"] = min(times)
        out[method + "_lml"] = float(np.squeeze(ll))
        grads[method] = g
    free = np.array([True, True, True] + [False, True] * (d - 1))
    # free entries (noise, variance 0, lengthscales): the two methods' gradients
    # differ by the forward differences' truncation (step 1e-6) and, with
    # --mask, by the estimators they differentiate
    for method in grads:
        out[method + "_grad"] = [float(v) for v in grads[method][free]]
    out["value"] = out["adjoint_ms"]
    out["speedup_vs_finite_difference"] = out["finite_difference_ms"] / out["adjoint_ms"]

    # the trace pass beside the log-det pass it is modelled on
    mod = model("adjoint")
    mod.parameters
    dd, ms, lamd = mod._lam_dev()
    rowlen = int(lamd.numel())
    L, sp = native.lib(), native.stream_ptr
    num = torch.ones((d + 2) * rowlen, dtype=torch.float64, device="cuda")
    num[rowlen:] = lamd.repeat(d + 1)
    res = (ctypes.c_double * (d + 2))()
    ld = ctypes.c_double()

    def t_trace(P):
        t0 = time.perf_counter()
        native.check(L.gg_kron_trace_ratio(dd, ms, native.dptr(lamd), s, P, native.dptr(num), res,
                                           sp()), "gg_kron_trace_ratio")
        return (time.perf_counter() - t0) * 1e3

    def t_logdet():
        t0 = time.perf_counter()
        native.check(L.gg_kron_logdet_shifted(dd, ms, native.dptr(lamd), s, ctypes.byref(ld),
                                              sp()), "gg_kron_logdet_shifted")
        return (time.perf_counter() - t0) * 1e3

    best = {"trace_ratio_ms": np.inf, "trace_ratio_p1_ms": np.inf, "logdet_shifted_ms": np.inf}
    for rep in range(22):
        cur = {"trace_ratio_ms": t_trace(d + 2), "trace_ratio_p1_ms": t_trace(1),
               "logdet_shifted_ms": t_logdet()}
        if rep >= 2:
            best = {k: min(best[k], cur[k]) for k in best}
    out["passes"] = dict(best, P=d + 2, points=N)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
