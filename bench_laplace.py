"""Laplace approximation with a Poisson likelihood on an incomplete grid on one
MI355X: the fused Newton pass (gg_lik_newton), the response moments
(gg_lik_response_accumulate) and a whole GPGridLaplaceModel.fit().

Workloads: 4-D RBF grids 32^4 (N = 1.0e6) and 72^4 (N = 2.7e7), counts y ~
Poisson(e exp f) of a smooth f of amplitude 1, exposure log-uniform on [0.5, 4],
10 % of the points missing.  Per shape, in the same run:
  pass, write form      reads y, aux, f, a (8 N bytes each) and the mask (N),
                        writes noise and b: 48 N + N bytes (40 N + N without aux);
  pass, read-only form  the four reads and the mask: 32 N + N bytes;
  copy                  a device copy of N doubles (8 N read + 8 N written): the
                        stream rate the byte counts are turned into times with;
  response accumulate   draw k >= 2: reads f, w, mean, m2, writes mean, m2 (48 N);
  fit()                 Newton steps, CG iterations per step, wall time and the
                        share of it spent outside the CG solves.
The ratios measured / predicted say how far each pass is from a pure stream.

Prints one JSON line and, with --out, writes it to a file.
"""
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
    ap.add_argument("--grids", type=int, nargs="+", default=[32, 72])
    ap.add_argument("--fit-grids", type=int, nargs="*", default=None,
                    help="grids to run fit() on (default: all of --grids)")
    ap.add_argument("--dims", type=int, default=4)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cg-rtol", type=float, default=1e-8)
    ap.add_argument("--newton-tol", type=float, default=1e-6)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    import gp_grief_amd as gg
    from gp_grief_amd import native

    d = a.dims
    fit_grids = a.grids if a.fit_grids is None else a.fit_grids
    L = native.lib()
    shapes = []

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        for _ in range(a.iters):
            fn()
        ev1.record()
        torch.cuda.synchronize()
        return ev0.elapsed_time(ev1) / a.iters

    for m in a.grids:
        N = m ** d
        g = np.linspace(0.0, 1.0, m)
        gen = torch.Generator(device="cuda").manual_seed(5)
        # a smooth latent field of amplitude 1: the mean of d separable waves
        f_true = torch.zeros([m] * d, dtype=torch.float64, device="cuda")
        for i in range(d):
            shape = [1] * d
            shape[i] = m
            f_true += torch.from_numpy(np.sin(2 * np.pi * (g + 0.1 * i))).cuda().reshape(shape)
        f_true = (f_true / d).reshape(-1)
        expo = torch.exp(torch.empty(N, dtype=torch.float64, device="cuda").uniform_(
            float(np.log(0.5)), float(np.log(4.0)), generator=gen))
        y = torch.poisson(expo * torch.exp(f_true), generator=gen)
        mask = torch.rand(N, device="cuda", generator=gen) >= a.missing
        mask[0] = mask[-1] = False
        md = mask.to(torch.uint8)
        fd = f_true.clone()
        ad = torch.randn(N, dtype=torch.float64, device="cuda", generator=gen)
        noise, b = gg.device.empty(N), gg.device.empty(N)
        sums = torch.zeros(5, dtype=torch.float64, device="cuda")
        part = gg.device.empty(native.GG_LIK_PARTIALS)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731

        def lik(aux, write):
            native.check(L.gg_lik_newton(native.GG_LIK_POISSON, p(y), p(aux), p(fd), p(ad), p(md),
                                         p(noise) if write else None, p(b) if write else None,
                                         p(sums), p(part), N, native.stream_ptr()))

        t_write = timed(lambda: lik(expo, True))
        t_write_noaux = timed(lambda: lik(None, True))
        t_read = timed(lambda: lik(expo, False))
        src, dst = gg.device.empty(N).normal_(generator=gen), gg.device.empty(N)
        t_copy = timed(lambda: dst.copy_(src))
        gbps = 16.0 * N / t_copy * 1e-6            # bytes / ms -> GB/s
        mean, m2 = gg.device.zeros(N), gg.device.zeros(N)
        t_resp = timed(lambda: native.check(L.gg_lik_response_accumulate(
            native.GG_LIK_POISSON, p(fd), p(src), p(mean), p(m2), 2, N, native.stream_ptr())))

        def predicted(nbytes):
            return nbytes / (gbps * 1e6)           # ms at the copy's rate

        row = {
            "grid": m, "n": N, "observed": int(mask.sum().item()),
            "copy_ms": t_copy, "copy_gb_per_s": gbps,
            "pass_write_ms": t_write, "pass_write_over_bytes": t_write / predicted(49.0 * N),
            "pass_write_noaux_ms": t_write_noaux,
            "pass_write_noaux_over_bytes": t_write_noaux / predicted(41.0 * N),
            "pass_readonly_ms": t_read, "pass_readonly_over_bytes": t_read / predicted(33.0 * N),
            "response_accumulate_ms": t_resp,
            "response_accumulate_over_bytes": t_resp / predicted(48.0 * N),
        }
        del src, dst, mean, m2, noise, b, fd, ad
        torch.cuda.empty_cache()
        if m in fit_grids:
            kerns = [gg.kern.RBF(1, variance=1.0, lengthscale=0.1 * (1 + 0.05 * (d - 1 - j)))
                     for j in range(d)]
            xg = [g.reshape(-1, 1) for _ in range(d)]
            model = gg.models.GPGridLaplaceModel(
                xg, y.reshape(-1, 1), gg.kern.GridKernel(kerns), "poisson", exposure=expo,
                mask=md, cg_rtol=a.cg_rtol, newton_tol=a.newton_tol)
            cg_s = [0.0]
            solve = gg.linalg.MaskedKronCG.solve

            def timed_solve(self, *args, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = solve(self, *args, **kw)      # ends in status(): synchronised
                cg_s[0] += time.perf_counter() - t0
                return out

            gg.linalg.MaskedKronCG.solve = timed_solve
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.fit()
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
            finally:
                gg.linalg.MaskedKronCG.solve = solve
            row.update({
                "fit_ms": 1e3 * total, "fit_cg_ms": 1e3 * cg_s[0],
                "fit_share_outside_cg": 1.0 - cg_s[0] / total,
                "newton_steps": model.newton_iters, "newton_converged": model.newton_converged,
                "newton_stalled": model.newton_stalled, "cg_iters": list(model.cg_iters),
                "halvings": list(model._newton.halvings),
            })
            del model
        shapes.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del y, expo, md, mask, f_true
        torch.cuda.empty_cache()
    out = {
        "metric": "gg_lik_newton (Poisson, write form) on a %d-D %d^%d grid, %.0f %% missing"
                  % (d, a.grids[-1], d, 100 * a.missing),
        "value": shapes[-1]["pass_write_ms"], "unit": "ms/pass",
        "higher_is_better": False, "n_gpus": 1, "iters": a.iters, "warmup": a.warmup,
        "dtype": "f64", "data": "synthetic",
        "config": {"dims": d, "likelihood": "poisson", "exposure": "log-uniform [0.5, 4]",
                   "missing": a.missing, "cg_rtol": a.cg_rtol, "newton_tol": a.newton_tol},
        "bytes_per_point": {"write": 49, "write_noaux": 41, "readonly": 33, "response": 48},
        "shapes": shapes,
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
