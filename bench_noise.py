"""Per-point noise on an incomplete grid on one MI355X: the weighted masked CG
(gg_cgm_set_noise) and the weighted masked Lanczos step
(gg_lanczos_probe_masked_noise) beside their scalar-noise twins.

Workloads: 4-D RBF grids 32^4 (N = 1.0e6) and 72^4 (N = 2.7e7), noise_var =
0.01, noise_scale log-uniform over two decades, 10 % of the points missing.
Per shape, in the same run:
  weighted CG    one iteration of MaskedKronCG(noise=): the matvec with shift 0,
                 the direction pass (3 passes + the noise), the update pass (6
                 passes + the noise), the mask twice;
  scalar CG      one iteration of MaskedKronCG(K, s, mask): the code path this
                 feature leaves untouched;
  weighted / scalar Lanczos step: (T(2 S) - T(S)) / S of two whole probes of S
                 and 2 S steps (HIP events around the calls; the start pass and
                 the closing copy cancel), the same way for both.
The pass count predicts two more reads on 2 d + 9 passes per CG iteration
(2 / 17 at d = 4) and one more read per Lanczos step; at 32^4 the iteration
is launch-bound.

Prints one JSON line and, with --out, writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[32, 72])
    ap.add_argument("--dims", type=int, default=4)
    ap.add_argument("--missing", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lanczos", type=int, default=20, metavar="STEPS")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    import gp_grief_amd as gg
    import oracle

    d, s = a.dims, 0.01
    shapes = []
    for m in a.grids:
        N = m ** d
        g = np.linspace(0.0, 1.0, m)
        F = [oracle.cov_1d("RBF", g, g, 1.0, 0.1 * (1 + 0.05 * i)) + 1e-12 * np.eye(m)
             for i in range(d)]
        K = gg.tensors.KronMatrix(F, sym=True)
        rng = np.random.default_rng(0)
        mask = np.ones(N, dtype=bool)
        mask[rng.choice(N, size=int(round(a.missing * N)), replace=False)] = False
        mask[0] = mask[-1] = False
        md = torch.from_numpy(mask).cuda().to(torch.uint8)
        noise = torch.from_numpy(
            s * np.exp(np.random.default_rng(3).uniform(np.log(0.1), np.log(10.0), N))).cuda()
        y = torch.randn(N, dtype=torch.float64, device="cuda",
                        generator=torch.Generator(device="cuda").manual_seed(1))

        def timed_cg(solver):
            # rtol = 0: the stopping test never fires, every iteration runs
            solver.start(y, rtol=0.0)
            solver.iterate(a.warmup)
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            solver.iterate(a.iters)
            ev1.record()
            torch.cuda.synchronize()
            assert solver.status()[0] == a.warmup + a.iters
            return ev0.elapsed_time(ev1) / a.iters

        work = gg.device.empty(4 * N)

        def timed_lz(shift=0.0, **kw):
            def probe(steps):
                ev0 = torch.cuda.Event(enable_timing=True)
                ev1 = torch.cuda.Event(enable_timing=True)
                ev0.record()
                gg.linalg.lanczos_tridiag(K, shift, steps, probe=1, mask=md, work=work, **kw)
                ev1.record()
                torch.cuda.synchronize()
                return ev0.elapsed_time(ev1)
            probe(min(a.warmup, a.lanczos))
            t1 = probe(a.lanczos)
            t2 = probe(2 * a.lanczos)
            return (t2 - t1) / a.lanczos

        ms_w = timed_cg(gg.linalg.MaskedKronCG(K, None, md, noise=noise))
        ms_s = timed_cg(gg.linalg.MaskedKronCG(K, s, md))
        lz_w = timed_lz(noise=noise)
        lz_s = timed_lz(shift=s)
        shapes.append({
            "grid": m, "n": N, "observed": int(mask.sum()),
            "weighted_cg_ms_per_iter": ms_w, "scalar_cg_ms_per_iter": ms_s,
            "weighted_over_scalar_cg": ms_w / ms_s,
            "weighted_lanczos_ms_per_step": lz_w, "scalar_lanczos_ms_per_step": lz_s,
            "weighted_over_scalar_lanczos": lz_w / lz_s,
        })
        del K, work, noise, y, md
        torch.cuda.empty_cache()
    out = {
        "metric": "weighted masked CG iteration on a %d-D %d^%d RBF grid, %.0f %% missing"
                  % (d, a.grids[-1], d, 100 * a.missing),
        "value": shapes[-1]["weighted_cg_ms_per_iter"], "unit": "ms/iteration",
        "higher_is_better": False, "n_gpus": 1, "iters": a.iters, "warmup": a.warmup,
        "dtype": "f64", "data": "synthetic",
        "config": {"dims": d, "noise_var": s, "noise_scale": "log-uniform [0.1, 10]",
                   "missing": a.missing, "lanczos_steps": a.lanczos},
        "predicted_cg_ratio_from_passes": (2.0 * d + 11.0) / (2.0 * d + 9.0),
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
