"""Masked CG on an incomplete grid (the grid GP with missing observations) on
one MI355X.

Workload: 3-D RBF grid 128^3 (N = 2.1e6), sigma^2 = 0.01, 25 % of the points
missing.  One "step" = one iteration of linalg.MaskedKronCG (gg_cgm_*): the
Kronecker matvec in the grid basis, the direction kernel (3 passes over N) and
the masked x / r update (6 passes + the mask).  Alongside, the same number of
iterations of cg(recurrence="textbook", basis="grid") on the same operator and
right-hand side: the unmasked CG the masked one is derived from, whose
direction update rides on the first mode product.  Pass counts predict
near-parity; the preconditioned iteration (precond='kron', two more Kronecker
matvecs) is reported too.

--lanczos STEPS (default 0: off) adds the masked Lanczos step of the SLQ log
det (gg_lanczos_probe_masked_timed): the same matvec and one masked update
pass (3 reads + 1 write + the mask, 4.125 passes beside the matvec against the
CG iteration's 9.125), timed per step by HIP events after a short warm-up
probe, and its ratio to the masked CG iteration of the same run.

Prints one JSON line: ms per iteration of each and the masked / textbook ratio.
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
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--dims", type=int, default=3)
    ap.add_argument("--missing", type=float, default=0.25)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lanczos", type=int, default=0, metavar="STEPS",
                    help="also time STEPS masked Lanczos steps (0: off)")
    a = ap.parse_args()
    import torch
    import gp_grief_amd as gg
    import oracle

    m, d, s = a.grid, a.dims, 0.01
    N = m ** d
    g = np.linspace(0.0, 1.0, m)
    F = [oracle.cov_1d("RBF", g, g, 1.0, 0.1 * (1 + 0.05 * i)) + 1e-12 * np.eye(m)
         for i in range(d)]
    K = gg.tensors.KronMatrix(F, sym=True)
    rng = np.random.default_rng(0)
    mask = np.ones(N, dtype=bool)
    mask[rng.choice(N, size=int(round(a.missing * N)), replace=False)] = False
    mask[0] = mask[-1] = False
    y = torch.randn(N, dtype=torch.float64, device="cuda",
                    generator=torch.Generator(device="cuda").manual_seed(1))

    def timed(solver):
        # rtol = 0: the stopping test never fires, every iteration runs
        solver.start(y, rtol=0.0)
        solver.iterate(a.warmup)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        solver.iterate(a.iters)
        ev1.record()
        torch.cuda.synchronize()
        it = solver.status()[0]
        assert it == a.warmup + a.iters, it
        return ev0.elapsed_time(ev1) / a.iters

    ms_masked = timed(gg.linalg.MaskedKronCG(K, s, mask))
    ms_pcg = timed(gg.linalg.MaskedKronCG(K, s, mask, precond='kron'))
    ms_text = timed(gg.linalg.KronCG(K, s, recurrence="textbook", basis="grid"))
    out = {
        "metric": "masked CG iteration on a %d-D %d^%d RBF grid, %.0f %% missing"
                  % (d, m, d, 100 * a.missing),
        "value": ms_masked, "unit": "ms/iteration", "higher_is_better": False,
        "n_gpus": 1, "iters": a.iters, "warmup": a.warmup, "dtype": "f64", "data": "synthetic",
        "config": {"grid": m, "dims": d, "sigma2": s, "missing": a.missing,
                   "observed": int(mask.sum())},
        "masked_ms_per_iter": ms_masked,
        "textbook_grid_ms_per_iter": ms_text,
        "masked_over_textbook": ms_masked / ms_text,
        "masked_kron_precond_ms_per_iter": ms_pcg,
        "streamed_passes_beside_matvec": 9.125,
    }
    if a.lanczos > 0:
        work = gg.device.empty(4 * N)
        md = torch.from_numpy(mask).cuda().to(torch.uint8)
        gg.linalg.lanczos_tridiag(K, s, min(a.warmup, a.lanczos), mask=md, work=work)
        _, _, step_ms = gg.linalg.lanczos_tridiag(K, s, a.lanczos, probe=1, mask=md, work=work,
                                                  timed=True)
        assert gg.linalg.lanczos_tridiag.n_observed == int(mask.sum())
        ms_lz = float(np.mean(step_ms))
        out["config"]["lanczos_steps"] = a.lanczos
        out["masked_lanczos_ms_per_step"] = ms_lz
        out["masked_lanczos_over_masked_cg"] = ms_lz / ms_masked
        out["lanczos_streamed_passes_beside_matvec"] = 4.125
    print(json.dumps(out))


if __name__ == "__main__":
    main()
