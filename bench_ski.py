"""Structured kernel interpolation on one MI355X: the passes of one CG iteration
on n = 10^6 scattered points (linalg.GridInterp, linalg.SKICG, GPSKIModel).

Shapes (RBF, points uniform in the interpolation domain): 1024^2 cubic, 128^3
cubic, 40^4 linear.  Per shape, in the same run, 50 calls after 10 warm-up:
  copy      a device copy of 2^26 doubles (1 GiB moved, past the last-level
            cache): the run's own HBM streaming rate
  interp    t = W g            spread   g = W^T p
  matvec    K.matvec_device    cg_iter  one iteration of SKICG
  spread_skew  spread with all points drawn into 1 % of the cells (long rows of
            the inverted index: the split path)
  fit       a whole GPSKIModel.fit() and its iteration count
Each pass is also given as a ratio to its byte count at the copy's rate
(x_bytes: 1 = the pass moves its bytes as fast as the copy does).  The byte
model: interp  n (d (4 + 8 order) + order^(d-1) max(32, 8 order) + 8),
       spread  12 nnz + 8 (N + 1) + 8 N (+ the gather of p, not counted),
       matvec  (2 d + 1) 8 N.

Prints one JSON line and, with --out, writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

COPY_ELEMS = 1 << 26
SHAPES = [((1024, 1024), "cubic", 0.02), ((128, 128, 128), "cubic", 0.1),
          ((40, 40, 40, 40), "linear", 0.3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--noise", type=float, default=0.1)
    ap.add_argument("--fit-rtol", type=float, default=1e-6)
    ap.add_argument("--shapes", type=int, nargs="+", default=[0, 1, 2],
                    help="indices into the shape list")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import torch
    import gp_grief_amd as gg

    n = a.points

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

    def points(xg, order, frac, seed):
        """n uniform points in the interpolation domain, or in a corner box
        that holds `frac` of its cells."""
        rng = np.random.default_rng(seed)
        pad = 1 if order == 4 else 0
        side = frac ** (1.0 / len(xg))
        X = np.empty((n, len(xg)))
        for f, g in enumerate(xg):
            lo, hi = g[pad, 0], g[len(g) - 1 - pad, 0]
            X[:, f] = rng.uniform(lo, lo + side * (hi - lo), n)
        return X

    shapes = []
    for idx in a.shapes:
        ms, kind, ls = SHAPES[idx]
        d, order = len(ms), 4 if kind == "cubic" else 2
        N = int(np.prod(ms))
        xg = [np.linspace(0.0, 1.0, m).reshape(-1, 1) for m in ms]
        kern = gg.kern.GridKernel([gg.kern.RBF(1, lengthscale=ls) for _ in range(d)])
        K = kern.cov_grid(xg, dim_noise_var=1e-12)
        X = points(xg, order, 1.0, 0)
        t0 = time.perf_counter()
        W = gg.linalg.GridInterp(xg, X, order=kind)
        torch.cuda.synchronize()
        setup_s = time.perf_counter() - t0
        gen = torch.Generator(device="cuda").manual_seed(1)
        g = torch.randn(N, dtype=torch.float64, device="cuda", generator=gen)
        p = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        tn, gN = gg.device.empty(n), gg.device.empty(N)
        # the baseline copy is sized past the last-level cache (2^26 doubles
        # each way: 1 GiB per call), so its rate is the HBM's
        c0, c1 = gg.device.zeros(COPY_ELEMS), gg.device.empty(COPY_ELEMS)
        copy_ms = timed(lambda: c1.copy_(c0))
        rate = 16.0 * COPY_ELEMS / (copy_ms * 1e-3)   # bytes / s
        del c0, c1
        interp_ms = timed(lambda: W.interp(g, out=tn))
        spread_ms = timed(lambda: W.spread(p, out=gN))
        matvec_ms = timed(lambda: K.matvec_device(g))
        solver = gg.linalg.SKICG(K, W, a.noise, max_steps=0)
        solver.start(p, rtol=0.0)   # rtol = 0: the stopping test never fires
        solver.iterate(a.warmup)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        solver.iterate(a.iters)
        ev1.record()
        torch.cuda.synchronize()
        assert solver.status()[0] == a.warmup + a.iters
        cg_ms = ev0.elapsed_time(ev1) / a.iters
        del solver
        b_interp = n * (d * (4 + 8 * order) + order ** (d - 1) * max(32, 8 * order) + 8)
        b_spread = 12 * W.nnz + 8 * (N + 1) + 8 * N
        b_matvec = (2 * d + 1) * 8 * N

        def ratio(ms_, nbytes):
            return ms_ * 1e-3 * rate / nbytes

        # the whole fit: a smooth function of the coordinates plus noise
        rng = np.random.default_rng(2)
        y = np.prod(np.sin(3.0 * X + 0.5), axis=1) + np.sqrt(a.noise) * rng.standard_normal(n)
        model = gg.models.GPSKIModel(torch.from_numpy(X).cuda(),
                                     torch.from_numpy(y.reshape(-1, 1)).cuda(), kern, xg,
                                     noise_var=a.noise, interp=kind, cg_rtol=a.fit_rtol)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.fit()
        torch.cuda.synchronize()
        fit_s = time.perf_counter() - t0
        fit_iters = model.cg_iters
        del model
        # the skew case: every point inside 1 % of the cells
        Ws = gg.linalg.GridInterp(xg, points(xg, order, 0.01, 3), order=kind)
        skew_ms = timed(lambda: Ws.spread(p, out=gN))
        shapes.append({
            "grid": list(ms), "interp": kind, "n": n, "N": N, "nnz": W.nnz,
            "setup_s": setup_s, "max_row": W.max_row, "long_rows": W.long_rows,
            "copy_ms": copy_ms, "copy_elems": COPY_ELEMS, "copy_GBps": rate / 1e9,
            "interp_ms": interp_ms, "interp_x_bytes": ratio(interp_ms, b_interp),
            "spread_ms": spread_ms, "spread_x_bytes": ratio(spread_ms, b_spread),
            "matvec_ms": matvec_ms, "matvec_x_bytes": ratio(matvec_ms, b_matvec),
            "cg_iter_ms": cg_ms,
            "cg_iter_share_of_W": (interp_ms + spread_ms) / cg_ms,
            "spread_skew_ms": skew_ms, "spread_skew_over_uniform": skew_ms / spread_ms,
            "skew_max_row": Ws.max_row, "skew_long_rows": Ws.long_rows,
            "skew_chunks": Ws.chunks,
            "fit_s": fit_s, "fit_iters": fit_iters, "fit_rtol": a.fit_rtol,
            "bytes": {"interp": b_interp, "spread": b_spread, "matvec": b_matvec},
        })
        del W, Ws, K, g, p, tn, gN
        torch.cuda.empty_cache()
    out = {
        "metric": "SKI CG iteration, n = %d points on a %s grid, %s interpolation"
                  % (n, "x".join(str(m) for m in shapes[-1]["grid"]), shapes[-1]["interp"]),
        "value": shapes[-1]["cg_iter_ms"], "unit": "ms/iteration",
        "higher_is_better": False, "n_gpus": 1, "iters": a.iters, "warmup": a.warmup,
        "dtype": "f64", "data": "synthetic",
        "config": {"noise_var": a.noise, "kernel": "RBF", "split": gg.linalg.GridInterp.SPLIT},
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
