"""bench.py on one MI355X at a small grid: a plain run prints the headline
line and nothing that takes a run of its own, --full adds the legs beside it,
and --dump-outputs writes the solve the timed path computed.

The dumped x is checked against the oracle's textbook CG on the same inputs
(bench.grid_factors, bench.rhs_at) after the same W + K iterations.  Bound
1e-8 relative: the two recurrences differ by rounding (1.1e-16 per operation),
which a CG iterate amplifies by at most the condition number of K + s I --
below 12^3 / 0.01 = 1.7e5 for three 12 x 12 unit-variance RBF factors -- per
iteration, over 5 iterations, with a factor 100 in hand.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

M, D, STEPS, WARMUP = 12, 3, 3, 2
LEGS = ("matvec", "block_matvec", "lanczos", "grief", "cpu_baseline", "box",
        "prologue_calibration", "prologue_calibration_gbs")


def _run_bench(out_dir, *extra):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--grid", str(M), "--dims", str(D), "--steps", str(STEPS),
                          "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)] + list(extra),
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def oracle_solve(gpu):
    """x and ||r|| after W + K textbook CG iterations on bench.py's inputs."""
    import torch
    import bench
    import oracle
    _, F = bench.grid_factors(M, D)
    b = bench.rhs_at(torch.arange(M ** D, dtype=torch.int64), M, D, torch).numpy()
    s = 0.01
    mv = lambda v: oracle.kron_matvec(F, v) + s * v
    x, _, it = oracle.cg_solve(mv, b, rtol=0.0, maxiter=WARMUP + STEPS)
    assert it == WARMUP + STEPS
    x.setflags(write=False)
    return x, float(np.linalg.norm(b - mv(x)))


def _check_dump(out_dir, oracle_solve):
    xs, rs = oracle_solve
    files = sorted(os.listdir(out_dir))
    assert files == ["resid.npy", "x.npy", "x_index.npy"]
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    x = np.load(os.path.join(out_dir, "x.npy"))
    idx = np.load(os.path.join(out_dir, "x_index.npy"))
    resid = np.load(os.path.join(out_dir, "resid.npy"))
    assert x.dtype == np.float64 and x.shape == (M ** D,)
    assert (idx == np.arange(M ** D)).all()
    err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
    print("x rel err %.3e, resid %.6e (oracle's b - A x: %.6e)" % (err, float(resid[0]), rs))
    assert err < 1e-8
    # the recurrence's own ||r|| (gg_cg_status): a norm, of the size of the true residual
    assert resid.dtype == np.float64 and resid.shape == (1,)
    assert 0.5 * rs < float(resid[0]) < 2.0 * rs


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(oracle_solve, tmp_path):
    rec = _run_bench(tmp_path)
    assert rec["steps"] == STEPS and rec["warmup"] == WARMUP and rec["n_gpus"] == 1
    assert rec["unit"] == "CG iters/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f64" and rec["metric"].startswith("CG iters/sec")
    assert rec["value"] > 0
    assert abs(rec["ms_per_step"] * rec["value"] - 1e3) < 1e-6 * 1e3
    for k in LEGS:
        assert k not in rec, k
    _check_dump(tmp_path, oracle_solve)


@pytest.mark.gpu
def test_full_run_adds_the_legs(oracle_solve, tmp_path):
    rec = _run_bench(tmp_path, "--full", "--matvec", "2", "--lanczos", "3", "--grief", "off",
                     "--cpu-baseline", "off")
    assert rec["steps"] == STEPS and rec["value"] > 0
    for k in ("matvec", "lanczos", "box", "prologue_calibration"):
        assert k in rec, k
    assert rec["matvec"]["reps"] == 2 and rec["lanczos"]["steps"] == 3
    assert "grief" not in rec and "cpu_baseline" not in rec
    _check_dump(tmp_path, oracle_solve)
