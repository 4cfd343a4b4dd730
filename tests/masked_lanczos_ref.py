"""NumPy restatement of the masked Lanczos / SLQ log det (test infrastructure
only).

Lanczos on A = W K W + s I, W = diag(mask), from the Rademacher probe zeroed
at the missing points.  Every Lanczos vector is zero off the observed set, so
the tridiagonal is that of K_oo + s I from the compressed probe, and the
quadrature scaled by the observed count estimates log det(K_oo + s I).  The
device runs the same recurrence (gg_lanczos_probe_masked,
linalg.slq_logdet(mask=...)); dense_masked_lanczos is the compressed dense
route both are compared against.
"""
import numpy as np

import oracle
import masked_ref as mr

# the shapes and missing fractions shared by the CPU and GPU tests: odd N = 105
# (unaligned tails), d = 2, 3, 4, unequal factor orders, 10 - 60 % missing
CASES = [((7, 5, 3), 0.2), ((16, 12), 0.3), ((12, 10, 8), 0.3), ((12, 10, 8), 0.1),
         ((16, 16, 8), 0.6), ((8, 6, 5, 4), 0.3)]


def masked_lanczos(F, mask, shift, seed, probe, steps):
    """(alphas, betas) of Lanczos on v -> where(mask, K v, 0) + shift v from
    where(mask, probe_signs(seed, probe, N), 0)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    z = np.where(mask, oracle.cg.probe_signs(seed, probe, mask.size), 0.0)

    def A(v):
        return np.where(mask, oracle.kron_matvec(F, v), 0.0) + shift * v
    return oracle.lanczos_tridiag(A, z, steps)


def dense_masked_lanczos(F, mask, shift, seed, probe, steps, Koo=None):
    """The same on the dense compressed matrix K_oo + shift I from the
    compressed probe."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    o = np.nonzero(mask)[0]
    if Koo is None:
        Koo = mr.dense_K(F)[np.ix_(o, o)]
    z = oracle.cg.probe_signs(seed, probe, mask.size)[o]
    return oracle.lanczos_tridiag(lambda v: Koo.dot(v) + shift * v, z, steps)


def masked_slq(F, mask, shift, probes=8, steps=30, seed=0):
    """(mean, per-probe estimates) of log det(K_oo + shift I): n_obs times each
    masked probe's quadrature, steps capped at n_obs."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    n_obs = int(mask.sum())
    steps = min(int(steps), n_obs)
    ests = []
    for j in range(probes):
        a, b = masked_lanczos(F, mask, shift, seed, j, steps)
        ests.append(oracle.cg.quadrature_logdet(a, b, float(n_obs)))
    return float(np.mean(ests)), np.array(ests)


_cache = {}


def case(ms, frac, shift):
    """dict(F, mask, ld, slq=(mean, ests)) for one of CASES at seed=3,
    probes=16, steps=40: computed once per session, shared and read-only."""
    key = (tuple(ms), frac, shift)
    if key not in _cache:
        F = mr.rbf_factors(ms)
        mask = mr.make_mask(int(np.prod(ms)), frac)
        ld = mr.dense_logdet(F, mask, shift)
        mean, ests = masked_slq(F, mask, shift, probes=16, steps=40, seed=3)
        for a in F + [mask, ests]:
            a.setflags(write=False)
        _cache[key] = dict(F=F, mask=mask, ld=ld, slq=(mean, ests))
    return _cache[key]
