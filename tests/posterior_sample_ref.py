"""NumPy restatement of the grid posterior sampler (test infrastructure only).

The Gaussian stream of gg_normal_fill in uint64 arithmetic, the coefficient
formulas of gg_kron_posterior_coeffs / gg_kron_prior_coeffs /
gg_sample_residual, Welford's moments of gg_sample_accumulate, and both
sampling routes of linalg.GridPosteriorSampler written densely:

  eigenbasis (complete grid, exact solver): with K = Q diag(t) Q^T and
    yt = Q^T y, the posterior of the latent field is diagonal in the
    eigenbasis, N(t / (t + s) yt, t s / (t + s)); draw k is Q c with
    c = t / (t + s) yt + sqrt(max(t, 0) s / (t + s)) z, z = stream 2k.
  Matheron (mask, or the CG solver): f = Q (sqrt(max(t, 0)) z), z = stream 2k,
    is a prior draw; b = y - f - sqrt(s) e at the observed points, e = stream
    2k + 1; alpha = (K_oo + s I)^-1 b_o (0 at the missing points); draw k is
    f + K alpha.

Eigenvectors are defined up to sign, and the draw depends on the signs (c is
indexed by eigenvector), so a device draw is compared with the restatement fed
the device's own eigenpairs.
"""
import numpy as np

import masked_ref as mr
import oracle

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_NORMAL = 0xD1B54A32D192ED03
MAX_DRAWS = 32768          # draw k uses streams 2k and 2k + 1 of 65536


def normal_hashes(seed, stream, idx):
    """h(i) = splitmix64's finaliser of base + i * 0x9E3779B97F4A7C15 (mod 2^64)."""
    i = np.asarray(idx, dtype=np.uint64)
    base = np.uint64((((int(seed) & 0xffffffff) << 32) ^ ((int(stream) & 0xffff) << 16)
                      ^ _NORMAL) & 0xffffffffffffffff)
    with np.errstate(over="ignore"):
        z = base + i * _GOLD
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def normal_stream(seed, stream, n):
    """The first n standard normals of stream (seed, stream): Box-Muller on
    pairs of hashes; an odd n takes the cosine half of its last pair."""
    n = int(n)
    npair = (n + 1) // 2
    h = normal_hashes(seed, stream, np.arange(2 * npair, dtype=np.uint64))
    u1 = ((h[0::2] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = (h[1::2] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(2 * npair)
    z[0::2] = r * np.cos(2.0 * np.pi * u2)
    z[1::2] = r * np.sin(2.0 * np.pi * u2)
    return z[:n]


def posterior_coeffs(t, s, yt, z):
    return t / (t + s) * yt + np.sqrt(np.maximum(t, 0.0) * s / (t + s)) * z


def prior_coeffs(t, z):
    return np.sqrt(np.maximum(t, 0.0)) * z


def residual(y, f, mask, noise_sd, z):
    """y - f - noise_sd z at the observed points, exactly 0 elsewhere (a
    select: NaN in y at a missing point does not pass)."""
    if mask is None:
        return y - f - noise_sd * z
    with np.errstate(invalid="ignore"):
        return np.where(mask, y - f - noise_sd * z, 0.0)


def welford(draws):
    """(mean, m2) after folding the columns of draws in one at a time."""
    mean = np.array(draws[:, 0], dtype=np.float64)
    m2 = np.zeros_like(mean)
    for k in range(2, draws.shape[1] + 1):
        x = draws[:, k - 1]
        dlt = x - mean
        mean = mean + dlt / k
        m2 = m2 + dlt * (x - mean)
    return mean, m2


class DenseSampler(object):
    """Both routes densely for (factors F, eigenvectors Q, eigenvalues lam per
    factor, y, mask or None, noise variance s), with the dense posterior
    N(mu, Sigma) of the latent field at all N grid points."""

    def __init__(self, F, Q, lam, y, mask, s):
        self.F = [np.asarray(f, dtype=np.float64) for f in F]
        self.Q = [np.asarray(q, dtype=np.float64) for q in Q]
        self.QT = [q.T for q in self.Q]
        self.t = mr.kron_eigs([np.asarray(l, dtype=np.float64).reshape(-1) for l in lam])
        self.n = self.t.size
        self.s = float(s)
        self.mask = None if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
        obs = np.arange(self.n) if self.mask is None else np.nonzero(self.mask)[0]
        self.obs = obs
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        self.y = y
        self.K = mr.dense_K(self.F)
        self.Ko = self.K[:, obs]
        self.Ainv = np.linalg.inv(self.K[np.ix_(obs, obs)] + self.s * np.eye(obs.size))
        self.mu = self.Ko.dot(self.Ainv.dot(y[obs]))
        Sig = self.K - self.Ko.dot(self.Ainv).dot(self.Ko.T)
        self.Sigma = 0.5 * (Sig + Sig.T)

    def prior_draw(self, seed, k):
        return oracle.kron_matvec(self.Q, prior_coeffs(self.t, normal_stream(seed, 2 * k, self.n)))

    def matheron_draw(self, seed, k):
        f = self.prior_draw(seed, k)
        b = residual(self.y, f, self.mask, np.sqrt(self.s), normal_stream(seed, 2 * k + 1, self.n))
        return f + self.Ko.dot(self.Ainv.dot(b[self.obs]))

    def eigen_draw(self, seed, k):
        assert self.mask is None
        yt = oracle.kron_matvec(self.QT, self.y)
        c = posterior_coeffs(self.t, self.s, yt, normal_stream(seed, 2 * k, self.n))
        return oracle.kron_matvec(self.Q, c)

    def draws(self, route, seed, count):
        fn = self.matheron_draw if route == "matheron" else self.eigen_draw
        return np.stack([fn(seed, k) for k in range(count)], axis=1)


def sample_scores(D, X):
    """The four standardised deviations of S draws X (N x S) from N(mu, Sigma):
    max |mean_S - mu| / (sigma / sqrt(S)), max |var_S / Sigma_ii - 1| /
    sqrt(2 / (S - 1)), and for the draws whitened by Sigma (covariance C about
    the known mean) max off-diagonal |C - I| sqrt(S) and max |C_ii - 1|
    sqrt(S / 2)."""
    S = X.shape[1]
    sd = np.sqrt(np.diag(D.Sigma))
    zmean = np.max(np.abs(X.mean(axis=1) - D.mu) / (sd / np.sqrt(S)))
    zvar = np.max(np.abs(X.var(axis=1, ddof=1) / sd ** 2 - 1.0)) / np.sqrt(2.0 / (S - 1))
    w, V = np.linalg.eigh(D.Sigma)
    Wh = (V / np.sqrt(w)).dot(V.T)
    Y = Wh.dot(X - D.mu[:, None])
    C = Y.dot(Y.T) / S
    off = C - np.diag(np.diag(C))
    return zmean, zvar, np.max(np.abs(off)) * np.sqrt(S), \
        np.max(np.abs(np.diag(C) - 1.0)) * np.sqrt(S / 2.0)
