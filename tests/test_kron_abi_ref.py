"""Pins tests/kron_abi_ref.py (the long-double reference of the Kronecker
operator section of the C ABI) against the oracle, and checks on the host that
NumPy's own float64 chain meets the elementwise bound
tests/test_gpu_kron_abi.py asserts on the device, for every shape of that
module: the bound is neither vacuous nor too tight.  No GPU."""
import numpy as np
import pytest

import kron_abi_ref as R
import oracle
from oracle import kron as okron

LD = np.longdouble


def rel(a, b):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_longdouble_is_extended():
    assert np.finfo(LD).eps < 2.0 ** -60


def test_fold_mask_model():
    for name in R.MATVEC_CASES:
        fs = R.matvec_case(name)[0]
        want = R.MATVEC_MASKS.get(name, 0)
        assert R.fold_mask(fs, False) == want and R.fold_mask(fs, True) == want, name
    fs = R.matvec_case("centro_nonsym")[0]
    assert not np.array_equal(fs[0], fs[0].T) and np.array_equal(fs[0], fs[0][::-1, ::-1])
    fs = R.matvec_case("centro_48_7_49")[0]
    assert np.array_equal(fs[2], fs[2].T) and np.array_equal(fs[2], fs[2][::-1, ::-1])


@pytest.mark.parametrize("name", sorted(R.MATVEC_CASES))
def test_numpy_meets_matvec_bound(name):
    """oracle.kron_matvec / kron_matvec_T (float64, BLAS) inside the bound,
    forward and transposed, shift 0 and (square operators) 0.37; the long
    double reference within 1e-13 of the oracle normwise."""
    fs, xf, xt = R.matvec_case(name)
    square = xf.size == xt.size
    mask = R.MATVEC_MASKS.get(name, 0)
    worst = 0.0
    for tr, x in ((False, xf), (True, xt)):
        got0 = oracle.kron_matvec_T(fs, x) if tr else oracle.kron_matvec(fs, x)
        for shift in (0.0, 0.37) if square else (0.0,):
            ref, mag = R.matvec_ref(fs, x, tr, shift, mask)
            assert ref.dtype == LD and ref.shape == mag.shape == got0.shape
            if shift == 0.0:
                assert np.all(mag >= np.abs(ref) * (1 - 1e-15))
            got = got0 + shift * x if shift != 0.0 else got0
            assert rel(ref, got) < 1e-13
            r = R.worst_ratio(got, ref, R.matvec_bound(fs, x, mag, tr, shift))
            print("numpy / bound, %s transpose=%d shift=%g c=%d: %.4f"
                  % (name, tr, shift, R.matvec_c(fs, tr), r))
            assert r <= 1.0, (name, tr, shift, r)
            worst = max(worst, r)
    # not vacuous: float64 NumPy uses a visible share of it.  (The worst case
    # c u mag is reached by errors that all align; random roundings add up
    # like sqrt(c), and mag exceeds |ref| by the cancellation of random signs,
    # so a long contraction sits near 1e-3 of its bound.)
    assert worst > 1e-4, worst


def test_matvec_ref_is_the_definition():
    """The staged reference against the dense expansion (kron_expand)."""
    for name in ("5x3", "growing", "shrinking", "mixed3"):
        fs, xf, xt = R.matvec_case(name)
        K = oracle.kron_expand(fs)
        assert rel(R.matvec_ref(fs, xf)[0], K @ xf) < 1e-13
        assert rel(R.matvec_ref(fs, xt, True)[0], K.T @ xt) < 1e-13
        assert rel(R.matvec_ref(fs, xf)[1], np.abs(K) @ np.abs(xf)) < 1e-13


@pytest.mark.parametrize("ms", R.BLOCK_OPS, ids=lambda m: "x".join(map(str, m)))
def test_numpy_meets_block_bound(ms):
    """oracle.kron.block_matvec (float64) inside the block-basis bound, whole
    layout and a ragged block range; the padding of the device layout stays
    zero; the reference is P K P^T of the grid reference."""
    fs = R.toeplitz_factors(ms)
    n = int(np.prod(ms))
    x = R.vector(n, 11)
    xb = okron.block_fold(x, ms, pad=True)
    padm = R.block_pad_mask(ms)
    nb = xb.size >> len(ms)
    assert padm.size == xb.size and int((~padm).sum()) == n
    assert (xb.size > n) == (ms == (4, 64, 64))
    assert np.all(xb[padm] == 0)
    got0 = okron.block_matvec(fs, xb, pad=True)
    assert np.all(got0[padm] == 0)
    for shift in (0.0, 0.05):
        ref, mag = R.block_matvec_ref(fs, xb, shift)
        assert np.all(ref[padm] == 0) and np.all(mag[padm] == 0)
        got = got0 + shift * xb
        assert rel(ref, got) < 1e-13
        r = R.worst_ratio(got, ref, R.block_bound(fs, xb, mag, shift))
        print("numpy / bound, block %s shift=%g c=%d: %.4f" % (ms, shift, R.block_c(fs), r))
        assert 1e-3 < r <= 1.0, (ms, shift, r)
        # the same operator as the grid's: unfold(block matvec(fold x)) = K x
        back = okron.block_fold(np.asarray(ref, dtype=np.float64), ms, inverse=True, pad=True)
        assert rel(back, oracle.kron_matvec(fs, x) + shift * x) < 1e-13
        if len(ms) >= 2:
            blk0, nblk = 1, 3
            rr, rm = R.block_matvec_ref(fs, xb[blk0 * nb:(blk0 + nblk) * nb], shift, True, blk0,
                                        nblk)
            assert np.array_equal(rr, ref[blk0 * nb:(blk0 + nblk) * nb])
            assert np.array_equal(rm, mag[blk0 * nb:(blk0 + nblk) * nb])


def test_toeplitz_factors_are_centrosymmetric_spd():
    for F in R.toeplitz_factors((4, 40, 64)):
        assert np.array_equal(F, F[::-1, ::-1]) and np.array_equal(F, F.T)
        lam = np.linalg.eigvalsh(F)
        assert lam[0] > 0.4 and lam[-1] < 2.5
