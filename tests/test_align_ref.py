"""tests/align_ref.py on the host: the float64 correlation and align_ref against scipy.signal.correlate(..., method='direct')
and the reference's find_audio_offset formula (utils.py:137-165), the tie rule on integer-valued tracks, and a sensitivity proof
for the per-bin metric that holds v3d_xcorr: an error of 0.1 % in ONE spectrum bin stands far above a float32 FFT's own noise in
that metric, and far below the old max-norm tolerance."""
import numpy as np
import pytest
import scipy.fft
from scipy import signal

import align_ref as AR


def _find_audio_offset(a1, a2):
    """the reference's formula on float64 tracks with the direct method: (lag, c, strength)"""
    x1 = (a1 - np.mean(a1)) / (np.std(a1) + 1e-10)
    x2 = (a2 - np.mean(a2)) / (np.std(a2) + 1e-10)
    c = signal.correlate(x2, x1, mode="full", method="direct")
    k = int(np.argmax(np.abs(c)))
    return k - (len(x1) - 1), c[k], np.abs(c[k]) / np.sqrt(np.sum(x1 ** 2) * np.sum(x2 ** 2))


SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (5, 1), (1, 9), (2, 700), (17, 5), (64, 64), (100, 257), (301, 212), (400, 400)]


@pytest.mark.parametrize("n1,n2", SIZES)
def test_correlation_against_scipy_direct(n1, n2):
    rng = np.random.default_rng(n1 * 1000 + n2)
    a1, a2 = rng.standard_normal(n1) * 3 + 0.5, rng.standard_normal(n2) - 0.25
    want = signal.correlate(a2, a1, mode="full", method="direct")
    got = AR._ref_corr(a1, a2)
    assert got.shape == want.shape == (n1 + n2 - 1,)
    scale = np.linalg.norm(a1) * np.linalg.norm(a2)
    assert np.abs(got - want).max() <= 1e-13 * scale
    for L in range(-(n1 - 1), n2):
        assert abs(AR._direct(a1, a2, L) - want[L + n1 - 1]) <= 1e-13 * scale
    N = 1 << AR.fft_log(n1, n2)
    assert N >= max(1024, n1 + n2 - 1) and (N == 1024 or N // 2 < n1 + n2 - 1)
    circ = AR.circular(want, n1, n2, N)
    for L in range(-(n1 - 1), n2):
        assert circ[L % N] == want[L + n1 - 1]
    assert np.count_nonzero(circ) <= n1 + n2 - 1


def test_normalise_rounds_to_float32():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(1001) * 0.3 + 2).astype(np.float32)
    x = AR.normalise(a)
    a64 = a.astype(np.float64)
    full = (a64 - a64.mean()) / (a64.std() + 1e-10)
    assert x.dtype == np.float64 and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    assert np.array_equal(x, full.astype(np.float32).astype(np.float64)) and not np.array_equal(x, full)
    assert not AR.normalise(np.full(7, 3.25, np.float32)).any()                 # a constant track: all zeros
    pm = np.float32([1, -1, -1, 1, 1, -1])
    assert np.array_equal(AR.normalise(pm), pm.astype(np.float64))              # balanced +-1: exactly +-1 in float32


@pytest.mark.parametrize("n1,n2,lag", [(300, 300, 0), (300, 257, 41), (212, 301, -77), (150, 400, 249), (400, 150, -260)])
def test_align_ref_against_the_reference_formula(n1, n2, lag):
    rng = np.random.default_rng(n1 + n2 + abs(lag))
    p1 = max(lag, 0) + 3
    s = rng.standard_normal(max(p1 + n1, p1 - lag + n2) + 1)
    a1 = (s[p1:p1 + n1] + 0.2 * rng.standard_normal(n1)).astype(np.float32)
    a2 = (-0.7 * s[p1 - lag:p1 - lag + n2] + 0.2 * rng.standard_normal(n2) + 0.01).astype(np.float32)
    L, c, strength, sd, tied = AR.align_ref(a1, a2)
    wl, wc, ws = _find_audio_offset(a1.astype(np.float64), a2.astype(np.float64))
    assert L == wl == lag and tied == [lag] and c < 0
    assert abs(c - wc) <= 1e-6 * np.sqrt(n1 * n2) and abs(strength - ws) <= 1e-6          # float32 rounding of the tracks
    assert sd == min(np.std(a1.astype(np.float64)), np.std(a2.astype(np.float64)))
    x1, x2 = AR.normalise(a1), AR.normalise(a2)
    direct = signal.correlate(x2, x1, mode="full", method="direct")
    k = int(np.argmax(np.abs(direct)))
    assert k - (n1 - 1) == L and abs(direct[k] - c) <= 1e-12 * np.sqrt(n1 * n2)
    oracle = AR._oracle_align(a1, a2)
    assert oracle[0] == L and abs(oracle[2] - strength) <= 1e-6


def test_tie_rule_on_integer_tracks():
    rng = np.random.default_rng(3)
    for n1 in (6, 50, 200):
        a1 = np.repeat(np.float32([1, -1]), n1 // 2)
        rng.shuffle(a1)
        a2 = np.concatenate([a1, a1])
        L, c, strength, sd, tied = AR.align_ref(a1, a2)
        direct = signal.correlate(a2.astype(np.float64), a1.astype(np.float64), mode="full", method="direct")
        assert np.array_equal(direct, np.rint(direct)) and np.abs(direct).max() == n1
        assert tied == sorted(np.flatnonzero(np.abs(direct) == n1) - (n1 - 1)) and {0, n1} <= set(tied)
        assert L == tied[0] and abs(c) == n1 and sd == 1.0
        assert strength == n1 / np.sqrt(n1 * 2 * n1)
    # a negative and a positive peak of one size tie: |c| decides, the smallest lag is reported
    a1 = np.float32([1, -1])
    a2 = np.float32([1, -1, 1, -1, 1, -1, 1, -1])
    L, c, _, _, tied = AR.align_ref(a1, a2)
    assert tied == [0, 1, 2, 3, 4, 5, 6] and L == 0 and c == 2.0
    assert AR._direct(AR.normalise(a1), AR.normalise(a2), 1) == -2.0
    # a track that normalises to zero ties every valid lag at c = 0
    L, c, strength, sd, tied = AR.align_ref(np.float32([2, 2, 2, 2, 2]), np.float32([7]))
    assert (L, c, strength, sd) == (-4, 0.0, 0.0, 0.0) and tied == [-4, -3, -2, -1, 0]
    L, c, strength, _, tied = AR.align_ref(np.float32([4]), np.float32([1, 5]))
    assert (L, c, strength) == (0, 0.0, 0.0) and tied == [0, 1]


def test_plan_digits_and_sizes():
    assert [AR.plan_digits(m) for m in (10, 12, 13, 18, 19, 24, 26)] == [[10], [12], [7, 6], [9, 9], [7, 6, 6], [8, 8, 8], [9, 9, 8]]
    last = {AR.plan_digits(m)[-1] for m in range(10, 21)}
    cols = {d for m in range(10, 21) for d in AR.plan_digits(m)[:-1]}
    assert last == set(range(6, 13)) and cols == {6, 7, 8, 9}                   # every LOG_R of the kernels within m = 10 .. 20
    for m in range(10, 25):
        for exact in (False, True):
            n1, n2 = AR.xcorr_sizes(m, exact)
            N = 1 << m
            assert n1 % 2 == 1 and n1 != n2 and N // 2 < n1 + n2 - 1 <= N and (n1 + n2 - 1 == N) == exact
            assert AR.fft_log(n1, n2) == m


# ---------------------------------------------------------------- the metric's sensitivity

def _host_float32_xcorr(a1, a2, N):
    """the device's pipeline on the host in float32: z = a1 + i a2 (complex64), one complex FFT, the two real spectra separated
    from Z[k] and conj Z[N-k], conj(A) B, inverse FFT (scipy.fft keeps complex64) -> the 'full' correlation"""
    n1, n2 = a1.size, a2.size
    z = np.zeros(N, np.complex64)
    z[:n1] = a1
    z[:n2] += np.complex64(1j) * a2
    Z = scipy.fft.fft(z)
    assert Z.dtype == np.complex64
    Zr = np.conj(np.roll(Z[::-1], 1))
    A = np.complex64(0.5) * (Z + Zr)
    B = np.complex64(-0.5j) * (Z - Zr)
    c = scipy.fft.ifft(np.conj(A) * B)
    assert c.dtype == np.complex64
    c = c.real.astype(np.float64)
    return np.concatenate([c[N - (n1 - 1):], c[:n2]])


@pytest.mark.parametrize("m", [10, 13, 16, 19])
def test_metric_sees_one_bin_off_by_a_thousandth(m):
    """zero-mean white float32 tracks.  noise: the metric of a host float32 pipeline (1.3 to 1.9 units here).  seeded: the
    float64 correlation with the bin of median |P_k| scaled by 1.001 -- what a wrong twiddle entry or a wrong conjugate on one
    (k, N-k) pair does at the very least.  The seeded error is at least 50 times the noise; the lag-domain tolerance the suite used
    alone before, max |got - want| <= 1e-5 |a1| |a2|, does not see it."""
    N = 1 << m
    n1, n2 = AR.xcorr_sizes(m)
    rng = np.random.default_rng(m)
    a1, a2 = AR.white(n1, rng), AR.white(n2, rng)
    want = AR._ref_corr(a1, a2)
    noise = AR.spectral_error(_host_float32_xcorr(a1, a2, N), a1, a2)
    assert 0.2 <= noise <= 4.0, noise                            # a float32 FFT pipeline: of the order of eps32 log2 N per bin
    assert AR.spectral_error(want, a1, a2) <= 1e-6 and AR.spectral_error(want, a1, a2, want) == 0.0

    P = np.conj(np.fft.rfft(a1.astype(np.float64), N)) * np.fft.rfft(a2.astype(np.float64), N)
    k = int(np.argsort(np.abs(P[1:-1]))[(P.size - 2) // 2]) + 1
    P[k] *= 1.001
    c = np.fft.irfft(P, N)
    seeded = np.concatenate([c[N - (n1 - 1):], c[:n2]])
    err = AR.spectral_error(seeded, a1, a2)
    assert abs(err - AR.spectral_error(seeded, a1, a2, want)) <= 1e-6 * err               # both forms of D agree
    print(f"m={m}: float32 pipeline {noise:.3f} units, seeded bin {k}: {err:.1f} units = {err * AR.EPS32 * m:.3e} absolute, ratio {err / noise:.0f}")
    assert err >= 50 * noise, (m, err, noise)
    assert err >= 10 * 8, (m, err)                               # ten times a K of 8 units
    old_tol = 1e-5 * np.linalg.norm(a1.astype(np.float64)) * np.linalg.norm(a2.astype(np.float64))
    assert np.abs(seeded - want).max() <= 0.5 * old_tol, (m, np.abs(seeded - want).max(), old_tol)
