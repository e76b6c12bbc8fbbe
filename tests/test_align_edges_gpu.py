"""v3d_xcorr held per spectrum bin on every FFT plan, and v3d_align_audio at the edges of its peak search, against the float64
restatement tests/align_ref.py (checked on the host by tests/test_align_ref.py).

The lag-domain bound of tests/test_align_gpu.py, max |got - want| <= 1e-5 |a1| |a2|, divides an error in one spectrum bin by N: a
twiddle entry, a conjugate on one (k, N-k) pair or one twiddle product that is off by 0.1 % passes it at every size.
align_ref.spectral_error does not divide: the same error is 550 to 1000 units there (test_align_ref.py), the kernel's own
rounding 1.3 to 3.8."""
import numpy as np
import pytest
import torch

import align_ref as AR

pytestmark = pytest.mark.gpu

# The bound on align_ref.spectral_error and impulse_error, in units of eps32 log2 N: four times the largest value measured on
# one MI355X over m = 10 .. 24 against the float64 reference -- 3.731, at m = 23; one pass 1.3 to 2.6, two passes 1.7 to 2.8, three
# passes 2.5 to 3.7 (per-m values in profiles/align_accuracy.json, written by tools/align_accuracy.py, and in DESIGN.md, "Audio
# alignment").  The factor of four covers the spread between seeds and sizes that one run does not show; one spectrum bin off
# by 0.1 % is 550 units or more (test_align_ref.py), a host float32 pipeline 1.3 to 1.9.
K = 4 * 3.731


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---------------------------------------------------------------- v3d_xcorr

SPECTRAL = [(m, False) for m in range(10, 21)] + [(m, True) for m in (10, 13, 19)]


@pytest.mark.parametrize("m,exact", SPECTRAL, ids=[f"2^{m}{'-exact' if e else ''}" for m, e in SPECTRAL])
def test_xcorr_per_bin(native, m, exact):
    """zero-mean white float32 tracks, n1 odd and unequal to n2, n1 + n2 - 1 in (N/2, N] (== N for the exact cases), in both
    orders (either track in the real part of the packed signal).  m = 10 .. 20 takes one, two and three passes, every LOG_R from
    6 to 12 on the last digit and 6 to 9 on the column passes (test_align_ref.py::test_plan_digits_and_sizes)."""
    rng = np.random.default_rng(m + 100 * exact)
    n1, n2 = AR.xcorr_sizes(m, exact)
    for n1, n2 in ((n1, n2), (n2, n1)):
        a1, a2 = AR.white(n1, rng), AR.white(n2, rng)
        got = native.xcorr(_dev(a1), _dev(a2)).cpu().numpy().astype(np.float64)
        assert got.shape == (n1 + n2 - 1,)
        units = AR.spectral_error(got, a1, a2)
        print(f"xcorr 2^{m} ({n1}, {n2}): {units:.3f} units of eps32 log2 N per bin")
        assert units <= K, (m, n1, n2, units, K)


def _digit_bits(m, pattern):
    """an index with `pattern` (a few low bits) set in every digit of the 2^m plan"""
    idx, lo = 0, m
    for d in AR.plan_digits(m):
        lo -= d
        idx |= pattern << lo
    return idx


@pytest.mark.parametrize("m", list(range(10, 21)))
def test_xcorr_of_two_impulses(native, m):
    """a1 = delta at p, a2 = delta at q: 1 at lag q - p, 0 elsewhere.  Both spectra are pure twiddles, so a storage position
    mapped to the wrong frequency anywhere (the digit-reversed order, the pair k / N-k, the extraction's wrap) moves or smears the
    peak.  The last pair has bits set in every digit of the plan (p = 5, q = 3 in each digit: a negative lag, through the wrap)."""
    n1, n2 = AR.xcorr_sizes(m)
    pairs = [(0, 0), (n1 - 1, 0), (0, n2 - 1), (_digit_bits(m, 5), _digit_bits(m, 3))]
    assert 0 < pairs[-1][1] < pairs[-1][0] < min(n1, n2)
    for p, q in pairs:
        a1, a2 = np.zeros(n1, np.float32), np.zeros(n2, np.float32)
        a1[p] = a2[q] = 1
        got = native.xcorr(_dev(a1), _dev(a2)).cpu().numpy()
        units = AR.impulse_error(got, n1, n2, p, q)
        print(f"impulses 2^{m} p={p} q={q}: {units:.3f} units")
        assert int(np.argmax(np.abs(got))) == q - p + n1 - 1, (m, p, q)
        assert units <= K, (m, p, q, units, K)


# ---------------------------------------------------------------- v3d_align_audio

def _hold(native, a1, a2, lag=None, tie=False):
    """v3d_align_audio against align_ref: lag exact (any member of the tied set with `tie`), |strength - ref| <= 1e-6,
    |c - ref| <= 1e-6 sqrt(n1 n2), std to 1e-9.  `lag`: where the case means the peak to be -- the reference must agree first."""
    a1, a2 = np.ascontiguousarray(a1, np.float32), np.ascontiguousarray(a2, np.float32)
    n1, n2 = a1.size, a2.size
    assert max(n1, n2) <= 70000
    L, c, strength, sd, tied = AR.align_ref(a1, a2)
    if lag is not None:
        assert L == lag and tied == [lag], (L, tied[:5])
    got = native.align_audio(_dev(a1), _dev(a2)).cpu().numpy()
    print(f"({n1}, {n2}): got {got.tolist()}, want lag {L} c {c!r} strength {strength!r} ({len(tied)} tied)")
    assert got[0] == int(got[0])
    if tie:
        assert int(got[0]) in set(tied), (got.tolist(), tied[:5])
        c = AR._direct(AR.normalise(a1), AR.normalise(a2), int(got[0]))      # ties may differ in sign
    else:
        assert len(tied) == 1 and int(got[0]) == L, (got.tolist(), L)
    assert abs(got[2] - strength) <= 1e-6, (got[2], strength)
    assert abs(got[1] - c) <= 1e-6 * np.sqrt(n1 * n2), (got[1], c)
    assert abs(got[3] - sd) <= 1e-9 * sd
    return got


def test_align_inverted_polarity(native):
    """a mis-wired microphone: the peak is negative (a max(c) in place of max|c| loses it)"""
    a1, a2 = AR._tracks(20000, 21000, 777, 5, gain=-0.7)
    got = _hold(native, a1, a2, 777)
    assert got[1] < 0 and got[2] > 0.9


@pytest.mark.parametrize("n1,n2,lag", [(20000, 20005, L) for L in (4095, 4096, -1, -4096, -4097)]
                         + [(40000, 40005, L) for L in (4096, -1, 8191)])
def test_align_peak_beside_a_nomination_block_edge(native, n1, n2, lag):
    """the peak on either side of a 4096-lag block of k_xc_blockmax (its +-2 neighbours come from the next block's lags) and at
    index N - 1 of the circular buffer; 16 blocks (== TOPK, N = 2^16) and 32 (N = 2^17)"""
    assert (1 << AR.fft_log(n1, n2)) // 4096 == (16 if n1 == 20000 else 32)
    _hold(native, *AR._tracks(n1, n2, lag, n1 + abs(lag)), lag)


@pytest.mark.parametrize("reverse", [False, True], ids=["lag=n2-1", "lag=-(n1-1)"])
def test_align_extreme_lags(native, reverse):
    """an overlap of one sample: a unit spike at a1[0] and a2[-1] in 1e-3 noise (lag n2 - 1); both reversed (lag -(n1 - 1))"""
    rng = np.random.default_rng(8)
    n1, n2 = 3000, 3500
    a1, a2 = (1e-3 * rng.standard_normal(n1)).astype(np.float32), (1e-3 * rng.standard_normal(n2)).astype(np.float32)
    a1[0] = a2[-1] = 1
    if reverse:
        a1, a2 = a1[::-1], a2[::-1]
    _hold(native, a1, a2, -(n1 - 1) if reverse else n2 - 1)


@pytest.mark.parametrize("n1", [32767, 32768, 32769])
def test_align_direct_sum_chunks(native, n1):
    """n1 on both sides of DIRECT_CHUNK = 32768: one chunk, one full chunk, a second chunk of one sample"""
    _hold(native, *AR._tracks(n1, 30000, -2500, n1), -2500)


@pytest.mark.parametrize("n1,n2", [(512, 513), (513, 513), (2048, 2049), (2049, 2049), (4096, 4097), (4097, 4097)])
def test_align_exact_and_just_over_sizes(native, n1, n2):
    """n1 + n2 - 1 == N (no padding: every index of the circle is a valid lag) and N / 2 + 1 (the next size, mostly padding)"""
    need = n1 + n2 - 1
    assert need == 1 << AR.fft_log(n1, n2) or need - 1 == 1 << (AR.fft_log(n1, n2) - 1)
    _hold(native, *AR._tracks(n1, n2, 100, n1 + n2), 100)


@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (5, 1), (2, 700)])
def test_align_tiny_tracks(native, n1, n2):
    """a track of one sample normalises to zero (every lag ties at c = 0); two samples normalise to +-1 (ties are common)"""
    rng = np.random.default_rng(10 * n1 + n2)
    _hold(native, rng.standard_normal(n1), rng.standard_normal(n2), tie=True)


def _balanced(n, seed):
    a = np.repeat(np.float32([1, -1]), n // 2)
    np.random.default_rng(seed).shuffle(a)
    return a


def test_align_exact_tie_in_two_blocks(native):
    """balanced +-1 tracks normalise to exactly +-1, so every c is an exact integer: a2 = [a1, a1] ties lags 0 and n1 at |c| = n1.
    n1 = 5000 puts them into different nomination blocks, both are nominated, and the smaller lag wins"""
    a1 = _balanced(5000, 1)
    L, c, strength, _, tied = AR.align_ref(a1, np.concatenate([a1, a1]))
    assert tied == [0, 5000] and c == 5000.0
    got = _hold(native, a1, np.concatenate([a1, a1]), tie=True)
    assert got[0] == 0 and got[1] == 5000.0 and got[2] == strength


def test_align_exact_tie_in_one_block(native):
    """n1 = 1000: both tied lags sit in one block, which nominates one of them by the float32 FFT's rounding: either is right,
    c and strength are exact"""
    a1 = _balanced(1000, 2)
    L, c, strength, _, tied = AR.align_ref(a1, np.concatenate([a1, a1]))
    assert tied == [0, 1000] and c == 1000.0
    got = _hold(native, a1, np.concatenate([a1, a1]), tie=True)
    assert got[0] in (0, 1000) and got[1] == 1000.0 and got[2] == strength


def test_align_constant_track_over_64_blocks(native):
    """a constant track (normalised: all zeros) against noise at n = 70000, N = 2^18, 64 blocks > TOPK: every c is 0, the lag is
    any valid one, c = 0 and strength = 0 exactly"""
    n = 70000
    a2 = np.random.default_rng(4).standard_normal(n).astype(np.float32)
    for a1, b in ((np.full(n, 3.25, np.float32), a2), (a2, np.full(n, 3.25, np.float32))):
        got = _hold(native, a1, b, tie=True)
        assert -(n - 1) <= got[0] <= n - 1 and got[1] == 0 and got[2] == 0


RANGES = [(1e-12, 0, 1, 0), (1e15, 0, 1e-15, 0), (1e-3, 1e4, 1, -300), (1e-10, 0, 1e-10, 0)]
QUIET = [(1e-18, 0, 1, 0), (1, 0, 1e-18, 0), (1e-18, 0, 1e-18, 0)]


def _scaled(s1, o1, s2, o2):
    a1, a2 = AR._tracks(20000, 21000, 321, 11)
    return (a1.astype(np.float64) * s1 + o1).astype(np.float32), (a2.astype(np.float64) * s2 + o2).astype(np.float32)


@pytest.mark.parametrize("s1,o1,s2,o2", RANGES)
def test_align_dynamic_range(native, s1, o1, s2, o2):
    """the domain of the header: finite samples, |a| <= 1e15, a std well above and around the 1e-10 of the normalisation, an
    offset that leaves float32 four digits of signal"""
    _hold(native, *_scaled(s1, o1, s2, o2), 321)


@pytest.mark.parametrize("s1,o1,s2,o2", QUIET, ids=["a1", "a2", "both"])
def test_align_quiet_tracks(native, s1, o1, s2, o2):
    """std = 3e-19, the lower edge of the header's domain: an = (a - mean) / (std + 1e-10) is 3e-9 per sample, so the packing
    norm must follow std / (std + 1e-10) -- with sqrt(n) the quiet track is packed 3e-9 below its partner, under the float32
    FFT's rounding of it, and the nominations are noise"""
    _hold(native, *_scaled(s1, o1, s2, o2), 321)
