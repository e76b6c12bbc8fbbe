"""Audio alignment restated in float64 (the contract of v3d_xcorr / v3d_align_audio in include/v3d_hip.h), the synthetic tracks
the alignment tests share, and the per-bin error metric that holds v3d_xcorr's float32 FFT.  Test infrastructure: checked on the
host by tests/test_align_ref.py, used on the device by tests/test_align_gpu.py, test_align_edges_gpu.py and
tools/align_accuracy.py."""
import numpy as np

RATE = 22050
EPS32 = 2.0 ** -24
XC_MIN_LOG = 10                                               # v3d_align.hip: N never below 2^10


def fft_log(n1, n2):
    """m of the device's FFT size N = 2^m: the smallest power of two >= n1 + n2 - 1, at least 2^10"""
    return max(XC_MIN_LOG, int(n1 + n2 - 2).bit_length())


def _ref_corr(a1, a2):
    """float64 scipy.signal.correlate(a2, a1, 'full'): index k = lag + n1 - 1"""
    a1 = np.asarray(a1, np.float64)
    a2 = np.asarray(a2, np.float64)
    n1, n2 = a1.size, a2.size
    n = 1 << int(np.ceil(np.log2(n1 + n2 - 1)))
    c = np.fft.irfft(np.conj(np.fft.rfft(a1, n)) * np.fft.rfft(a2, n), n)
    return np.concatenate([c[n - (n1 - 1):], c[:n2]]) if n1 > 1 else c[:n2]


def _direct(a1, a2, L):
    """c(L) = sum_n a2[n + L] a1[n] in float64"""
    a1 = np.asarray(a1, np.float64)
    a2 = np.asarray(a2, np.float64)
    lo, hi = max(0, -L), min(a1.size, a2.size - L)
    return float(np.dot(a2[lo + L:hi + L], a1[lo:hi])) if hi > lo else 0.0


def _norm64(a):
    a = np.asarray(a, np.float64)
    return (a - a.mean()) / (a.std() + 1e-10)


def _band_noise(n, rng, lo=80.0, hi=5000.0):
    """band-limited noise plus a few tones"""
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / RATE)
    spec[(f < lo) | (f > hi)] = 0
    x = np.fft.irfft(spec, n)
    t = np.arange(n) / RATE
    for fr, amp in ((220.0, 0.3), (997.0, 0.2), (3150.0, 0.1)):
        x += amp * x.std() * np.sin(2 * np.pi * fr * t + rng.uniform(0, 6))
    return x / np.abs(x).max()


def _tracks(n1, n2, lag, seed, noise=0.2, gain=0.7):
    """a1[n] ~ a2[n + lag]: two recordings of one source, each with its own noise, float32; `gain` is the second recording's
    (negative: inverted polarity)"""
    rng = np.random.default_rng(seed)
    p1 = max(lag, 0) + 17
    p2 = p1 - lag
    s = _band_noise(max(p1 + n1, p2 + n2) + 1, rng)
    a1 = s[p1:p1 + n1] + noise * rng.standard_normal(n1) * s.std()
    a2 = gain * s[p2:p2 + n2] + noise * rng.standard_normal(n2) * s.std() + 0.01
    return a1.astype(np.float32), a2.astype(np.float32)


def _oracle_align(a1, a2):
    """find_audio_offset in float64: (lag, signed c, strength, min std)"""
    x1, x2 = _norm64(a1), _norm64(a2)
    c = _ref_corr(x1, x2)
    k = int(np.argmax(np.abs(c)))
    strength = abs(c[k]) / np.sqrt(np.sum(x1 * x1) * np.sum(x2 * x2))
    return k - (a1.size - 1), c[k], strength, min(np.std(a1.astype(np.float64)), np.std(a2.astype(np.float64)))


def white(n, rng):
    """zero-mean white float32 track (the mean removed after the rounding, so it is zero to float32 precision)"""
    a = rng.standard_normal(n).astype(np.float32)
    return (a - np.float32(a.astype(np.float64).mean())).astype(np.float32)


# ---------------------------------------------------------------- v3d_align_audio

def normalise(a):
    """an = (a - mean) / (std + 1e-10) with the float64 mean and population std, rounded to float32 (the header's rule);
    returned as float64"""
    a = np.asarray(a, np.float64)
    return ((a - a.mean()) / (a.std() + 1e-10)).astype(np.float32).astype(np.float64)


def align_ref(a1, a2):
    """(lag, c(lag), strength, min(std1, std2), tied lags) by the header's rule on direct float64 sums of the rounded normalised
    tracks.  A float64 FFT correlation finds every lag within 1e-9 (relative) of the maximum |c|; those lags are re-evaluated by
    direct sums; the tied set (sorted) holds the lags whose direct |c| equal the maximum exactly, and lag is its smallest member.
    A track that normalises to all zeros ties every valid lag at c = 0."""
    x1, x2 = normalise(a1), normalise(a2)
    n1, n2 = x1.size, x2.size
    sd = min(float(np.std(np.asarray(a1, np.float64))), float(np.std(np.asarray(a2, np.float64))))
    e = float(np.sum(x1 * x1) * np.sum(x2 * x2))
    if not x1.any() or not x2.any():
        return -(n1 - 1), 0.0, 0.0, sd, list(range(-(n1 - 1), n2))
    c = np.abs(_ref_corr(x1, x2))
    near = np.flatnonzero(c >= c.max() * (1 - 1e-9) - 1e-12 * np.sqrt(e)) - (n1 - 1)
    vals = {int(L): _direct(x1, x2, int(L)) for L in near}
    top = max(abs(v) for v in vals.values())
    tied = sorted(L for L, v in vals.items() if abs(v) == top)
    lag = tied[0]
    return lag, vals[lag], abs(vals[lag]) / np.sqrt(e), sd, tied


# ---------------------------------------------------------------- v3d_xcorr

def circular(c, n1, n2, N):
    """a 'full' correlation (index k = lag + n1 - 1) as a length-N circular array: lag L at index L mod N, zeros where no lag exists"""
    out = np.zeros(N, np.float64)
    c = np.asarray(c, np.float64)
    out[:n2] = c[n1 - 1:]
    if n1 > 1:
        out[N - (n1 - 1):] = c[:n1 - 1]
    return out


def spectral_error(got, a1, a2, want=None):
    """the largest error of any one bin of the correlation's spectrum, relative to the rms bin of the true cross spectrum, in
    units of eps32 log2 N (eps32 = 2^-24): D = rfft(got - want) on the length-N circle, P = conj(rfft(a1, N)) rfft(a2, N),
    max_k |D_k| / sqrt(mean_k |P_k|^2) / (eps32 log2 N).  `want` defaults to the float64 correlation of a1 and a2.  A max-norm
    bound in the lag domain divides a one-bin error by N; this metric does not.  (The float64 correlation on the circle is
    irfft(P): without `want` D is taken as rfft(got) - P, the same thing with three transforms fewer.)"""
    n1, n2 = np.size(a1), np.size(a2)
    m = fft_log(n1, n2)
    N = 1 << m
    P = np.conj(np.fft.rfft(np.asarray(a1, np.float64), N)) * np.fft.rfft(np.asarray(a2, np.float64), N)
    if want is None:
        D = np.fft.rfft(circular(got, n1, n2, N)) - P
    else:
        D = np.fft.rfft(circular(got, n1, n2, N) - circular(want, n1, n2, N))
    return float(np.abs(D).max() / np.sqrt(np.mean(np.abs(P) ** 2)) / (EPS32 * m))


def impulse_error(got, n1, n2, p, q):
    """a1 = delta at p, a2 = delta at q: the largest deviation of `got` from 1 at lag q - p and 0 elsewhere, in units of
    eps32 log2 N"""
    want = np.zeros(n1 + n2 - 1, np.float64)
    want[q - p + n1 - 1] = 1.0
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (EPS32 * fft_log(n1, n2)))


def plan_digits(m):
    """v3d_align.hip's FftPlan: the digit widths of the passes of a 2^m-point FFT (pass 0 has the largest stride)"""
    if m <= 12:
        return [m]
    passes = (m + 8) // 9
    return [m // passes + (1 if i < m % passes else 0) for i in range(passes)]


def xcorr_sizes(m, exact=False):
    """(n1, n2) for the FFT size 2^m: n1 odd, n1 != n2, n1 + n2 - 1 in (N/2, N] -- == N when `exact`"""
    N = 1 << m
    need = N if exact else N - 37 if m > 10 else N - 5
    n1 = (need * 3 // 5) | 1
    return n1, need + 1 - n1
