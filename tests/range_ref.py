"""NumPy restatement of the robust depth range contract (include/v3d_hip.h, v3d_range.hip).  Test infrastructure: the GPU entry
is compared with these functions bit for bit.  All arithmetic is integer except the final conversion of the white point.

q is the percentile in parts per 10000, an integer in [5000, 10000]; a frame is float32 [H,W] (d16 = rint(16 D) >= 1 valid)."""
import numpy as np

import temporal_ref as TR

NB = 2048
Q_MIN, Q_OFF = 5000, 10000


def histogram(frame):
    """hist[b] = #{d16 == b} for 1 <= b <= 2046, hist[2047] = #{d16 >= 2047}; hist[0] stays 0: invalid pixels are not counted
    (NaN and -inf are invalid, +inf lands in the last bin: TR.d16_of)"""
    d16 = TR.d16_of(frame).reshape(-1)
    return np.bincount(np.minimum(d16[d16 >= 1], NB - 1), minlength=NB).astype(np.int64)


def rank_of(q, n_valid):
    """k = max(1, ceil(q n_valid / 10000)) in exact integers"""
    return max(1, -(-int(q) * int(n_valid) // 10000))


def select(hist, q):
    """(n_valid, k, hi16): hi16 the smallest b whose cumulative count reaches k (None for an empty histogram)"""
    n_valid = int(hist.sum())
    if n_valid == 0:
        return 0, 0, None
    k = rank_of(q, n_valid)
    return n_valid, k, int(np.searchsorted(np.cumsum(hist), k, side="left"))


def white_point(frame, q):
    """(mn, hi) of one frame as float32; a frame that holds a NaN gives (NaN, NaN) whatever its histogram says"""
    f = np.asarray(frame, np.float32)
    mn, mx = TR.minmax(f.reshape(1, -1))[0]
    if np.isnan(mn):
        return mn, mx
    n_valid, _, hi16 = select(histogram(f), q)
    if n_valid == 0 or hi16 == NB - 1:
        return mn, mx
    return mn, max(np.float32(hi16) / np.float32(16), mn)


def robust_minmax(depth, q):
    """float32 [T,H,W] -> float32 [T,2] = (mn, hi): the layout TR.minmax gives, for TR.ranges and TR.to_u16_range"""
    if not Q_MIN <= q <= Q_OFF:
        raise ValueError(f"q = {q} outside [{Q_MIN}, {Q_OFF}]")
    return np.array([white_point(f, q) for f in np.asarray(depth, np.float32)], np.float32).reshape(len(depth), 2)


def to_u16(depth, q):
    """radius 0: every frame against its own (mn, hi)"""
    return TR.to_u16_range(depth, robust_minmax(depth, q))


def stabilize(depth, gray, R, tau=12, c=20, fill=1, t0=0, n=None, q=Q_OFF):
    """TR.stabilize with the per-frame max replaced by the robust white point"""
    cut = TR.cuts(gray, c)
    filt = TR.filter_clip(depth, gray, R, tau, cut, fill, t0, n)
    return TR.to_u16_range(filt, TR.ranges(robust_minmax(depth, q), cut, R, t0, n))


def above(frame, hi):
    """valid pixels strictly above the white point, in the fixed point the percentile is taken in (a blend's float may exceed
    hi16 / 16 by less than 1/32 and still round into bin hi16)"""
    d16 = TR.d16_of(frame)
    return int(((d16 >= 1) & (d16 > TR.d16_of(np.float32(hi)))).sum())


def white_point_loops(frame, q):
    """the contract as a literal per-pixel loop (checks the vectorised form above on small frames)"""
    f = np.asarray(frame, np.float32)
    hist = [0] * NB
    mn = mx = None
    nan = False
    for v in f.reshape(-1):
        nan = nan or v != v
        mn = v if mn is None or v < mn or (v == mn and np.signbit(v)) else mn          # -0.0 sorts below +0.0
        mx = v if mx is None or v > mx or (v == mx and not np.signbit(v)) else mx
        d16 = TR.d16_loop(v)
        if d16 >= 1:
            hist[min(d16, NB - 1)] += 1
    if nan:
        return np.float32(np.nan), np.float32(np.nan)
    n_valid = sum(hist)
    if n_valid == 0:
        return np.float32(mn), np.float32(mx)
    k = max(1, (q * n_valid + 9999) // 10000)
    run = 0
    for b in range(NB):
        run += hist[b]
        if run >= k:
            break
    if b == NB - 1:
        return np.float32(mn), np.float32(mx)
    return np.float32(mn), max(np.float32(b) / np.float32(16), np.float32(mn))
