"""NumPy restatement of the matcher's post stage at the level of its input, the WTA records (test helper).

The domain of a record plane, uint32 [H][W] (wta_word in csrc/v3d_sgbm_internal.h, written by wta_pixel in csrc/v3d_sgbm_paths.hip):
  columns [64, W)  one record per cost-region pixel, in RELATIVE columns (x1 + 64): 0 for a rejected pixel, otherwise
                   minS << 17 | (d16 + 16) << 6 | best with minS in [0, 32766], best in [0, 63], d16 = 16 best + subpix,
                   subpix in [-8, 8] and 0 at best = 0 and best = 63 (so d16 in [0, 1008] and d16 + 16 is never 0)
  columns [0, 64)  never written: whatever the allocation held; no reader may let them move its output
The L-R check (stereosgbm.cpp, lr_check in csrc/v3d_sgbm_post.hip): the right-view key of target column c is the minimum of
minS << 6 | 63 - best over the records of the columns x with x - best == c (the cheapest source; among equally cheap ones the
largest d), 0xFFFFFFFF without a source.  A valid d16 at column x is invalidated when BOTH roundings da = d16 >> 4 and
db = (d16 + 15) >> 4 find a key, at x - da and x - db, whose d differs from the rounding by more than d12.
Placement for minDisparity m in [-64, 0]: out[y][x + m] = rel16 + 16 m for x in [64, W), the invalid value 16 (m - 1) at rejected
pixels and in every other column; then the 3x3 median with replicated borders."""
import numpy as np

import np_sgm

D = 64
NONE = np.uint32(0xFFFFFFFF)


def word(minS, d16, best):
    return (np.asarray(minS, np.uint32) << np.uint32(17)) | ((np.asarray(d16, np.uint32) + np.uint32(16)) << np.uint32(6)) | np.asarray(best, np.uint32)


def fields(rec):
    """-> (valid, minS, d16, best) of a record plane"""
    rec = np.asarray(rec, np.uint32)
    return (rec & np.uint32(0x1FFC0)) != 0, (rec >> np.uint32(17)).astype(np.int64), ((rec >> np.uint32(6)) & np.uint32(0x7FF)).astype(np.int64) - 16, (rec & np.uint32(63)).astype(np.int64)


def in_domain(rec):
    valid, minS, d16, best = (a[:, D:] for a in fields(rec))
    sub = d16 - 16 * best
    ok = (minS <= 32766) & (np.abs(sub) <= 8) & ((sub == 0) | ((best > 0) & (best < D - 1)))
    return bool(np.all(ok | ~valid) and np.all(np.asarray(rec)[:, D:][~valid] == 0))


def records(S, W, uniq=10):
    """aggregated costs [H][W - 64][64] (np_sgm.aggregate) -> the record plane [H][W]; columns [0, 64) hold 0"""
    S = np.asarray(S, np.int64)
    H, W1, _ = S.shape
    assert W1 == W - D
    rec = np.zeros((H, W), np.uint32)
    ds = np.arange(D)
    for y in range(H):
        for x in range(W1):
            s = S[y, x]
            best = int(np.argmin(s))
            ms = int(s[best])
            if ms >= np_sgm.MAXC or np.any((s * (100 - uniq) < ms * 100) & (np.abs(ds - best) > 1)):
                continue
            sub = 0
            if 0 < best < D - 1:
                den = max(int(s[best - 1] + s[best + 1] - 2 * ms), 1)
                num = int(s[best - 1] - s[best + 1]) * 16 + den
                sub = abs(num) // (2 * den) * (1 if num >= 0 else -1)
            rec[y, x + D] = word(ms, 16 * best + sub, best)
    return rec


def keys(rec):
    """the right-view key map [H][W], vectorised"""
    H, W = rec.shape
    valid, minS, _, best = fields(rec)
    valid[:, :D] = False
    ys, xs = np.nonzero(valid)
    out = np.full((H, W), NONE, np.uint32)
    np.minimum.at(out, (ys, xs - best[ys, xs]), ((minS[ys, xs] << 6) | (63 - best[ys, xs])).astype(np.uint32))
    return out


def keys_loop(rec):
    """the same, pixel by pixel: every target column looks at its 64 possible sources"""
    H, W = rec.shape
    out = np.full((H, W), NONE, np.uint32)
    for y in range(H):
        for c in range(W):
            for d in range(D):
                x = c + d
                if x < D or x >= W:
                    continue
                r = int(rec[y, x])
                if (r & 0x1FFC0) and (r & 63) == d:
                    out[y, c] = min(int(out[y, c]), ((r >> 17) << 6) | (63 - d))
    return out


def lrcheck_rel(rec, d12=1, key_map=None):
    """-> relative disparities int32 [H][W], -16 invalid (columns [0, 64) invalid)"""
    H, W = rec.shape
    valid, _, d16, _ = fields(rec)
    valid[:, :D] = False
    k = keys(rec) if key_map is None else key_map
    xs = np.broadcast_to(np.arange(W), (H, W))
    ys = np.broadcast_to(np.arange(H)[:, None], (H, W))
    d1 = np.where(valid, d16, 0)
    da, db = d1 >> 4, (d1 + 15) >> 4
    ka, kb = k[ys, np.where(valid, xs - da, 0)], k[ys, np.where(valid, xs - db, 0)]
    bad = ((ka != NONE) & (np.abs(63 - (ka & np.uint32(63)).astype(np.int64) - da) > d12) &
           (kb != NONE) & (np.abs(63 - (kb & np.uint32(63)).astype(np.int64) - db) > d12))
    return np.where(valid & ~bad, d16, -16).astype(np.int32)


def place(rel, m):
    H, W = rel.shape
    out = np.full((H, W), 16 * (m - 1), np.int32)
    out[:, D + m:W + m] = rel[:, D:] + 16 * m
    return out.astype(np.int16)


def lrcheck(rec, d12=1, m=0):
    """record plane -> the int16 plane before the median (the debug_raw export)"""
    assert -D <= m <= 0
    return place(lrcheck_rel(rec, d12), m)


def lrcheck_median(rec, d12=1, m=0):
    from scipy.ndimage import median_filter
    return median_filter(lrcheck(rec, d12, m), size=3, mode="nearest")


def random_records(rng, W, H, reject=0.15, few_costs=False, best63_at_64=False, subpix_extremes=False, empty_rows=(), noise=0.2):
    """a record plane inside the domain: disparities piecewise constant along a row with a share `noise` of outliers (so that the
    check both passes and rejects), a share `reject` of rejected pixels.  few_costs: minS from four values only (ties in the key
    map's cost part: the larger d must win); best63_at_64: column 64 holds best = 63 (target column 1, the leftmost any source
    reaches); subpix_extremes: every inner pixel carries -8 or +8; empty_rows: rows without any record.  Columns [0, 64) hold 0"""
    seg = rng.integers(0, D, (H, W // 16 + 2))
    best = np.repeat(seg, 16, axis=1)[:, :W] + rng.integers(-1, 2, (H, W))
    out = rng.random((H, W)) < noise
    best = np.clip(np.where(out, rng.integers(0, D, (H, W)), best), 0, D - 1)
    if best63_at_64:
        best[:, D] = 63
    minS = rng.integers(0, 4, (H, W)) * 8191 if few_costs else rng.integers(0, 32767, (H, W))
    minS = np.minimum(minS, 32766)
    sub = rng.choice([-8, 8], (H, W)) if subpix_extremes else rng.integers(-8, 9, (H, W))
    sub = np.where((best > 0) & (best < D - 1), sub, 0)
    rec = word(minS, 16 * best + sub, best)
    gone = rng.random((H, W)) < reject
    if best63_at_64:
        gone[:, D] = False
    rec[gone] = 0
    rec[list(empty_rows)] = 0
    rec[:, :D] = 0
    return rec.astype(np.uint32)
