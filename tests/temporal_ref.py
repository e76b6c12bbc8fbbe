"""NumPy restatement of the temporal depth stabilisation contract (include/v3d_hip.h; the device side is v3d_temporal.hip with
the closed forms of v3d_temporal_math.h).  Test infrastructure:
the GPU entries and the streaming driver are compared with these functions bit for bit.  All arithmetic is integer (int64
here; the device proves int32 enough) except the final range normalisation, which repeats v3d_depth_to_u16's float32 steps.

A clip is depth float32 [T,H,W] (<= 0 invalid) and left gray uint8 [T,H,W]; radius R in 0..8, tau in 1..255, cut threshold c in
0..256, fill 0/1."""
import numpy as np

MAX_RADIUS = 8
S_MAX = 9 * 255                     # largest 3x3 sum of absolute luma differences


D16_MAX = 32767                     # a valid tap above the range, +inf included, counts as this (v3d_depth_math.h's v3d_d16_tap)


def d16_of(depth):
    """step 1: fixed point x16, round half to even -> int64, 0 = invalid, else 1 .. D16_MAX.  Validity is decided on the float,
    before any conversion: valid iff 1 <= rint(16 D), which NaN, -inf, -0.0 and every D < 1/32 fail; a valid value above D16_MAX
    saturates.  Only values an integer holds are ever converted (an astype of a NaN or an infinity is a platform accident)."""
    with np.errstate(over="ignore", invalid="ignore"):    # 16 * FLT_MAX is +inf: saturates like every tap above the range; a signalling NaN
        r = np.rint(np.asarray(depth, np.float32) * np.float32(16))
    ok = r >= 1                                           # False for NaN
    return np.where(ok, np.minimum(np.where(ok, r, 0), D16_MAX), 0).astype(np.int64)


def cuts(gray, c):
    """step 2: cut[u] = 1 iff sum |Y_u - Y_{u-1}| > c * W * H (u >= 1); cut[0] = 0"""
    g = np.asarray(gray).astype(np.int64)
    T = g.shape[0]
    out = np.zeros(T, np.uint8)
    if T > 1:
        sad = np.abs(g[1:] - g[:-1]).reshape(T - 1, -1).sum(axis=1)
        out[1:] = sad > int(c) * g.shape[1] * g.shape[2]
    return out


def admissible(cut, T, t, R):
    """(first, last) frame that may contribute to target t: |u - t| <= R, 0 <= u < T, no cut in (min(t,u), max(t,u)]"""
    lo = t
    while lo - 1 >= max(0, t - R) and not cut[lo]:
        lo -= 1
    hi = t
    while hi + 1 <= min(T - 1, t + R) and not cut[hi + 1]:
        hi += 1
    return lo, hi


def rw_magic(tau):
    """floor(256 s / (9 tau)) for s in 0..2295 as (256 s * mul) >> 32, mul = ceil(2^32 / (9 tau)) (the kernel's form)"""
    d = 9 * int(tau)
    return ((1 << 32) + d - 1) // d


def range_weight(s, tau):
    """step 3: rw = max(0, 256 - floor(256 s / (9 tau)))"""
    return np.maximum(0, 256 - (256 * np.asarray(s, np.int64)) // (9 * int(tau)))


def box3(a):
    """3x3 sum, edge-replicated; a int64 [H,W]"""
    p = np.pad(a, 1, mode="edge")
    H, W = a.shape
    return sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))


def filter_clip(depth, gray, R, tau=12, cut=None, fill=1, t0=0, n=None):
    """steps 1, 3, 4 for targets t0 .. t0+n-1 of a T-frame buffer -> float32 [n,H,W] (multiples of 1/16)"""
    depth = np.asarray(depth, np.float32)
    T = depth.shape[0]
    n = T - t0 if n is None else n
    cut = np.zeros(T, np.uint8) if cut is None else np.asarray(cut)
    d16 = d16_of(depth)
    g = np.asarray(gray).astype(np.int64)
    out = np.zeros((n,) + depth.shape[1:], np.float32)
    for j in range(n):
        t = t0 + j
        lo, hi = admissible(cut, T, t, R)
        Wsum = np.zeros(depth.shape[1:], np.int64)
        Dsum = np.zeros(depth.shape[1:], np.int64)
        for u in range(lo, hi + 1):
            s = box3(np.abs(g[u] - g[t]))
            w = (R + 1 - abs(u - t)) * range_weight(s, tau) * (d16[u] >= 1)
            Wsum += w
            Dsum += w * d16[u]
        o = np.where(Wsum > 0, (2 * Dsum + Wsum) // np.maximum(2 * Wsum, 1), 0)
        if not fill:
            o = np.where(d16[t] >= 1, o, 0)
        out[j] = o.astype(np.float32) / np.float32(16)
    return out


def minmax(depth):
    """per-frame min and max of the unfiltered depth, float32 [T,2]; a frame that holds a NaN gives (NaN, NaN) (ndarray.min / .max
    propagate), -0.0 sorts below +0.0 on the device and compares equal here, +-inf are ordinary extrema"""
    d = np.ascontiguousarray(depth, np.float32).reshape(len(depth), -1)
    u = d.view(np.uint32)
    o = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))                # the device's order-preserving code: -0.0 below +0.0
    o = np.stack([o.min(axis=1), o.max(axis=1)], axis=1)
    out = np.where(o >> 31 == 1, o & np.uint32(0x7FFFFFFF), ~o).astype(np.uint32).view(np.float32)
    out[np.isnan(d).any(axis=1)] = np.nan
    return out


def ranges(mm, cut, R, t0=0, n=None):
    """step 5: lo_t = min mn_u, hi_t = max mx_u over the admissible u -> float32 [n,2]; a NaN bound in any admissible frame, at
    any position of the window, makes both bounds of the target NaN (and to_u16_range then writes a frame of 0)"""
    T = len(mm)
    n = T - t0 if n is None else n
    out = np.zeros((n, 2), np.float32)
    for j in range(n):
        lo, hi = admissible(cut, T, t0 + j, R)
        win = np.asarray(mm[lo:hi + 1], np.float32)
        out[j] = (np.nan, np.nan) if np.isnan(win).any() else (win[:, 0].min(), win[:, 1].max())
    return out


def to_u16_range(depth, lohi):
    """v3d_depth_to_u16's float32 expression with (lo, hi) given per frame; hi == lo -> 0; clamped to [0, 65535] in float32.
    A range that is unordered or holds a NaN gives a frame of 0; so does an infinite bound (every quotient is 0, NaN or negative);
    a NaN sample gives 0 (the device's clamp `v >= 65535 ? 65535 : v > 0 ? v : 0` lets no NaN through, and none is converted here)"""
    depth = np.asarray(depth, np.float32)
    out = np.zeros(depth.shape, np.uint16)
    for f in range(len(depth)):
        mn, mx = np.float32(lohi[f][0]), np.float32(lohi[f][1])
        if mx > mn:
            with np.errstate(over="ignore", invalid="ignore"):          # inf - inf, inf / inf, FLT_MAX * 65535: all defined below
                v = (depth[f] - mn) / np.float32(mx - mn) * np.float32(65535.0)
            v = np.where(v >= np.float32(65535), np.float32(65535), np.where(v > 0, v, np.float32(0)))
            out[f] = v.astype(np.uint16)
    return out


def stabilize(depth, gray, R, tau=12, c=20, fill=1, t0=0, n=None):
    """the whole stage on a buffer of T frames: cuts, filter, clip-stable range -> uint16 [n,H,W]"""
    cut = cuts(gray, c)
    filt = filter_clip(depth, gray, R, tau, cut, fill, t0, n)
    return to_u16_range(filt, ranges(minmax(depth), cut, R, t0, n))


def d16_loop(v):
    """d16_of for one sample, as branches on the float: nothing that is not a finite value in range reaches int()"""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.float32(v) * np.float32(16))
    if not r >= 1:                                        # NaN, -inf, zeros, negatives
        return 0
    return D16_MAX if r >= D16_MAX else int(r)


def filter_loops(depth, gray, R, tau, cut, fill):
    """the contract as a literal per-pixel, per-tap loop (checks the vectorised form above on small clips)"""
    T, H, W = depth.shape
    out = np.zeros((T, H, W), np.float32)
    d16 = [[[d16_loop(depth[t, y, x]) for x in range(W)] for y in range(H)] for t in range(T)]
    Y = np.asarray(gray).astype(int).tolist()
    for t in range(T):
        for y in range(H):
            for x in range(W):
                Wsum = Dsum = 0
                for k in range(-R, R + 1):
                    u = t + k
                    if u < 0 or u >= T or any(cut[v] for v in range(min(t, u) + 1, max(t, u) + 1)):
                        continue
                    s = 0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            yy, xx = min(max(y + dy, 0), H - 1), min(max(x + dx, 0), W - 1)
                            s += abs(Y[u][yy][xx] - Y[t][yy][xx])
                    w = (R + 1 - abs(k)) * max(0, 256 - (256 * s) // (9 * tau)) * (1 if d16[u][y][x] >= 1 else 0)
                    Wsum += w
                    Dsum += w * d16[u][y][x]
                o = (2 * Dsum + Wsum) // (2 * Wsum) if Wsum > 0 else 0
                if not fill and d16[t][y][x] < 1:
                    o = 0
                out[t, y, x] = np.float32(o) / np.float32(16)
    return out
