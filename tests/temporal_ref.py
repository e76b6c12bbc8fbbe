"""NumPy restatement of the temporal depth stabilisation contract (include/v3d_hip.h; the device side is v3d_temporal.hip with
the closed forms of v3d_temporal_math.h).  Test infrastructure:
the GPU entries and the streaming driver are compared with these functions bit for bit.  All arithmetic is integer (int64
here; the device proves int32 enough) except the final range normalisation, which repeats v3d_depth_to_u16's float32 steps.

A clip is depth float32 [T,H,W] (<= 0 invalid) and left gray uint8 [T,H,W]; radius R in 0..8, tau in 1..255, cut threshold c in
0..256, fill 0/1."""
import numpy as np

MAX_RADIUS = 8
S_MAX = 9 * 255                     # largest 3x3 sum of absolute luma differences


def d16_of(depth):
    """step 1: fixed point x16, round half to even"""
    return np.rint(np.asarray(depth, np.float32) * np.float32(16)).astype(np.int64)


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
    """per-frame min and max of the unfiltered depth, float32 [T,2]"""
    d = np.asarray(depth, np.float32).reshape(len(depth), -1)
    return np.stack([d.min(axis=1), d.max(axis=1)], axis=1).astype(np.float32)


def ranges(mm, cut, R, t0=0, n=None):
    """step 5: lo_t = min mn_u, hi_t = max mx_u over the admissible u -> float32 [n,2]"""
    T = len(mm)
    n = T - t0 if n is None else n
    out = np.zeros((n, 2), np.float32)
    for j in range(n):
        lo, hi = admissible(cut, T, t0 + j, R)
        out[j] = mm[lo:hi + 1, 0].min(), mm[lo:hi + 1, 1].max()
    return out


def to_u16_range(depth, lohi):
    """v3d_depth_to_u16's float32 expression with (lo, hi) given per frame; hi == lo -> 0; clamped to [0, 65535] in float32"""
    depth = np.asarray(depth, np.float32)
    out = np.zeros(depth.shape, np.uint16)
    for f in range(len(depth)):
        mn, mx = np.float32(lohi[f][0]), np.float32(lohi[f][1])
        if mx > mn:
            v = (depth[f] - mn) / np.float32(mx - mn) * np.float32(65535.0)
            out[f] = np.clip(v, np.float32(0), np.float32(65535)).astype(np.uint16)
    return out


def stabilize(depth, gray, R, tau=12, c=20, fill=1, t0=0, n=None):
    """the whole stage on a buffer of T frames: cuts, filter, clip-stable range -> uint16 [n,H,W]"""
    cut = cuts(gray, c)
    filt = filter_clip(depth, gray, R, tau, cut, fill, t0, n)
    return to_u16_range(filt, ranges(minmax(depth), cut, R, t0, n))


def filter_loops(depth, gray, R, tau, cut, fill):
    """the contract as a literal per-pixel, per-tap loop (checks the vectorised form above on small clips)"""
    T, H, W = depth.shape
    out = np.zeros((T, H, W), np.float32)
    d16 = [[[int(np.rint(np.float32(depth[t, y, x]) * np.float32(16))) for x in range(W)] for y in range(H)] for t in range(T)]
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
