"""NumPy restatement of the quality report's two measures (include/v3d_hip.h, v3d_quality.hip).  Test infrastructure: the GPU
entries and the host driver (video_3d_pipeline/quality.py) are compared with these functions bit for bit.  All arithmetic is
integer (int64 here; Python integers in the loop twins); the only float step is the temporal contract's d16 = rint(16 D).

Reprojection, per frame: left / right gray uint8 [H,W], disparity int16 [H,W] (x16; valid iff >= 1).  With u = 16 x - d a valid
pixel is compared iff u >= 0; i = u >> 4, f = u & 15, r16 = (16 - f) R[y][i] + f R[y][i+1], e = |16 L[y][x] - r16|,
e0 = 16 |L[y][x] - R[y][x]|.  Record: n_valid, n_cmp, sad, ssd, n_bad, sad0, ssd0, n_bad0 (REPROJ_FIELDS).

A hand-computed row, W = 4, bad_thr = 1:  L = [10, 20, 30, 40], R = [12, 24, 36, 48], d = [16, 8, -16, 40]
  x = 0: valid, u = -16: not compared.
  x = 1: valid, u = 8: i = 0, f = 8, r16 = 8*12 + 8*24 = 288, e = |320 - 288| = 32, e0 = 16*4 = 64.
  x = 2: invalid.
  x = 3: valid, u = 8: i = 0, f = 8, r16 = 288, e = |640 - 288| = 352, e0 = 16*8 = 128.
  record = (3, 2, 384, 32^2 + 352^2 = 124928, 2, 192, 64^2 + 128^2 = 20480, 2).

Flicker, per pair of consecutive frames u, u+1 of a clip (depth float32 [T,H,W], gray uint8 [T,H,W]): luma_sad = sum |dY| over all
pixels; over the pixels with |dY| <= still and both d16 >= 1: n_still, flicker = sum |d16_{u+1} - d16_u|, n_jump = #{> jump16}
(FLICKER_FIELDS)."""
import numpy as np

import temporal_ref as TR

REPROJ_FIELDS = ("n_valid", "n_cmp", "sad", "ssd", "n_bad", "sad0", "ssd0", "n_bad0")
FLICKER_FIELDS = ("luma_sad", "n_still", "flicker", "n_jump")
E_MAX = 4080                        # 16 * 255


def d16_of(depth):
    """the temporal contract's fixed point (tests/temporal_ref.py d16_of): rint(16 D) in float32, half to even; NaN, -inf and
    everything below 1 are invalid (0), +inf and everything above 32767 count as 32767; no non-finite value is converted"""
    return TR.d16_of(depth)


def reproj_frame(left, right, disp16, bad_thr=16):
    """one frame -> int64 [8]"""
    L, R, d = np.asarray(left).astype(np.int64), np.asarray(right).astype(np.int64), np.asarray(disp16).astype(np.int64)
    H, W = L.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    valid = d >= 1
    u = 16 * x - d
    cmp_ = valid & (u >= 0)
    us = np.where(cmp_, u, 0)
    i, f = us >> 4, us & 15
    i1 = np.minimum(i + 1, W - 1)                             # only differs where the pixel is not compared
    rows = np.arange(H)[:, None]
    r16 = (16 - f) * R[rows, i] + f * R[rows, i1]
    e = np.abs(16 * L - r16)[cmp_]
    e0 = (16 * np.abs(L - R))[cmp_]
    t = 16 * int(bad_thr)
    return np.array([valid.sum(), cmp_.sum(), e.sum(), (e * e).sum(), (e > t).sum(), e0.sum(), (e0 * e0).sum(), (e0 > t).sum()], np.int64)


def reproj(left, right, disp16, bad_thr=16):
    """[n,H,W] planes -> int64 [n,8]"""
    return np.stack([reproj_frame(l, r, d, bad_thr) for l, r, d in zip(left, right, disp16)])


def reproj_loops(left, right, disp16, bad_thr=16):
    """the contract as a literal per-pixel loop over Python integers (one frame)"""
    L, R, d = np.asarray(left).tolist(), np.asarray(right).tolist(), np.asarray(disp16).tolist()
    rec = [0] * 8
    for y in range(len(L)):
        for x in range(len(L[0])):
            dd = d[y][x]
            if dd < 1:
                continue
            rec[0] += 1
            u = 16 * x - dd
            if u < 0:
                continue
            i, f = u >> 4, u & 15
            e = abs(16 * L[y][x] - ((16 - f) * R[y][i] + f * R[y][i + 1]))
            e0 = 16 * abs(L[y][x] - R[y][x])
            rec[1] += 1
            rec[2] += e
            rec[3] += e * e
            rec[4] += e > 16 * bad_thr
            rec[5] += e0
            rec[6] += e0 * e0
            rec[7] += e0 > 16 * bad_thr
    return rec


def flicker(depth, gray, still, jump16):
    """a clip of T >= 2 frames -> int64 [T-1,4]"""
    d = d16_of(depth)
    g = np.asarray(gray).astype(np.int64)
    T = len(d)
    out = np.zeros((T - 1, 4), np.int64)
    for u in range(T - 1):
        dy = np.abs(g[u + 1] - g[u])
        s = (dy <= int(still)) & (d[u] >= 1) & (d[u + 1] >= 1)
        dd = np.abs(d[u + 1] - d[u])[s]
        out[u] = dy.sum(), s.sum(), dd.sum(), (dd > int(jump16)).sum()
    return out


def flicker_loops(depth, gray, still, jump16):
    """the contract as a literal per-pixel loop over Python integers"""
    depth = np.asarray(depth, np.float32)
    T, H, W = depth.shape
    Y = np.asarray(gray).astype(int).tolist()

    d16 = TR.d16_loop
    out = []
    for u in range(T - 1):
        rec = [0] * 4
        for y in range(H):
            for x in range(W):
                dy = abs(Y[u + 1][y][x] - Y[u][y][x])
                a, b = d16(depth[u, y, x]), d16(depth[u + 1, y, x])
                rec[0] += dy
                if dy <= still and a >= 1 and b >= 1:
                    rec[1] += 1
                    rec[2] += abs(b - a)
                    rec[3] += abs(b - a) > jump16
        out.append(rec)
    return out
