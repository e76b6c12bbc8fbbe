"""NumPy restatement of the motion-compensated temporal stabilisation contract (include/v3d_hip.h; the block search is
v3d_temporal_mc.hip, the filter v3d_temporal.hip's one kernel; `--temporal-motion S`).  Test infrastructure: the GPU entries and the streaming driver are compared with these functions bit for
bit.  All arithmetic is integer.  Everything the motion leaves alone (d16, the admissible window, the range weight, the
clip-stable range, the normalisation) is tests/temporal_ref.py's.

Blocks are 16x16 luma pixels on a grid anchored at (0,0), edge blocks clipped to the frame.  A field holds one vector (dx, dy)
per block: F_u points from frame u into frame u+1, Bk_u from frame u into frame u-1; F_{T-1} = Bk_0 = 0."""
import numpy as np

import temporal_ref as TR

BLOCK = 16
MAX_SEARCH = 32
KEY_SHIFT = 8192                     # key = cost * 8192 + rank; rank <= (2*32+1)^2 - 1 = 4224
MAX_COST = 255 * 256 + 64 * 64       # a block's SAD plus the largest penalty: 64 px * (32 + 32)


def blocks(W, H):
    return -(-W // BLOCK), -(-H // BLOCK)


def _block_sums(a):
    """int64 [H,W] -> sums over the clipped 16x16 blocks [BH,BW]"""
    H, W = a.shape
    BW, BH = blocks(W, H)
    p = np.zeros((BH * BLOCK, BW * BLOCK), np.int64)
    p[:H, :W] = a
    return p.reshape(BH, BLOCK, BW, BLOCK).sum(axis=(1, 3))


def penalty(W, H):
    """max(n_b >> 2, 1) per block, n_b the block's pixel count [BH,BW]"""
    return np.maximum(_block_sums(np.ones((H, W), np.int64)) >> 2, 1)


def search(Yu, Yv, S):
    """one field from frame Yu into frame Yv -> (vectors int16 [BH,BW,2] as (dx,dy), the chosen candidates' unpenalised SAD
    int64 [BH,BW])"""
    Yu, Yv = np.asarray(Yu).astype(np.int64), np.asarray(Yv).astype(np.int64)
    H, W = Yu.shape
    pen = penalty(W, H)
    pad = np.pad(Yv, S, mode="edge")                         # Yv(clamp(x + dx), clamp(y + dy)) = pad[y + dy + S, x + dx + S]
    best_key = best_sad = None
    n = 2 * S + 1
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            sad = _block_sums(np.abs(Yu - pad[dy + S:dy + S + H, dx + S:dx + S + W]))
            key = (sad + pen * (abs(dx) + abs(dy))) * KEY_SHIFT + (dy + S) * n + (dx + S)
            if best_key is None:
                best_key, best_sad = key, sad
            else:
                take = key < best_key
                best_key, best_sad = np.where(take, key, best_key), np.where(take, sad, best_sad)
    rank = best_key % KEY_SHIFT
    mv = np.stack([rank % n - S, rank // n - S], axis=-1).astype(np.int16)
    return mv, best_sad


def fields(gray, S):
    """forward and backward fields of a buffer -> (F int16 [T,BH,BW,2], Bk int16 [T,BH,BW,2], resid uint64 [T])"""
    g = np.asarray(gray)
    T, H, W = g.shape
    BW, BH = blocks(W, H)
    F, Bk = np.zeros((T, BH, BW, 2), np.int16), np.zeros((T, BH, BW, 2), np.int16)
    resid = np.zeros(T, np.uint64)
    for u in range(T - 1):
        F[u], _ = search(g[u], g[u + 1], S)
        Bk[u + 1], sad = search(g[u + 1], g[u], S)
        resid[u + 1] = int(sad.sum())
    return F, Bk, resid


def cuts(resid, c, W, H):
    """cut[u] = resid[u] > c * W * H (resid[0] = 0)"""
    return (np.asarray(resid).astype(np.int64) > int(c) * W * H).astype(np.uint8)


def chain(F, Bk, t, u, W, H):
    """the chained vector of every block from target t to frame u -> int64 [BH,BW,2]"""
    BW, BH = blocks(W, H)
    cx = np.minimum(BLOCK * np.arange(BW) + 8, W - 1)[None, :].repeat(BH, 0)
    cy = np.minimum(BLOCK * np.arange(BH) + 8, H - 1)[:, None].repeat(BW, 1)
    m = np.zeros((BH, BW, 2), np.int64)
    step = 1 if u > t else -1
    for f in range(t, u, step):
        fld = (F if step > 0 else Bk)[f].astype(np.int64)
        px, py = np.clip(cx + m[..., 0], 0, W - 1), np.clip(cy + m[..., 1], 0, H - 1)
        m = m + fld[py // BLOCK, px // BLOCK]
    return m


def filter_clip(depth, gray, R, tau, cut, F, Bk, fill=1, t0=0, n=None):
    """steps 1, 3, 4 with frame u read at q = p + m for targets t0 .. t0+n-1 -> float32 [n,H,W] (multiples of 1/16)"""
    depth = np.asarray(depth, np.float32)
    T, H, W = depth.shape
    n = T - t0 if n is None else n
    d16 = TR.d16_of(depth)
    g = np.asarray(gray).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.float32)
    for j in range(n):
        t = t0 + j
        lo, hi = TR.admissible(cut, T, t, R)
        Wsum, Dsum = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
        for u in range(lo, hi + 1):
            m = chain(F, Bk, t, u, W, H)
            mx = np.repeat(np.repeat(m[..., 0], BLOCK, 0), BLOCK, 1)[:H, :W]
            my = np.repeat(np.repeat(m[..., 1], BLOCK, 0), BLOCK, 1)[:H, :W]
            qx, qy = xx + mx, yy + my
            s = np.zeros((H, W), np.int64)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    a = g[u][np.clip(qy + dy, 0, H - 1), np.clip(qx + dx, 0, W - 1)]
                    b = g[t][np.clip(yy + dy, 0, H - 1), np.clip(xx + dx, 0, W - 1)]
                    s += np.abs(a - b)
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            tap = d16[u][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
            w = (R + 1 - abs(u - t)) * TR.range_weight(s, tau) * (tap >= 1) * inside
            Wsum += w
            Dsum += w * tap
        o = np.where(Wsum > 0, (2 * Dsum + Wsum) // np.maximum(2 * Wsum, 1), 0)
        if not fill:
            o = np.where(d16[t] >= 1, o, 0)
        out[j] = o.astype(np.float32) / np.float32(16)
    return out


def stabilize(depth, gray, R, S, tau=12, c=20, fill=1, t0=0, n=None):
    """the whole stage with motion on a buffer of T frames: fields, compensated cuts, filter, clip-stable range -> uint16 [n,H,W]"""
    g = np.asarray(gray)
    F, Bk, resid = fields(g, S)
    cut = cuts(resid, c, g.shape[2], g.shape[1])
    filt = filter_clip(depth, g, R, tau, cut, F, Bk, fill, t0, n)
    return TR.to_u16_range(filt, TR.ranges(TR.minmax(depth), cut, R, t0, n))


# ---- the contract as literal loops (checks the vectorised forms above on small clips) ----

def search_loops(Yu, Yv, S):
    Yu, Yv = np.asarray(Yu).astype(int).tolist(), np.asarray(Yv).astype(int).tolist()
    H, W = len(Yu), len(Yu[0])
    BW, BH = blocks(W, H)
    mv, sads = np.zeros((BH, BW, 2), np.int16), np.zeros((BH, BW), np.int64)
    for by in range(BH):
        for bx in range(BW):
            xs, ys = range(16 * bx, min(16 * bx + 16, W)), range(16 * by, min(16 * by + 16, H))
            pen = max((len(xs) * len(ys)) >> 2, 1)
            best = None
            for dy in range(-S, S + 1):
                for dx in range(-S, S + 1):
                    sad = 0
                    for y in ys:
                        row_u, row_v = Yu[y], Yv[min(max(y + dy, 0), H - 1)]
                        for x in xs:
                            sad += abs(row_u[x] - row_v[min(max(x + dx, 0), W - 1)])
                    cost = sad + pen * (abs(dx) + abs(dy))
                    assert cost <= MAX_COST
                    key = cost * KEY_SHIFT + (dy + S) * (2 * S + 1) + (dx + S)
                    if best is None or key < best[0]:
                        best = (key, dx, dy, sad)
            mv[by, bx] = best[1], best[2]
            sads[by, bx] = best[3]
    return mv, sads


def filter_loops(depth, gray, R, tau, cut, F, Bk, fill):
    T, H, W = depth.shape
    BW, BH = blocks(W, H)
    out = np.zeros((T, H, W), np.float32)
    d16 = [[[TR.d16_loop(depth[t, y, x]) for x in range(W)] for y in range(H)] for t in range(T)]
    Y = np.asarray(gray).astype(int).tolist()
    clx, cly = (lambda v: min(max(v, 0), W - 1)), (lambda v: min(max(v, 0), H - 1))
    for t in range(T):
        for y in range(H):
            for x in range(W):
                bx, by = x // 16, y // 16
                cbx, cby = min(16 * bx + 8, W - 1), min(16 * by + 8, H - 1)
                Wsum = Dsum = 0
                for k in range(-R, R + 1):
                    u = t + k
                    if u < 0 or u >= T or any(cut[v] for v in range(min(t, u) + 1, max(t, u) + 1)):
                        continue
                    mx = my = 0
                    for j in range(abs(k)):
                        fld = F[t + j] if k > 0 else Bk[t - j]
                        vx, vy = fld[cly(cby + my) // 16][clx(cbx + mx) // 16]
                        mx, my = mx + int(vx), my + int(vy)
                    assert abs(mx) <= R * MAX_SEARCH and abs(my) <= R * MAX_SEARCH
                    qx, qy = x + mx, y + my
                    if not (0 <= qx < W and 0 <= qy < H):
                        continue
                    s = 0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            s += abs(Y[u][cly(qy + dy)][clx(qx + dx)] - Y[t][cly(y + dy)][clx(x + dx)])
                    w = (R + 1 - abs(k)) * max(0, 256 - (256 * s) // (9 * tau)) * (1 if d16[u][qy][qx] >= 1 else 0)
                    Wsum += w
                    Dsum += w * d16[u][qy][qx]
                o = (2 * Dsum + Wsum) // (2 * Wsum) if Wsum > 0 else 0
                if not fill and d16[t][y][x] < 1:
                    o = 0
                out[t, y, x] = np.float32(o) / np.float32(16)
    return out
