"""NumPy restatement of the disparity hole-filling contract (include/v3d_hip.h, v3d_fill.hip).  Test infrastructure: the GPU entry
is compared with these functions bit for bit.  All arithmetic is integer.

A frame is int16 [H,W]; a pixel is a hole iff d < 0 (0 is a valid disparity).
  1. rows: in a row with a non-hole pixel, a hole takes min(d[a], d[b]) of the nearest non-hole pixels a (left) and b (right) of the
     INPUT row, or the only one; non-hole pixels are copied;
  2. empty rows: a row without a non-hole pixel becomes a copy of the step-1 output of the nearest non-empty row by |r - y| (ties: the
     row above); a frame without a non-hole pixel is copied unchanged."""
import numpy as np

_NONE = np.int32(1 << 16)          # above every int16: "no neighbour on this side"


def fill_frame(d):
    d = np.asarray(d)
    if d.dtype != np.int16 or d.ndim != 2:
        raise ValueError(f"expected an int16 [H,W] frame, got {d.dtype} {d.shape}")
    H, W = d.shape
    valid = d >= 0
    x = np.arange(W)
    # index of the nearest valid pixel at or left of x (-1: none) and at or right of x (W: none)
    left = np.maximum.accumulate(np.where(valid, x, -1), axis=1)
    right = np.minimum.accumulate(np.where(valid, x, W)[:, ::-1], axis=1)[:, ::-1]
    wide = d.astype(np.int32)
    a = np.where(left >= 0, np.take_along_axis(wide, np.maximum(left, 0), axis=1), _NONE)
    b = np.where(right < W, np.take_along_axis(wide, np.minimum(right, W - 1), axis=1), _NONE)
    m = np.minimum(a, b)
    out = np.where(valid | (m == _NONE), wide, m).astype(np.int16)
    rows = np.flatnonzero(valid.any(axis=1))
    if rows.size and rows.size < H:
        y = np.arange(H)
        pos = np.searchsorted(rows, y)                              # rows[pos - 1] < y <= rows[pos]
        above = rows[np.maximum(pos - 1, 0)]
        below = rows[np.minimum(pos, rows.size - 1)]
        da = np.where(pos > 0, y - above, H + 1)
        db = np.where(pos < rows.size, below - y, H + 1)
        src = np.where(da <= db, above, below)                      # ties: the row above
        out = out[src]
    return out


def fill(disp):
    """int16 [n,H,W] (or one [H,W] frame) -> the filled disparity, frame by frame"""
    disp = np.asarray(disp)
    if disp.ndim == 2:
        return fill_frame(disp)
    return np.stack([fill_frame(f) for f in disp])


def fill_frame_loops(d):
    """the contract as a literal per-pixel loop (checks the vectorised form above on small frames)"""
    d = np.asarray(d, np.int16)
    H, W = d.shape
    out = d.copy()
    nonempty = []
    for y in range(H):
        has = False
        for x in range(W):
            if d[y, x] >= 0:
                has = True
                continue
            a = x - 1
            while a >= 0 and d[y, a] < 0:
                a -= 1
            b = x + 1
            while b < W and d[y, b] < 0:
                b += 1
            if a >= 0 and b < W:
                out[y, x] = min(int(d[y, a]), int(d[y, b]))
            elif a >= 0:
                out[y, x] = d[y, a]
            elif b < W:
                out[y, x] = d[y, b]
        nonempty.append(has)
    if not any(nonempty):
        return out
    step1 = out.copy()
    for y in range(H):
        if nonempty[y]:
            continue
        best = None
        for r in range(H):
            if nonempty[r] and (best is None or abs(r - y) < abs(best - y)):      # strict: the first (upper) row keeps a tie
                best = r
        out[y] = step1[best]
    return out
