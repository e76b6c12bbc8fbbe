"""NumPy restatement of the colour-matching contract of include/v3d_hip.h (v3d_bgr_hist_batch, v3d_colour_lut_batch,
v3d_bgr_lut_batch; csrc/v3d_colour.hip).  Every number is an integer and the device must agree bit for bit.  Each function has a
vectorised form and a literal twin that walks the pixels / the levels one by one (`*_loop`), which tests/test_colour_ref.py holds
against each other.

    hist[f][c][v]  = #{pixels of frame f in [x0, x1) x [y0, y1) whose byte c equals v}
    table j        : the frames [j group, min(n, (j + 1) group)) of both histogram sets, summed per bin; per channel, with Cs, Cf the
                     inclusive prefix sums and Ns = Cs[255], Nf = Cf[255]:
                       lut[v] = the smallest u with Cf[u] Ns >= Cs[v] Nf;   the identity if Ns == 0 or Nf == 0
                     Python integers: totals reach 2^48 and the products 2^96.  Cs does not decrease, so neither does lut.
    apply          : dst = lut[f][c][src] inside the rectangle, src outside it
"""
import numpy as np

# the grading of the quality experiment ("Colour matching"): per BGR channel s' = clip(floor(255 (s/255)^g k + o + 1/2))
GRADE_GAMMA, GRADE_GAIN, GRADE_OFFSET = (1.25, 0.9, 0.8), (0.85, 1.0, 1.12), (-6, 10, 14)


def _rect(rect, W, H):
    x0, y0, x1, y1 = (0, 0, W, H) if rect is None else (int(v) for v in rect)
    if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f"rectangle {rect} is empty or leaves the {W} x {H} image")
    return x0, y0, x1, y1


def hist(frames, rect=None):
    """u8 [n,H,W,3] -> uint32 [n,3,256]"""
    frames = np.asarray(frames, np.uint8)
    n, H, W, _ = frames.shape
    x0, y0, x1, y1 = _rect(rect, W, H)
    out = np.zeros((n, 3, 256), np.uint32)
    for f in range(n):
        for c in range(3):
            out[f, c] = np.bincount(frames[f, y0:y1, x0:x1, c].reshape(-1), minlength=256)
    return out


def hist_loop(frames, rect=None):
    frames = np.asarray(frames, np.uint8)
    n, H, W, _ = frames.shape
    x0, y0, x1, y1 = _rect(rect, W, H)
    out = np.zeros((n, 3, 256), np.uint32)
    for f in range(n):
        for y in range(y0, y1):
            for x in range(x0, x1):
                for c in range(3):
                    out[f, c, int(frames[f, y, x, c])] += 1
    return out


def _groups(n, group):
    if not 1 <= group <= n:
        raise ValueError(f"group {group} outside [1, {n}]")
    return [(j, min(n, j + group)) for j in range(0, n, group)]


def lut(hist_src, hist_dst, group=1):
    """two integer [n,3,256] histogram sets (counts up to 2^32 - 1) -> u8 [ceil(n / group),3,256]"""
    hs, hd = np.asarray(hist_src), np.asarray(hist_dst)
    assert hs.shape == hd.shape and hs.shape[1:] == (3, 256)
    spans = _groups(hs.shape[0], int(group))
    out = np.zeros((len(spans), 3, 256), np.uint8)
    for j, (a, b) in enumerate(spans):
        for c in range(3):
            Cs = np.cumsum(hs[a:b, c].astype(object).sum(axis=0))          # Python integers
            Cf = np.cumsum(hd[a:b, c].astype(object).sum(axis=0))
            Ns, Nf = Cs[255], Cf[255]
            if Ns == 0 or Nf == 0:
                out[j, c] = np.arange(256)
                continue
            reach = ((Cf * Ns)[None, :] >= (Cs * Nf)[:, None]).astype(bool)     # [v][u]
            out[j, c] = reach.argmax(axis=1)
    return out


def lut_loop(hist_src, hist_dst, group=1):
    hs, hd = np.asarray(hist_src), np.asarray(hist_dst)
    spans = _groups(hs.shape[0], int(group))
    out = np.zeros((len(spans), 3, 256), np.uint8)
    for j, (a, b) in enumerate(spans):
        for c in range(3):
            s = [sum(int(hs[f, c, v]) for f in range(a, b)) for v in range(256)]
            d = [sum(int(hd[f, c, v]) for f in range(a, b)) for v in range(256)]
            Cs, Cf, rs, rd = [], [], 0, 0
            for v in range(256):
                rs += s[v]
                rd += d[v]
                Cs.append(rs)
                Cf.append(rd)
            Ns, Nf = Cs[255], Cf[255]
            for v in range(256):
                if Ns == 0 or Nf == 0:
                    out[j, c, v] = v
                    continue
                u = 0
                while Cf[u] * Ns < Cs[v] * Nf:
                    u += 1
                out[j, c, v] = u
    return out


def _tables(table, n):
    t = np.asarray(table, np.uint8)
    if t.ndim == 2:
        t = t[None]
    assert t.shape[1:] == (3, 256) and t.shape[0] in (1, n)
    return np.broadcast_to(t, (n, 3, 256))


def apply(frames, table, rect=None):
    """u8 [n,H,W,3], table u8 [3,256] / [1,3,256] (shared) or [n,3,256] -> a copy with the rectangle mapped"""
    frames = np.asarray(frames, np.uint8)
    n, H, W, _ = frames.shape
    x0, y0, x1, y1 = _rect(rect, W, H)
    t = _tables(table, n)
    out = frames.copy()
    for f in range(n):
        for c in range(3):
            out[f, y0:y1, x0:x1, c] = t[f, c][frames[f, y0:y1, x0:x1, c]]
    return out


def apply_loop(frames, table, rect=None):
    frames = np.asarray(frames, np.uint8)
    n, H, W, _ = frames.shape
    x0, y0, x1, y1 = _rect(rect, W, H)
    t = _tables(table, n)
    out = frames.copy()
    for f in range(n):
        for y in range(y0, y1):
            for x in range(x0, x1):
                for c in range(3):
                    out[f, y, x, c] = t[f, c, int(frames[f, y, x, c])]
    return out


def grade(bgr, gamma=GRADE_GAMMA, gain=GRADE_GAIN, offset=GRADE_OFFSET):
    """another release's look (test input only): per channel s' = clip(floor(255 (s / 255)^gamma gain + offset + 1/2), 0, 255)"""
    s = np.asarray(bgr, np.uint8).astype(np.float64) / 255.0
    g = 255.0 * s ** np.asarray(gamma, np.float64) * np.asarray(gain, np.float64) + np.asarray(offset, np.float64)
    return np.clip(np.floor(g + 0.5), 0, 255).astype(np.uint8)
