"""NumPy restatement of the rendered-eye fidelity record (v3d_eye_fidelity_batch; DESIGN.md §4, "Rendered-eye fidelity report").
All integer arithmetic in int64: the GPU must match it bit for bit.

E is one eye as rendered, u8 [H,W,3]; P = stereo_source_ref.eye_plane(sbs, eye, W, H, ax, bx, ay, by) is the stored eye of the SBS
frame sampled at every target, as in tests/verify_ref.py, and the cells are that file's: cx x cy targets, ncx = ceil(W / cx) by
ncy = ceil(H / cy) of them, ragged last cells of npix targets.  Per cell and channel c (0 = B):

  A_c = sum E,  B_c = sum P,  a_c = (2 A_c + npix) // (2 npix),  b_c likewise             (the cell means, u8)
  colour record:  n_cells,  sad = sum |a_c - b_c|,  ssd = sum (a_c - b_c)^2,  n_bad = #{cells: sum_c |a_c - b_c| > bad_thr}
  luma:  Ya = (9798 a_2 + 19235 a_1 + 3735 a_0 + 16384) >> 15,  Yb likewise from b

SSIM in the x264 / ffmpeg form over windows of 8 x 8 cells at stride 4 (window (i, j): cells [4i, 4i+8) x [4j, 4j+8), for every
i, j with 4i + 8 <= ncx and 4j + 8 <= ncy):

  s1 = sum Ya, s2 = sum Yb, ss = sum (Ya^2 + Yb^2), s12 = sum Ya Yb;  vars = 64 ss - s1^2 - s2^2;  covar = 64 s12 - s1 s2
  A = 2 s1 s2 + C1, B = s1^2 + s2^2 + C1, C = 2 covar + C2, D = vars + C2       (C1 = 416, C2 = 235963; A <= B, |C| <= D)
  q1 = A 2^20 // B,  q2 = |C| 2^20 // D,  Q = sign(C) ((q1 q2) >> 20)

record = (n_cells, sad, ssd, n_bad, n_win, ssim_q20 = sum Q)."""
import numpy as np

import stereo_source_ref as X
import verify_ref as V

FIELDS = 6
BAD_MAX = 765
C1, C2 = 416, 235963
ONE = 1 << 20


def _check(E, eye, bad_thr):
    E = np.asarray(E)
    if E.dtype != np.uint8 or E.ndim != 3 or E.shape[2] != 3 or E.shape[0] < 1 or E.shape[1] < 1:
        raise ValueError(f"eye image {E.dtype} {E.shape}")
    if isinstance(bad_thr, bool) or int(bad_thr) != bad_thr or not 0 <= bad_thr <= BAD_MAX:
        raise ValueError(f"bad threshold {bad_thr!r} outside [0, {BAD_MAX}]")
    if eye not in (0, 1):
        raise ValueError(f"eye {eye!r}")
    return E


def windows(ncx, ncy):
    """(window columns, window rows); (0, 0) when either is 0"""
    nwx, nwy = ((ncx - 8) // 4 + 1 if ncx >= 8 else 0), ((ncy - 8) // 4 + 1 if ncy >= 8 else 0)
    return (nwx, nwy) if nwx and nwy else (0, 0)


def cell_means(I, cx, cy):
    """u8 [H,W,3] -> int64 [ncy,ncx,3]: the rounded cell means"""
    H, W = I.shape[:2]
    ys, xs = np.arange(0, H, cy), np.arange(0, W, cx)
    s = np.add.reduceat(np.add.reduceat(I.astype(np.int64), ys, axis=0), xs, axis=1)
    npix = (np.minimum(cy, H - ys)[:, None] * np.minimum(cx, W - xs)[None, :])[..., None]
    return (2 * s + npix) // (2 * npix)


def luma(m):
    """cell means int64 [..,3] (BGR) -> int64 [..]"""
    return (9798 * m[..., 2] + 19235 * m[..., 1] + 3735 * m[..., 0] + 16384) >> 15


def window_sums(Ya, Yb):
    """luma cell planes int64 [ncy,ncx] -> (s1, s2, ss, s12), int64 [nwy,nwx] each"""
    ncy, ncx = Ya.shape
    nwx, nwy = windows(ncx, ncy)

    def win(p):
        out = np.zeros((nwy, nwx), np.int64)
        for j in range(nwy):
            for i in range(nwx):
                out[j, i] = p[4 * j:4 * j + 8, 4 * i:4 * i + 8].sum()
        return out
    return win(Ya), win(Yb), win(Ya * Ya + Yb * Yb), win(Ya * Yb)


def abcd(s1, s2, ss, s12):
    vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    return 2 * s1 * s2 + C1, s1 * s1 + s2 * s2 + C1, 2 * covar + C2, vars_ + C2


def window_q(s1, s2, ss, s12):
    """int64 arrays -> Q per window, int64 in [-2^20, 2^20]"""
    A, B, C, D = abcd(s1, s2, ss, s12)
    q1, q2 = (A << 20) // B, (np.abs(C) << 20) // D
    return np.sign(C) * ((q1 * q2) >> 20)


def window_ssim_f64(s1, s2, ss, s12):
    """the same windows in float64, from the same sums: what the fixed-point quotients are held to"""
    s1, s2, ss, s12 = (np.asarray(v, np.float64) for v in (s1, s2, ss, s12))
    vars_, covar = ss * 64.0 - s1 * s1 - s2 * s2, s12 * 64.0 - s1 * s2
    return (2.0 * s1 * s2 + C1) * (2.0 * covar + C2) / ((s1 * s1 + s2 * s2 + C1) * (vars_ + C2))


def compare(E, P, cx, cy, bad_thr):
    """E, P u8 [H,W,3] -> the record, int64 [6]"""
    a, b = cell_means(E, cx, cy), cell_means(P, cx, cy)
    d = np.abs(a - b)
    q = window_q(*window_sums(luma(a), luma(b)))
    return np.array([d.shape[0] * d.shape[1], d.sum(), (d * d).sum(), (d.sum(axis=2) > int(bad_thr)).sum(), q.size, q.sum()], np.int64)


def fidelity(E, sbs, eye, ax, bx, ay, by, bad_thr):
    """one eye image and its SBS frame -> the record, int64 [6]"""
    E = _check(E, eye, bad_thr)
    H, W = E.shape[:2]
    cx, cy = V.cell(ax, ay)
    return compare(E, X.eye_plane(sbs, eye, W, H, ax, bx, ay, by), cx, cy, bad_thr)


def fidelity_batch(E, sbs, eye, ax, bx, ay, by, bad_thr):
    """u8 [n,H,W,3], u8 [n,Hs,Ws,3] -> int64 [n,6]"""
    return np.stack([fidelity(e, s, eye, ax, bx, ay, by, bad_thr) for e, s in zip(E, sbs)])


def fidelity_loop(E, sbs, eye, ax, bx, ay, by, bad_thr):
    """the same contract as a literal loop over cells and windows in Python integers (small inputs only)"""
    E = _check(E, eye, bad_thr)
    H, W = E.shape[:2]
    cx, cy = V.cell(ax, ay)
    P = X.eye_plane(sbs, eye, W, H, ax, bx, ay, by)
    ncx, ncy = -(-W // cx), -(-H // cy)
    sad = ssd = bad = 0
    Y = [[None] * ncx for _ in range(ncy)]
    for r in range(ncy):
        for p in range(ncx):
            ys, xs = slice(r * cy, min((r + 1) * cy, H)), slice(p * cx, min((p + 1) * cx, W))
            npix = (ys.stop - ys.start) * (xs.stop - xs.start)
            a = [(2 * int(E[ys, xs, c].sum(dtype=np.int64)) + npix) // (2 * npix) for c in range(3)]
            b = [(2 * int(P[ys, xs, c].sum(dtype=np.int64)) + npix) // (2 * npix) for c in range(3)]
            d = [abs(x - y) for x, y in zip(a, b)]
            sad, ssd, bad = sad + sum(d), ssd + sum(v * v for v in d), bad + (sum(d) > bad_thr)
            Y[r][p] = tuple((9798 * m[2] + 19235 * m[1] + 3735 * m[0] + 16384) >> 15 for m in (a, b))
    nwx, nwy = windows(ncx, ncy)
    total = 0
    for j in range(nwy):
        for i in range(nwx):
            cells = [Y[r][p] for r in range(4 * j, 4 * j + 8) for p in range(4 * i, 4 * i + 8)]
            s1, s2 = sum(c[0] for c in cells), sum(c[1] for c in cells)
            ss, s12 = sum(c[0] ** 2 + c[1] ** 2 for c in cells), sum(c[0] * c[1] for c in cells)
            A, B, C, D = abcd(s1, s2, ss, s12)
            assert 0 < A <= B < 1 << 31 and abs(C) <= D < 1 << 31
            q = (((A << 20) // B) * ((abs(C) << 20) // D)) >> 20
            total += -q if C < 0 else q
    return np.array([ncx * ncy, sad, ssd, bad, nwx * nwy, total], np.int64)
