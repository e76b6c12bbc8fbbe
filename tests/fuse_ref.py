"""NumPy restatement of the source-fused eye (v3d_fuse_eye_source_batch; DESIGN.md §4, "Source-fused right eye").  All integer
arithmetic: the GPU must match it bit for bit.

E is one eye as rendered (and possibly verified), u8 [H,W,3]; P = stereo_source_ref.eye_plane(sbs, eye, W, H, ax, bx, ay, by) is the
stored eye of the SBS frame sampled at every target.  Per axis (coefficient a, offset b, Nd targets, Ns samples), for target t:

  q(t) = clamp(a t + b, 0, (Ns - 1) << 16)  (64-bit),  near(t) = (q + 32768) >> 16,  lo = near(0),  hi = near(Nd - 1);
  i0 = q >> 16, i1 = min(i0 + 1, Ns - 1), f = (q >> 8) & 255: stereo_source_ref._taps.

With a <= 65536 near never steps by more than 1, so every sample of [lo, hi] owns at least one target; a larger scale is refused.
Means plane, j in [jlo, jhi], i in [ilo, ihi]:  A = sum of E[y][t][c] over the targets with near_y(y) = j and near_x(t) = i, N their
number, M[j][i][c] = (2 A + N) // (2 N).  Low band: LP = the bilinear formula of P with the same fx, fy over M, the tap indices
clamped to the populated range.  Result: out = clamp(E - LP + P, 0, 255); every byte of E is written."""
import numpy as np

import stereo_source_ref as X

A_FUSE_MAX = 65536                                             # one stored sample per target at most


def _check(E, eye, ax, ay):
    E = np.asarray(E)
    if E.dtype != np.uint8 or E.ndim != 3 or E.shape[2] != 3 or E.shape[0] < 1 or E.shape[1] < 1:
        raise ValueError(f"eye image {E.dtype} {E.shape}")
    if eye not in (0, 1):
        raise ValueError(f"eye {eye!r}")
    if not (X.A_MIN <= ax <= A_FUSE_MAX and X.A_MIN <= ay <= A_FUSE_MAX):
        raise ValueError(f"map scales ({ax}, {ay}) outside [2^12, 2^16]")
    return E


def near(coef, off, n_dst, n_src):
    """the sample nearest to every target, int64 [n_dst]"""
    t = np.arange(n_dst, dtype=np.int64)
    return (np.clip(int(coef) * t + int(off), 0, (n_src - 1) << 16) + 32768) >> 16


def footprint_counts(coef, off, n_dst, n_src):
    """(lo, counts): the targets that each sample of the populated range [lo, hi] owns, int64 [hi - lo + 1]"""
    n = near(coef, off, n_dst, n_src)
    return int(n[0]), np.bincount(n - n[0], minlength=int(n[-1] - n[0]) + 1)


def means(E, ax, bx, ay, by, We, Hs):
    """E u8 [H,W,3] -> (M u8 [jhi - jlo + 1, ihi - ilo + 1, 3], (ilo, ihi, jlo, jhi))"""
    H, W = E.shape[:2]
    (ilo, nx), (jlo, ny) = footprint_counts(ax, bx, W, We), footprint_counts(ay, by, H, Hs)
    if not (nx > 0).all() or not (ny > 0).all():
        raise ValueError("a sample of the populated range owns no target")
    xs, ys = np.cumsum(nx) - nx, np.cumsum(ny) - ny             # near is monotone: a sample's targets are a run
    A = np.add.reduceat(np.add.reduceat(E.astype(np.int64), ys, axis=0), xs, axis=1)
    N = (ny[:, None] * nx[None, :])[..., None]
    return ((2 * A + N) // (2 * N)).astype(np.uint8), (ilo, ilo + len(nx) - 1, jlo, jlo + len(ny) - 1)


def low_band(M, rng, W, H, ax, bx, ay, by, We, Hs):
    """the means plane sampled back at every target -> LP u8 [H,W,3]"""
    ilo, ihi, jlo, jhi = rng
    i0, i1, fx = X._taps(ax, bx, W, We)
    j0, j1, fy = X._taps(ay, by, H, Hs)
    i0, i1, j0, j1 = np.clip(i0, ilo, ihi) - ilo, np.clip(i1, ilo, ihi) - ilo, np.clip(j0, jlo, jhi) - jlo, np.clip(j1, jlo, jhi) - jlo
    M = M.astype(np.int32)                                      # every term is below 2^24 + 2^15
    fx, fy = fx[None, :, None].astype(np.int32), fy[:, None, None].astype(np.int32)
    top = (256 - fx) * M[j0][:, i0] + fx * M[j0][:, i1]
    bot = (256 - fx) * M[j1][:, i0] + fx * M[j1][:, i1]
    return (((256 - fy) * top + fy * bot + 32768) >> 16).astype(np.uint8)


def fuse(E, sbs, eye, ax, bx, ay, by):
    """one eye image and its SBS frame -> the fused eye u8 [H,W,3]"""
    E = _check(E, eye, ax, ay)
    H, W = E.shape[:2]
    sbs = np.asarray(sbs, np.uint8)
    Hs, We = sbs.shape[0], sbs.shape[1] // 2
    P = X.eye_plane(sbs, eye, W, H, ax, bx, ay, by)
    M, rng = means(E, ax, bx, ay, by, We, Hs)
    LP = low_band(M, rng, W, H, ax, bx, ay, by, We, Hs)
    return np.clip(E.astype(np.int16) - LP + P, 0, 255).astype(np.uint8)


def fuse_batch(E, sbs, eye, ax, bx, ay, by):
    """u8 [n,H,W,3], u8 [n,Hs,Ws,3] -> u8 [n,H,W,3]"""
    return np.stack([fuse(e, s, eye, ax, bx, ay, by) for e, s in zip(E, sbs)])


def fuse_loop(E, sbs, eye, ax, bx, ay, by):
    """the same contract as a literal per-pixel loop (small inputs only): what the vectorised form is checked against"""
    E = _check(E, eye, ax, ay)
    H, W = E.shape[:2]
    sbs = np.asarray(sbs, np.uint8)
    Hs, We = sbs.shape[0], sbs.shape[1] // 2

    def axis(a, b, t, Ns):
        q = min(max(a * t + b, 0), (Ns - 1) << 16)
        return (q + 32768) >> 16, q >> 16, min((q >> 16) + 1, Ns - 1), (q >> 8) & 255

    xs, ys = [axis(ax, bx, t, We) for t in range(W)], [axis(ay, by, y, Hs) for y in range(H)]
    ilo, ihi, jlo, jhi = xs[0][0], xs[-1][0], ys[0][0], ys[-1][0]
    A, N = {}, {}
    for y in range(H):
        for t in range(W):
            k = (ys[y][0], xs[t][0])
            N[k] = N.get(k, 0) + 1
            for c in range(3):
                A[k + (c,)] = A.get(k + (c,), 0) + int(E[y, t, c])

    def mean(j, i, c):
        j, i = min(max(j, jlo), jhi), min(max(i, ilo), ihi)
        return (2 * A[(j, i, c)] + N[(j, i)]) // (2 * N[(j, i)])

    def bilinear(tap, y, t, c):
        _, j0, j1, fy = ys[y]
        _, i0, i1, fx = xs[t]
        top, bot = (256 - fx) * tap(j0, i0, c) + fx * tap(j0, i1, c), (256 - fx) * tap(j1, i0, c) + fx * tap(j1, i1, c)
        return ((256 - fy) * top + fy * bot + 32768) // 65536

    out = np.empty_like(E)
    for y in range(H):
        for t in range(W):
            for c in range(3):
                p = bilinear(lambda j, i, ch: int(sbs[j, eye * We + i, ch]), y, t, c)
                out[y, t, c] = min(max(int(E[y, t, c]) - bilinear(mean, y, t, c) + p, 0), 255)
    return out
