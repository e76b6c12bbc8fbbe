"""NumPy restatement of the source-verified eye (v3d_verify_eye_source_batch; DESIGN.md §4, "Source-verified right eye").  All
integer arithmetic: the GPU must match it bit for bit.

E is one eye as rendered, u8 [H,W,3]; P = stereo_source_ref.eye_plane(sbs, eye, W, H, ax, bx, ay, by) is the stored eye of the SBS
frame sampled at every target, with the source fill's own u, v, clamps, fx, fy and rounding.  The targets are cut into cells of

  cx = (65536 + ax - 1) // ax   by   cy = (65536 + ay - 1) // ay          (1 .. 16 each for ax, ay in [2^12, 2^20]):

the targets that one stored sample spans.  Cell (p, r) holds the targets [p cx, min((p+1) cx, W)) x [r cy, min((r+1) cy, H)), npix
of them.  Per cell and channel c:  A_c = sum E,  B_c = sum P,  m = |A_0 - B_0| + |A_1 - B_1| + |A_2 - B_2|.  The cell is replaced
iff m > tau * npix: every target of it takes P.  Every other byte of E stays.  tau lies in [0, 765]."""
import numpy as np

import stereo_source_ref as X

TAU_MAX = 765
DEFAULT_TAU = 48


def cell(ax, ay):
    if not (X.A_MIN <= ax <= X.A_MAX and X.A_MIN <= ay <= X.A_MAX):
        raise ValueError(f"map scales ({ax}, {ay}) outside [2^12, 2^20]")
    return (65536 + int(ax) - 1) // int(ax), (65536 + int(ay) - 1) // int(ay)


def _check(E, tau, eye):
    E = np.asarray(E)
    if E.dtype != np.uint8 or E.ndim != 3 or E.shape[2] != 3 or E.shape[0] < 1 or E.shape[1] < 1:
        raise ValueError(f"eye image {E.dtype} {E.shape}")
    if isinstance(tau, bool) or int(tau) != tau or not 0 <= tau <= TAU_MAX:
        raise ValueError(f"tau {tau!r} outside [0, {TAU_MAX}]")
    if eye not in (0, 1):
        raise ValueError(f"eye {eye!r}")
    return E


def verdicts(E, P, cx, cy, tau):
    """E, P u8 [H,W,3] -> bool [ceil(H/cy), ceil(W/cx)]: the replaced cells"""
    H, W = E.shape[:2]
    ys, xs = np.arange(0, H, cy), np.arange(0, W, cx)
    d = E.astype(np.int64) - P.astype(np.int64)
    s = np.add.reduceat(np.add.reduceat(d, ys, axis=0), xs, axis=1)                       # A_c - B_c per cell
    npix = np.minimum(cy, H - ys)[:, None] * np.minimum(cx, W - xs)[None, :]
    return np.abs(s).sum(axis=2) > int(tau) * npix


def verify(E, sbs, eye, ax, bx, ay, by, tau):
    """one eye image and its SBS frame -> (the verified eye u8 [H,W,3], the number of replaced cells)"""
    E = _check(E, tau, eye)
    H, W = E.shape[:2]
    cx, cy = cell(ax, ay)
    P = X.eye_plane(sbs, eye, W, H, ax, bx, ay, by)
    bad = verdicts(E, P, cx, cy, tau)
    mask = np.repeat(np.repeat(bad, cy, axis=0), cx, axis=1)[:H, :W]
    return np.where(mask[..., None], P, E), int(bad.sum())


def verify_batch(E, sbs, eye, ax, bx, ay, by, tau):
    """u8 [n,H,W,3], u8 [n,Hs,Ws,3] -> (u8 [n,H,W,3], uint32 [n])"""
    out = [verify(e, s, eye, ax, bx, ay, by, tau) for e, s in zip(E, sbs)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.uint32)


def disturbed(P, seed, amp=40, share=0.15):
    """test scenes: sampled eyes P u8 [n,H,W,3] -> rendered eyes that agree with them up to noise of +-amp, but for `share` of the
    pixels, which have any colour, and `share` of the aligned 8 x 8 blocks, which are black: cells of every size fall on both
    sides of a threshold"""
    rng = np.random.default_rng(seed)
    P = np.asarray(P, np.uint8).astype(np.int64)
    n, H, W = P.shape[:3]
    out = np.clip(P + rng.integers(-amp, amp + 1, P.shape), 0, 255)
    wrong = rng.random((n, H, W)) < share
    out[wrong] = rng.integers(0, 256, (int(wrong.sum()), 3))
    blocks = rng.random((n, -(-H // 8), -(-W // 8))) < share
    out[np.repeat(np.repeat(blocks, 8, axis=1), 8, axis=2)[:, :H, :W]] = 0
    return out.astype(np.uint8)


def verify_loop(E, sbs, eye, ax, bx, ay, by, tau):
    """the same contract as a literal per-pixel loop (small inputs only): what the vectorised form is checked against"""
    E = _check(E, tau, eye)
    H, W = E.shape[:2]
    sbs = np.asarray(sbs, np.uint8)
    Hs, We = sbs.shape[0], sbs.shape[1] // 2
    cx, cy = cell(ax, ay)

    def sample(t, y, c):
        u = min(max(ax * t + bx, 0), (We - 1) << 16)
        v = min(max(ay * y + by, 0), (Hs - 1) << 16)
        i0, fx, j0, fy = u >> 16, (u >> 8) & 255, v >> 16, (v >> 8) & 255
        i1, j1 = min(i0 + 1, We - 1), min(j0 + 1, Hs - 1)
        s = [[int(sbs[j, eye * We + i, c]) for i in (i0, i1)] for j in (j0, j1)]
        top, bot = (256 - fx) * s[0][0] + fx * s[0][1], (256 - fx) * s[1][0] + fx * s[1][1]
        return ((256 - fy) * top + fy * bot + 32768) // 65536

    out, count = E.copy(), 0
    for r in range((H + cy - 1) // cy):
        for p in range((W + cx - 1) // cx):
            targets = [(t, y) for y in range(r * cy, min((r + 1) * cy, H)) for t in range(p * cx, min((p + 1) * cx, W))]
            m = 0
            for c in range(3):
                A = sum(int(E[y, t, c]) for t, y in targets)
                B = sum(sample(t, y, c) for t, y in targets)
                m += abs(A - B)
            if m > tau * len(targets):
                count += 1
                for t, y in targets:
                    for c in range(3):
                        out[y, t, c] = sample(t, y, c)
    return out, count
