"""NumPy restatement of the source fill of the DIBR step (v3d_render_stereo_source_batch; DESIGN.md §4, "Source-faithful 3D").
All integer arithmetic: the GPU must match it bit for bit.

The render is that of tests/stereo_pack_ref.py (the integer contract of tests/stereo_ref.py or the sub-pixel contract of
tests/stereo_sub_ref.py, then the packing), with one difference: in an eye whose bit is set in fill_eyes (bit 0 left, bit 1 right) a
target t of row y that no source reached (Z[t] == 0) takes P(eye)[y][t], the stored eye of the SBS frame sampled bilinearly:

  We = Ws / 2; eye e's column i is SBS column e * We + i (S below is that eye's [Hs][We][3] plane);
  u = clamp(ax * t + bx, 0, (We - 1) << 16), v = clamp(ay * y + by, 0, (Hs - 1) << 16)          (Q16 coordinates, 64-bit)
  i0 = u >> 16, i1 = min(i0 + 1, We - 1), fx = (u >> 8) & 255; j0, j1, fy from v in the same way
  P = ((256 - fy) * ((256 - fx) * S[j0][i0] + fx * S[j0][i1]) + fy * ((256 - fx) * S[j1][i0] + fx * S[j1][i1]) + 32768) >> 16

per channel: the arithmetic of v3d_warp_u16_batch (tests/register_ref.py), with the coordinates clamped to the eye in place of a fill
value.  An eye whose bit is clear fills its holes from the background as before; fill_eyes = 0 is stereo_pack_ref.render.
"""
import numpy as np

import stereo_pack_ref as P
import stereo_ref as R
import stereo_sub_ref as S

A_MIN, A_MAX, B_MAX = 1 << 12, 1 << 20, 1 << 40                # legal map scales and offsets


def identity_map(n_src, n_dst):
    """(a, b) in Q16 of the map that lays n_src source samples over n_dst targets, pixel centres aligned: target t reads source
    (t + 1/2) n_src / n_dst - 1/2.  Exact for the sizes used here (n_dst a power of two times a divisor of n_src * 32768)."""
    a = (n_src << 16) // n_dst
    return a, (a - 65536) // 2


def _taps(coef, off, n_dst, n_src):
    t = np.arange(n_dst, dtype=np.int64)
    q = np.clip(int(coef) * t + int(off), 0, (n_src - 1) << 16)
    i0 = q >> 16
    return i0, np.minimum(i0 + 1, n_src - 1), (q >> 8) & 255


def eye_plane(sbs, eye, W, H, ax, bx, ay, by):
    """SBS BGR u8 [Hs,Ws,3] -> P(eye) u8 [H,W,3]"""
    sbs = np.asarray(sbs, np.uint8)
    Hs, Ws = sbs.shape[:2]
    if Ws < 2 or Ws % 2 or sbs.ndim != 3 or sbs.shape[2] != 3:
        raise ValueError(f"SBS frame {sbs.shape}")
    We = Ws // 2
    E = sbs[:, eye * We:(eye + 1) * We].astype(np.int64)
    i0, i1, fx = _taps(ax, bx, W, We)
    j0, j1, fy = _taps(ay, by, H, Hs)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = (256 - fx) * E[j0][:, i0] + fx * E[j0][:, i1]
    bot = (256 - fx) * E[j1][:, i0] + fx * E[j1][:, i1]
    return (((256 - fy) * top + fy * bot + 32768) >> 16).astype(np.uint8)


def hit_mask(depth, gain, conv, subpixel=False):
    """u16 depth [H,W] -> bool [H,W]: target t of row y was reached by a source (Z[t] != 0), steps 1-2 / 1-3 of the two contracts"""
    D = np.asarray(depth).astype(np.int64)
    H, W = D.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    hit = np.zeros((H, W), bool)
    rows = np.broadcast_to(np.arange(H)[:, None], D.shape)
    if not subpixel:
        t = x + ((int(gain) * (D - int(conv)) + (1 << 23)) >> 24)
        keep = (t >= 0) & (t < W)
        hit[rows[keep], t[keep]] = True
        return hit
    p = 16 * x + ((int(gain) * (D - int(conv)) + (1 << 19)) >> 20)
    Lp = np.zeros_like(p)
    Lp[:, :-1] = p[:, 1:] - p[:, :-1]
    L = np.where((x + 1 < W) & (Lp > 0) & (Lp <= S.TEAR16), Lp, 16)
    t0 = (p + 15) >> 4
    for t in (t0, t0 + 1):
        keep = (16 * t < p + L) & (t >= 0) & (t < W)
        hit[rows[keep], t[keep]] = True
    return hit


def eyes(frame, depth, gain_left, gain_right, conv, subpixel, sbs, fill_eyes, ax, bx, ay, by):
    """one frame -> (EL, ER) with the holes of the eyes named by fill_eyes taken from the stored eye"""
    if fill_eyes not in (0, 1, 2, 3):
        raise ValueError(f"fill_eyes {fill_eyes}")
    out = list(P.eyes(frame, depth, gain_left, gain_right, conv, subpixel))
    H, W = np.asarray(depth).shape
    for e, g in enumerate((gain_left, gain_right)):
        if (fill_eyes >> e) & 1:
            hole = ~hit_mask(depth, g, conv, subpixel)
            out[e] = np.where(hole[..., None], eye_plane(sbs, e, W, H, ax, bx, ay, by), out[e])
    return tuple(out)


def render(frame, depth, gain_left, gain_right, conv, packing, subpixel=False, sbs=None, fill_eyes=0, ax=65536, bx=0, ay=65536, by=0):
    """one frame -> the packed frame u8 [outH,outW,3]"""
    return P.pack(*eyes(frame, depth, gain_left, gain_right, conv, subpixel, sbs, fill_eyes, ax, bx, ay, by), packing)


def render_loop(frame, depth, gain_left, gain_right, conv, packing, subpixel=False, sbs=None, fill_eyes=0, ax=65536, bx=0, ay=65536,
                by=0):
    """the same contract as a literal per-pixel loop (small inputs only): what the vectorised form is checked against"""
    F, D = np.asarray(frame, np.uint8), np.asarray(depth, np.uint16)
    H, W = D.shape
    full = (S.render_loop(F, D, gain_left, gain_right, conv)[0] if subpixel else R.render_loop(F, D, gain_left, gain_right, conv))
    E = [full[:, :W].copy(), full[:, W:].copy()]
    for e, g in enumerate((gain_left, gain_right)):
        if not (fill_eyes >> e) & 1:
            continue
        Hs, We = sbs.shape[0], sbs.shape[1] // 2
        for y in range(H):
            hit = [False] * W
            for x in range(W):
                d = int(D[y, x])
                if subpixel:
                    p = 16 * x + (g * (d - conv) + (1 << 19)) // (1 << 20)
                    L = 16
                    if x + 1 < W:
                        Lp = 16 * (x + 1) + (g * (int(D[y, x + 1]) - conv) + (1 << 19)) // (1 << 20) - p
                        if 0 < Lp <= S.TEAR16:
                            L = Lp
                    targets = [t for t in range(p // 16 - 1, p // 16 + 4) if p <= 16 * t < p + L]
                else:
                    targets = [x + (g * (d - conv) + (1 << 23)) // (1 << 24)]
                for t in targets:
                    if 0 <= t < W:
                        hit[t] = True
            v = min(max(ay * y + by, 0), (Hs - 1) << 16)
            j0, fy = v >> 16, (v >> 8) & 255
            j1 = min(j0 + 1, Hs - 1)
            for t in range(W):
                if hit[t]:
                    continue
                u = min(max(ax * t + bx, 0), (We - 1) << 16)
                i0, fx = u >> 16, (u >> 8) & 255
                i1 = min(i0 + 1, We - 1)
                for c in range(3):
                    s = [[int(sbs[j, e * We + i, c]) for i in (i0, i1)] for j in (j0, j1)]
                    top, bot = (256 - fx) * s[0][0] + fx * s[0][1], (256 - fx) * s[1][0] + fx * s[1][1]
                    E[e][y, t, c] = ((256 - fy) * top + fy * bot + 32768) // 65536
    return P.pack_loop(E[0], E[1], packing)
