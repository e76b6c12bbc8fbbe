"""NumPy restatement of the DIBR stereo rendering contract (v3d_render_stereo_batch; DESIGN.md §4, "DIBR stereo rendering").
All integer arithmetic: the GPU must match it bit for bit.

For each row y and each eye with gain g:
  1. shift: t = x + floor((g * (D[y][x] - conv) + 2^23) / 2^24); sources with t outside [0, W) are dropped;
  2. z-buffer: Z[t] = max over kept sources of (D[y][x] << 16) | (x + 1) (u32), 0 where nothing landed;
  3. hole fill: a zero Z[t] takes the nearest non-zero key on its left (a) or right (b): the farther one, (Z[a] >> 16) <=
     (Z[b] >> 16) -> a; the only one if one side has none; 0 (black) if the row has no key at all;
  4. colour: F[y][(K & 0xFFFF) - 1], black for K == 0;
  5. layout: full SBS [H][2W][3] (left eye first); half SBS [H][W][3], eye pixel x' = (E[2x'] + E[2x'+1] + 1) >> 1.
"""
import math

import numpy as np

FULL_SBS, HALF_SBS = 0, 1


def stereo_gains(max_shift=48.0, convergence=0.5, eye_split=0.5):
    """the host mapping from the user parameters, exactly as specified"""
    gl = math.floor(max_shift * eye_split * 256 + 0.5)
    gr = -math.floor(max_shift * (1 - eye_split) * 256 + 0.5)
    return gl, gr, math.floor(convergence * 65535 + 0.5)


def far_key_scene():
    """(F, D, gains) of a 2048 x 2 frame (8 targets per thread, 512 per wave) whose nearest key lies more than one wave's run
    away or does not exist: the near half (65535) moves 600 px.  Row 0: a 600-target hole at [1024, 1624) in the left eye, a
    600-target tail without a right neighbour in the right eye; row 1 mirrors it (a head without a left neighbour)."""
    W, H = 2048, 2
    F = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    D = np.zeros((H, W), np.uint16)
    D[0, 1024:] = 65535
    D[1, :1024] = 65535
    return F, D, stereo_gains(1200, 0.0, 0.5)


def eye_keys(depth, gain, conv):
    """u16 depth [H,W] -> the filled key rows K [H,W] (int64 holding the u32 keys)"""
    D = np.asarray(depth).astype(np.int64)
    H, W = D.shape
    x = np.arange(W, dtype=np.int64)
    t = x[None, :] + ((int(gain) * (D - int(conv)) + (1 << 23)) >> 24)          # >> on int64 is floor division
    key = (D << 16) | (x[None, :] + 1)
    keep = (t >= 0) & (t < W)
    flat = (np.arange(H, dtype=np.int64)[:, None] * W + t)[keep]
    Z = np.zeros(H * W, np.int64)
    np.maximum.at(Z, flat, key[keep])
    Z = Z.reshape(H, W)
    nz = Z != 0
    a = np.maximum.accumulate(np.where(nz, x[None, :], -1), axis=1)             # last key at or left of t
    b = np.minimum.accumulate(np.where(nz, x[None, :], W)[:, ::-1], axis=1)[:, ::-1]   # first key at or right of t
    Za = np.where(a >= 0, np.take_along_axis(Z, np.clip(a, 0, W - 1), axis=1), 0)
    Zb = np.where(b < W, np.take_along_axis(Z, np.clip(b, 0, W - 1), axis=1), 0)
    both = (Za != 0) & (Zb != 0)
    fill = np.where(both, np.where((Za >> 16) <= (Zb >> 16), Za, Zb), np.where(Za != 0, Za, Zb))
    return np.where(nz, Z, fill)


def eye_image(frame, K):
    """BGR u8 [H,W,3] + keys [H,W] -> the eye image [H,W,3]"""
    F = np.asarray(frame, np.uint8)
    src = np.clip((K & 0xFFFF) - 1, 0, F.shape[1] - 1)
    E = np.take_along_axis(F, src[..., None], axis=1)
    return np.where((K != 0)[..., None], E, 0).astype(np.uint8)


def render(frame, depth, gain_left, gain_right, conv, layout=FULL_SBS):
    """one frame: BGR u8 [H,W,3], u16 depth [H,W] -> u8 [H,2W,3] (full SBS) or [H,W,3] (half SBS)"""
    F = np.asarray(frame, np.uint8)
    D = np.asarray(depth, np.uint16)
    if F.shape[:2] != D.shape or F.ndim != 3 or F.shape[2] != 3:
        raise ValueError(f"frame {F.shape} and depth {D.shape} disagree")
    eyes = [eye_image(F, eye_keys(D, g, conv)) for g in (gain_left, gain_right)]
    if layout == HALF_SBS:
        if D.shape[1] % 2:
            raise ValueError("half SBS needs an even width")
        eyes = [((e[:, 0::2].astype(np.uint16) + e[:, 1::2] + 1) >> 1).astype(np.uint8) for e in eyes]
    elif layout != FULL_SBS:
        raise ValueError(f"layout {layout}")
    return np.concatenate(eyes, axis=1)


def render_loop(frame, depth, gain_left, gain_right, conv, layout=FULL_SBS):
    """the same contract as a literal per-pixel loop (small inputs only): what the vectorised form is checked against"""
    F = np.asarray(frame, np.uint8)
    D = np.asarray(depth, np.uint16)
    H, W = D.shape
    out = []
    for g in (gain_left, gain_right):
        E = np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            Z = [0] * W
            for x in range(W):
                d = int(D[y, x])
                t = x + (g * (d - conv) + (1 << 23)) // (1 << 24)
                if 0 <= t < W:
                    Z[t] = max(Z[t], (d << 16) | (x + 1))
            for t in range(W):
                k = Z[t]
                if k == 0:
                    za = next((Z[i] for i in range(t - 1, -1, -1) if Z[i]), 0)
                    zb = next((Z[i] for i in range(t + 1, W) if Z[i]), 0)
                    if za and zb:
                        k = za if (za >> 16) <= (zb >> 16) else zb
                    else:
                        k = za or zb
                if k:
                    E[y, t] = F[y, (k & 0xFFFF) - 1]
        if layout == HALF_SBS:
            h = np.zeros((H, W // 2, 3), np.uint8)
            for y in range(H):
                for x in range(W // 2):
                    for c in range(3):
                        h[y, x, c] = (int(E[y, 2 * x, c]) + int(E[y, 2 * x + 1, c]) + 1) >> 1
            E = h
        out.append(E)
    return np.concatenate(out, axis=1)
