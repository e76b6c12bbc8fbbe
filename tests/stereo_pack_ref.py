"""NumPy restatement of the output packings of the DIBR step (v3d_render_stereo_packed_batch; DESIGN.md §4, "Output packings").
All integer arithmetic: the GPU must match it bit for bit.

The eye images EL, ER ([H][W][3] BGR u8) are those of tests/stereo_ref.py (steps 1-4) for the integer render and of
tests/stereo_sub_ref.py for the sub-pixel render.  Step 5, the packing:

  0 FULL_SBS         [H][2W][3]  EL | ER
  1 HALF_SBS         [H][W][3]   W even: eye pixel x' = (E[2x'] + E[2x'+1] + 1) >> 1, EL | ER
  2 FULL_TB          [2H][W][3]  EL above ER
  3 HALF_TB          [H][W][3]   H even: eye row y' = (E[2y'] + E[2y'+1] + 1) >> 1, EL above ER
  4 ROWS             [H][W][3]   row y = EL[y] for even y, ER[y] for odd y
  5 ANAGLYPH_COLOUR  [H][W][3]   B = ER.B, G = ER.G, R = EL.R
  6 ANAGLYPH_DUBOIS  [H][W][3]   (B', G', R') = clamp255((DUBOIS @ (Rl, Gl, Bl, Rr, Gr, Br) + 32768) >> 16)
"""
import numpy as np

import stereo_ref as R
import stereo_sub_ref as S

FULL_SBS, HALF_SBS, FULL_TB, HALF_TB, ROWS, ANAGLYPH_COLOUR, ANAGLYPH_DUBOIS = range(7)
PACKINGS = tuple(range(7))
NAMES = {FULL_SBS: "full-sbs", HALF_SBS: "half-sbs", FULL_TB: "full-tb", HALF_TB: "half-tb", ROWS: "interlaced",
         ANAGLYPH_COLOUR: "anaglyph-colour", ANAGLYPH_DUBOIS: "anaglyph-dubois"}

# Dubois' least-squares red-cyan matrices in 1/65536: rows R', G', B'; columns Rl, Gl, Bl, Rr, Gr, Br.  Every row sums to 65536.
DUBOIS = np.array([[29891, 32800, 11559, -2849, -5763, -102],
                   [-2627, -2479, -1033, 24804, 48080, -1209],
                   [-997, -1350, -358, -4729, -7403, 80373]], np.int64)


def output_size(packing, W, H):
    """(outW, outH)"""
    if packing not in PACKINGS:
        raise ValueError(f"packing {packing}")
    if packing == HALF_SBS and W % 2:
        raise ValueError("half SBS needs an even width")
    if packing == HALF_TB and H % 2:
        raise ValueError("half top-bottom needs an even height")
    return (2 * W if packing == FULL_SBS else W), (2 * H if packing == FULL_TB else H)


def dubois_unclamped(l_bgr, r_bgr):
    """BGR [...,3] of the left and the right eye -> the three sums (B', G', R') after the floor, before the clamp (int64)"""
    l, r = np.asarray(l_bgr).astype(np.int64), np.asarray(r_bgr).astype(np.int64)
    v = np.stack([l[..., 2], l[..., 1], l[..., 0], r[..., 2], r[..., 1], r[..., 0]], axis=-1)     # Rl Gl Bl Rr Gr Br
    rgb = (v @ DUBOIS.T + 32768) >> 16                                                         # >> on int64 is the floor
    return rgb[..., ::-1]


def pack(EL, ER, packing):
    """the two eye images u8 [H,W,3] -> the packed frame u8 [outH,outW,3]"""
    EL, ER = np.asarray(EL, np.uint8), np.asarray(ER, np.uint8)
    H, W = EL.shape[:2]
    output_size(packing, W, H)
    eyes = [EL, ER]
    if packing == FULL_SBS:
        return np.concatenate(eyes, axis=1)
    if packing == HALF_SBS:
        return np.concatenate([((e[:, 0::2].astype(np.uint16) + e[:, 1::2] + 1) >> 1).astype(np.uint8) for e in eyes], axis=1)
    if packing == FULL_TB:
        return np.concatenate(eyes, axis=0)
    if packing == HALF_TB:
        return np.concatenate([((e[0::2].astype(np.uint16) + e[1::2] + 1) >> 1).astype(np.uint8) for e in eyes], axis=0)
    if packing == ROWS:
        out = EL.copy()
        out[1::2] = ER[1::2]
        return out
    if packing == ANAGLYPH_COLOUR:
        out = ER.copy()
        out[..., 2] = EL[..., 2]
        return out
    return np.clip(dubois_unclamped(EL, ER), 0, 255).astype(np.uint8)


def pack_loop(EL, ER, packing):
    """the same rules as a literal per-pixel loop (small inputs only): what the vectorised form is checked against"""
    H, W = EL.shape[:2]
    oW, oH = output_size(packing, W, H)
    out = np.zeros((oH, oW, 3), np.uint8)
    E = (EL, ER)
    for y in range(oH):
        for x in range(oW):
            for c in range(3):
                if packing == FULL_SBS:
                    v = int(E[x // W][y, x % W, c])
                elif packing == HALF_SBS:
                    e, xx = E[x // (W // 2)], x % (W // 2)
                    v = (int(e[y, 2 * xx, c]) + int(e[y, 2 * xx + 1, c]) + 1) >> 1
                elif packing == FULL_TB:
                    v = int(E[y // H][y % H, x, c])
                elif packing == HALF_TB:
                    e, yy = E[y // (H // 2)], y % (H // 2)
                    v = (int(e[2 * yy, x, c]) + int(e[2 * yy + 1, x, c]) + 1) >> 1
                elif packing == ROWS:
                    v = int(E[y % 2][y, x, c])
                elif packing == ANAGLYPH_COLOUR:
                    v = int((EL if c == 2 else ER)[y, x, c])
                else:
                    k = DUBOIS[2 - c]                                                          # channel c of BGR: row 2 - c of R'G'B'
                    bl, gl, rl = (int(t) for t in EL[y, x])
                    br, gr, rr = (int(t) for t in ER[y, x])
                    s = int(k[0]) * rl + int(k[1]) * gl + int(k[2]) * bl + int(k[3]) * rr + int(k[4]) * gr + int(k[5]) * br + 32768
                    v = min(max(s // 65536, 0), 255)                                           # // is the floor
                out[y, x, c] = v
    return out


def eyes(frame, depth, gain_left, gain_right, conv, subpixel=False):
    """one frame: BGR u8 [H,W,3], u16 depth [H,W] -> (EL, ER) of the integer or the sub-pixel render"""
    F = np.asarray(frame, np.uint8)
    D = np.asarray(depth, np.uint16)
    if F.shape[:2] != D.shape or F.ndim != 3 or F.shape[2] != 3:
        raise ValueError(f"frame {F.shape} and depth {D.shape} disagree")
    if subpixel:
        return tuple(S.eye_image(F, D, g, conv)[0] for g in (gain_left, gain_right))
    return tuple(R.eye_image(F, R.eye_keys(D, g, conv)) for g in (gain_left, gain_right))


def render(frame, depth, gain_left, gain_right, conv, packing, subpixel=False):
    """one frame -> the packed frame u8 [outH,outW,3]"""
    return pack(*eyes(frame, depth, gain_left, gain_right, conv, subpixel), packing)
