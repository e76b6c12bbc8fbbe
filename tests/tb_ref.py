"""The contract of the top-bottom split (v3d_tb_to_gray, v3d_tb_to_gray_batch, v3d_split_tb; include/v3d_hip.h), twice:

  split / to_gray        a NumPy int64 restatement of the arithmetic the header states: eye e of a W x H frame is rows e Hh ..
                         e Hh + Hh - 1 (Hh = H / 2, left eye on top); unsqueezed, output rows 2m and 2m + 1 are the 8-tap sums
                         of rows m - 4 .. m + 3 (taps of the fraction 0.75) and m - 3 .. m + 4 (fraction 0.25), rows clamped to
                         the eye, descaled by (acc + 1024) >> 11 and saturated; gray is the luma of the clamped channels
  split_by_transposition the existing oracle with the axes swapped: each eye transposed, the two side by side as an H-wide,
                         W-high SBS frame through oracle.split_sbs(., True), transposed back; gray = oracle.bgr_to_gray of it

Neither touches the code under test; tests/test_tb_ref.py pins that they agree byte for byte.  Test infrastructure only."""
import numpy as np

from oracle import oracle as O


def eyes(tb):
    """[H,W,3] -> (top, bottom) = (left, right), H even"""
    H = tb.shape[0]
    if H % 2 or H < 2:
        raise ValueError("top-bottom frame height must be even")
    return tb[:H // 2], tb[H // 2:]


def stretch(eye):
    """one eye [Hh,W,C] u8 -> [2 Hh,W,C] u8"""
    S = np.asarray(eye, np.int64)
    Hh = S.shape[0]
    t0, t1 = O.lanczos4_taps(0.75).astype(np.int64), O.lanczos4_taps(0.25).astype(np.int64)
    m = np.arange(Hh)
    acc = np.zeros((2 * Hh,) + S.shape[1:], np.int64)
    for k in range(8):
        acc[0::2] += t0[k] * S[np.clip(m - 4 + k, 0, Hh - 1)]
        acc[1::2] += t1[k] * S[np.clip(m - 3 + k, 0, Hh - 1)]
    return np.clip((acc + 1024) >> 11, 0, 255).astype(np.uint8)


def gray_of(bgr):
    b, g, r = (np.asarray(bgr[..., c], np.int64) for c in range(3))
    return ((r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def split(tb, unsqueeze=True):
    """[H,W,3] BGR -> (left, right) BGR [H or H/2, W, 3]"""
    top, bottom = eyes(np.asarray(tb, np.uint8))
    if not unsqueeze:
        return np.ascontiguousarray(top), np.ascontiguousarray(bottom)
    return stretch(top), stretch(bottom)


def to_gray(tb, unsqueeze=True):
    """[H,W,3] BGR -> (left, right) gray [H or H/2, W]"""
    L, R = split(tb, unsqueeze)
    return gray_of(L), gray_of(R)


def to_gray_batch(frames, unsqueeze=True):
    both = [to_gray(f, unsqueeze) for f in frames]
    return np.stack([b[0] for b in both]), np.stack([b[1] for b in both])


def split_by_transposition(tb):
    """the unsqueezed BGR eyes through oracle.split_sbs on the transposed frame"""
    top, bottom = eyes(np.asarray(tb, np.uint8))
    sbs = np.concatenate([top.transpose(1, 0, 2), bottom.transpose(1, 0, 2)], axis=1)      # [W, 2 Hh, 3]: H wide, W high
    L, R = O.split_sbs(np.ascontiguousarray(sbs), True)                                     # [W, 2 Hh, 3] each
    return np.ascontiguousarray(L.transpose(1, 0, 2)), np.ascontiguousarray(R.transpose(1, 0, 2))


def to_gray_by_transposition(tb):
    L, R = split_by_transposition(tb)
    return O.bgr_to_gray(L), O.bgr_to_gray(R)


def content(n, H, W, seed):
    """random frames [n,H,W,3] with saturated 255 and 0 bands of rows across the seam and inside each eye: hard edges overshoot
    under Lanczos (the saturation), and a leak across the seam would show"""
    tb = np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    Hh = H // 2
    tb[:, max(Hh - 3, 0):Hh] = 255
    tb[:, Hh:min(Hh + 3, H)] = 0
    if Hh >= 8:
        tb[:, Hh // 4:Hh // 4 + 2, : W // 2] = 0
        tb[:, Hh + Hh // 2:Hh + Hh // 2 + 2, W // 2:] = 255
    return tb
