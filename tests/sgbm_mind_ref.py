"""NumPy restatement of the matcher with a negative search window, minDisparity m in [-64, 0] (test helper, tiny images only).

The contract ("minDisparity"), with D = 64, W1 = W - 64, x1 in [0, W1), d' in [0, 64):
  cost     C[y][x1][d'] compares the left record of image column x1 + 64 + m with the right record of column x1 + 64 - d';
           records (gradient, raw byte, their Birchfield-Tomasi intervals) keep the real image borders
  paths    aggregation, winner-take-all, uniqueness, sub-pixel and the L-R check run on (x1, d') exactly as for m = 0
  output   raw[y][x1 + 64 + m] = rel16 + 16 m, INVALID = 16 (m - 1) at rejected pixels and at every column outside
           [64 + m, W + m); then the 3x3 median and the speckle filter with newVal = 16 (m - 1)
Built from np_sgm's functions (planes, intervals, paths, WTA); the median and the speckle filter are the oracle's."""
import numpy as np

import np_sgm

D = 64


def invalid(m):
    return 16 * (m - 1)


def cost_volume(L, R, m=0, P2=2400, ft=15, half=2):
    """np_sgm.cost_volume with the left planes read at column x1 + 64 + m"""
    H, W = L.shape
    W1 = W - D
    pix = np.zeros((H, W1, D), np.int32)
    for (p1, p2), shift in zip(zip(np_sgm._planes(L, ft), np_sgm._planes(R, ft)), (0, 2)):
        u0, u1 = np_sgm._interval(p1)
        v0, v1 = np_sgm._interval(p2)
        u, uu0, uu1 = (a[:, D + m:W + m] for a in (p1, u0, u1))
        for d in range(D):
            v, vv0, vv1 = (a[:, D - d:W - d] for a in (p2, v0, v1))
            c0 = np.maximum(0, np.maximum(u - vv1, vv0 - u))
            c1 = np.maximum(0, np.maximum(v - uu1, uu0 - v))
            pix[:, :, d] += np.minimum(c0, c1) >> shift
    pad = np.pad(pix, ((half, half), (half, half), (0, 0)), mode="edge")
    C = np.full((H, W1, D), P2, np.int32)
    for j in range(2 * half + 1):
        for i in range(2 * half + 1):
            C += pad[j:j + H, i:i + W1]
    return C


def place(rel, m):
    """relative disparities [H][W] (column x1 + 64, -16 invalid) -> the raw image of the contract"""
    H, W = rel.shape
    out = np.full((H, W), invalid(m), np.int32)
    out[:, D + m:W + m] = rel[:, D:] + 16 * m
    return out.astype(np.int16)


def raw(L, R, m=0, mode=0, P1=600, P2=2400, ft=15, uniq=10, d12=1):
    C = cost_volume(L, R, m, P2, ft)
    S = np_sgm.aggregate(C, P1, P2, np_sgm.DIRS8 if mode == 1 else np_sgm.DIRS5)
    return place(np_sgm.wta(S, L.shape[1], D, uniq, d12), m)


def finish(raw16, m, oracle, speckle_window=100, speckle_range=32):
    out = oracle.median3x3(raw16)
    if speckle_window > 0:
        out = oracle.filter_speckles(out, invalid(m), speckle_window, 16 * speckle_range)
    return out


def compute(L, R, m, oracle, mode=0, speckle_window=100, speckle_range=32):
    return finish(raw(L, R, m, mode), m, oracle, speckle_window, speckle_range)


# ---- identity (b): the contract through the C oracle, for m in [-62, -1] ----
def band_left(L, m, ft=15):
    """columns [W + m - 2, W + m + 1] of the left image set to ftzero: the shifted image's border columns then carry
    what OpenCV's border rule gives them (raw = gradient = ftzero), and so do their neighbours' intervals"""
    W = L.shape[1]
    out = L.copy()
    out[:, max(W + m - 2, 0):min(W + m + 2, W)] = ft
    return out


def shift_left(L, m):
    """L'(x) = L(x + m): the window [m, m + 64) on (L, R) is the window [0, 64) on (L', R); columns < -m repeat column 0"""
    W = L.shape[1]
    return np.ascontiguousarray(L[:, np.clip(np.arange(W) + m, 0, W - 1)])


def from_oracle(fn, L, R, m, **kw):
    """fn = oracle.sgbm_raw on the shifted pair, its columns [64, W) re-placed at [64 + m, W + m) with 16 m added (its -16 becomes
    16 (m - 1)), every other column invalid: the raw image of the contract.  L carries the band (band_left) where the identity is
    meant to hold exactly"""
    H, W = L.shape
    got = fn(shift_left(L, m), R, **kw).astype(np.int32)
    out = np.full((H, W), invalid(m), np.int32)
    out[:, D + m:W + m] = got[:, D:] + 16 * m
    return out.astype(np.int16)


def window_pair(W, H, seed, m):
    """conftest.textured_pair (disparities 2 .. 40) with the left view moved so that most of its disparities fall inside
    [m, m + 64): L(x) = L0(x + s), s = min(-m, 50), i.e. d = d0 - s"""
    from conftest import textured_pair
    s = min(-m, 50)
    L0, R0 = textured_pair(W + 64, H, seed=seed)
    return np.ascontiguousarray(L0[:, s:s + W]), np.ascontiguousarray(R0[:, :W])


# ---- scene of case (c): background behind the screen at -20, one object in front at +6 ----
def behind_screen_pair(W=208, H=14, bg=-20, fg=6, seed=5):
    """(L, R, truth): R is a smooth random texture, L(x) = R(x - d) with d = bg, and d = fg inside an object; the border
    columns are fed from a texture wider than the image (no wrap-around)"""
    rng = np.random.default_rng(seed)
    pad = 96
    wide = rng.integers(0, 256, (H + 2, W + 2 * pad + 2)).astype(np.float64)
    wide = (wide[:-2] + wide[1:-1] + wide[2:]) / 3
    wide = (wide[:, :-2] + wide[:, 1:-1] + wide[:, 2:]) / 3
    tex = np.clip((wide - 128) * 2.2 + 128, 0, 255).astype(np.uint8)      # [H][W + 2 pad]
    R = tex[:, pad:pad + W].copy()
    truth = np.full((H, W), bg, np.int32)
    x0, x1 = W // 2 - 20, W // 2 + 20
    truth[2:H - 2, x0:x1] = fg
    obj = rng.integers(0, 256, (H, W + 2 * pad)).astype(np.uint8)          # the object has its own texture
    L = np.empty_like(R)
    xs = np.arange(W)
    for y in range(H):
        L[y] = tex[y, pad + xs - truth[y]]
    Lobj = np.zeros_like(L)
    for y in range(H):
        Lobj[y] = obj[y, pad + xs]
    m_obj = truth == fg
    L[m_obj] = Lobj[m_obj]
    # the object as the right eye sees it: shifted by fg
    for y in range(2, H - 2):
        R[y, x0 - fg:x1 - fg] = Lobj[y, x0:x1]
    return L, R, truth


def share_within_one(disp16, truth, m):
    """share of ALL pixels whose disparity is valid and within one pixel of the truth"""
    ok = (disp16 != invalid(m)) & (np.abs(disp16.astype(np.float64) / 16 - truth) <= 1)
    return ok.mean()
