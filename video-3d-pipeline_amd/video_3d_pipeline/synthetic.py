"""Deterministic synthetic stereo input (SURVEY.md section 8d recipe).

There is no network for datasets, so tests, smoke() and bench.py all draw frames from here:
a blurred random texture viewed through a piecewise-planar disparity field (three
fronto-parallel rectangles at d = 12, 28, 44 over a 4 -> 20 ramp), squeezed into a
side-by-side BGR frame the way a 3D blu-ray stores it, plus a matching 2x guide frame.
"""
import numpy as np


def _blur(img, sigma):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(img.astype(np.float32), sigma=(sigma, sigma, 0) if img.ndim == 3 else sigma)


def gt_disparity(W, H):
    """ground-truth disparity d*(x, y) in [1, 62], float32 HxW"""
    x = np.arange(W, dtype=np.float32)[None, :]
    d = np.broadcast_to(4.0 + 16.0 * x / max(W - 1, 1), (H, W)).copy()
    for (fx0, fx1, fy0, fy1, dv) in ((0.10, 0.35, 0.15, 0.55, 12.0), (0.40, 0.70, 0.30, 0.80, 28.0),
                                     (0.72, 0.92, 0.10, 0.45, 44.0)):
        d[int(fy0 * H):int(fy1 * H), int(fx0 * W):int(fx1 * W)] = dv
    return d


_pair_cache = {}


def stereo_pair(W, H, frame_idx=0, margin=64):
    """full-width BGR left/right views (HxWx3 u8) with L(x) ~ R(x - d*) (read-only: the last few pairs are memoised,
    sbs_frame and guide_frame of one index share the texture synthesis)"""
    key = (W, H, frame_idx, margin)
    hit = _pair_cache.get(key)
    if hit is None:
        hit = _stereo_pair(W, H, frame_idx, margin)
        for a in hit:
            a.setflags(write=False)
        if len(_pair_cache) >= 4:
            _pair_cache.pop(next(iter(_pair_cache)), None)
        _pair_cache[key] = hit
    return hit


def _stereo_pair(W, H, frame_idx, margin):
    rng = np.random.default_rng(1234 + frame_idx)
    T = _blur(rng.integers(0, 256, (H, W + 2 * margin, 3)), 1.5)
    T = np.clip((T - 127.5) * 2.5 + 127.5, 0, 255)           # restore contrast lost to the blur
    left = T[:, margin:margin + W]
    d = gt_disparity(W, H)
    xs = np.arange(W, dtype=np.float32)[None, :] + d + margin  # R(x) = T(x + d)
    x0 = np.floor(xs).astype(np.int64)
    w = (xs - x0)[..., None]
    x0 = np.clip(x0, 0, T.shape[1] - 2)
    rows = np.arange(H)[:, None]
    right = T[rows, x0] * (1 - w) + T[rows, x0 + 1] * w
    return np.rint(left).astype(np.uint8), np.rint(right).astype(np.uint8)


def sbs_frame(W, H, frame_idx=0):
    """side-by-side BGR frame HxWx3 u8: each eye squeezed to W/2 by 2:1 area averaging"""
    assert W % 2 == 0
    left, right = stereo_pair(W, H, frame_idx)

    def squeeze(a):
        a = a.astype(np.uint16)
        return ((a[:, 0::2] + a[:, 1::2] + 1) >> 1).astype(np.uint8)

    return np.ascontiguousarray(np.hstack([squeeze(left), squeeze(right)]))


def tb_frame(W, H, frame_idx=0):
    """top-bottom BGR frame HxWx3 u8, the left eye on top: each eye squeezed to H/2 by 2:1 area averaging of row pairs
    (sbs_frame's counterpart for --input-layout tb)"""
    assert H % 2 == 0
    left, right = stereo_pair(W, H, frame_idx)

    def squeeze(a):
        a = a.astype(np.uint16)
        return ((a[0::2] + a[1::2] + 1) >> 1).astype(np.uint8)

    return np.ascontiguousarray(np.vstack([squeeze(left), squeeze(right)]))


def guide_frame(W, H, frame_idx=0, scale=2):
    """2x 'original 4K' luma guide (scale*H x scale*W u8) of the left view, + N(0,2) noise"""
    left, _ = stereo_pair(W, H, frame_idx)
    luma = (left[..., 2].astype(np.float32) * 0.299 + left[..., 1] * 0.587 + left[..., 0] * 0.114)
    from scipy.ndimage import zoom
    g = zoom(luma, scale, order=3, mode="nearest", grid_mode=True)
    rng = np.random.default_rng(99991 + frame_idx)
    g = g + rng.normal(0.0, 2.0, g.shape)
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


def gray_pair(W, H, frame_idx=0):
    """full-width gray left/right u8 (no SBS squeeze) -- the direct StereoSGBM input"""
    left, right = stereo_pair(W, H, frame_idx)

    def gray(a):
        return ((a[..., 2].astype(np.int32) * 9798 + a[..., 1].astype(np.int32) * 19235
                 + a[..., 0].astype(np.int32) * 3735 + (1 << 14)) >> 15).astype(np.uint8)

    return gray(left), gray(right)


# ---- a temporally coherent clip (temporal stabilisation: tests, tools/temporal_rate.py) ----
# The frames above draw a new texture per index, which is right for per-frame work and useless for anything that compares
# neighbouring frames.  Here a scene (seed) fixes the background texture and its disparity ramp; a textured rectangle at
# d = 40 moves `speed` pixels per frame over it; every frame and eye gets fresh N(0, sigma) sensor noise.

TEMPORAL_OBJECT_DISPARITY = 40.0


def _gray_texture(rng, h, w, sigma=1.5, gain=2.5):
    t = _blur(rng.integers(0, 256, (h, w)), sigma)
    return np.clip((t - 127.5) * gain + 127.5, 0, 255)


def temporal_object_box(W, H, t, speed=6):
    """(x0, y0, x1, y1) of the moving rectangle in the left view of frame t (half-open)"""
    ow, oh = max(W * 3 // 20, 4), max(H * 2 // 5, 4)
    x0, y0 = W * 3 // 10 + int(speed) * t, H * 3 // 10
    return x0, y0, x0 + ow, y0 + oh


def temporal_gt_disparity(W, H, t, scene_seed=0, speed=6):
    """ground-truth disparity of the left view of frame t, float32 HxW: the scene's ramp, the rectangle at 40"""
    a = 4.0 + 2.0 * (scene_seed % 3)
    x = np.arange(W, dtype=np.float64)[None, :]
    d = np.broadcast_to(a + 16.0 * x / max(W - 1, 1), (H, W)).astype(np.float32).copy()
    x0, y0, x1, y1 = temporal_object_box(W, H, t, speed)
    d[max(y0, 0):min(y1, H), max(x0, 0):min(x1, W)] = TEMPORAL_OBJECT_DISPARITY
    return d


def temporal_gray_pair(W, H, t, scene_seed=0, speed=6, sigma=3.0, noise_seed=0, margin=64):
    """full-width gray left / right views (HxW u8) of frame t of scene `scene_seed`"""
    rng = np.random.default_rng(777000 + scene_seed)
    bg = _gray_texture(rng, H, W + 2 * margin)
    x0, y0, x1, y1 = temporal_object_box(W, H, t, speed)
    obj = _gray_texture(rng, y1 - y0, x1 - x0, sigma=1.0, gain=3.0)
    left_full = bg.copy()                                            # the left view with its margins, object pasted in
    ya, yb, xa, xb = max(y0, 0), min(y1, H), max(x0 + margin, 0), min(x1 + margin, W + 2 * margin)
    if yb > ya and xb > xa:
        left_full[ya:yb, xa:xb] = obj[ya - y0:yb - y0, xa - x0 - margin:xb - x0 - margin]
    left = left_full[:, margin:margin + W]
    # right view: pixel x shows the left view's x + d.  Background: x_l = x_r + a + s x_l  =>  x_l = (x_r + a) / (1 - s);
    # the rectangle sits 40 px to the left of its left-view position and hides the background there
    a, s = 4.0 + 2.0 * (scene_seed % 3), 16.0 / max(W - 1, 1)
    xr = np.arange(W, dtype=np.float64)
    r = np.arange(H)[:, None]

    def sample(img, src):
        src = np.clip(src + margin, 0, W + 2 * margin - 1.001)
        i0 = np.floor(src).astype(np.int64)
        w = src - i0
        return img[r, i0] * (1 - w) + img[r, i0 + 1] * w

    right = sample(bg, np.broadcast_to((xr + a) / (1.0 - s), (H, W)))          # the background alone, also where the left view hides it
    ox = xr + TEMPORAL_OBJECT_DISPARITY
    in_obj = np.zeros((H, W), bool)
    in_obj[max(y0, 0):min(y1, H)] = ((ox >= x0) & (ox < x1))[None, :]
    right = np.where(in_obj, sample(left_full, np.broadcast_to(ox, (H, W))), right)
    nrng = np.random.default_rng([888000 + scene_seed, t, noise_seed])
    left = left + nrng.normal(0.0, sigma, left.shape)
    right = right + nrng.normal(0.0, sigma, right.shape)
    return np.clip(np.rint(left), 0, 255).astype(np.uint8), np.clip(np.rint(right), 0, 255).astype(np.uint8)


def temporal_clip(W, H, n_frames, scene_seed=0, speed=6, sigma=3.0, cut_at=None, noise_seed=0):
    """n_frames of one scene, or, with cut_at, of scene `scene_seed` up to frame cut_at - 1 and of scene `scene_seed + 1` from
    frame cut_at on (the object keeps moving) -> (left u8 [n,H,W], right u8 [n,H,W], ground-truth disparity f32 [n,H,W])"""
    L, R, G = [], [], []
    for t in range(n_frames):
        seed = scene_seed + (1 if cut_at is not None and t >= cut_at else 0)
        l, r = temporal_gray_pair(W, H, t, seed, speed, sigma, noise_seed)
        L.append(l)
        R.append(r)
        G.append(temporal_gt_disparity(W, H, t, seed, speed))
    return np.stack(L), np.stack(R), np.stack(G)


def temporal_sbs_clip(W, H, n_frames, **kw):
    """the same clip as side-by-side BGR frames [n,H,W,3] u8 (each eye squeezed to W/2, gray in all three channels)"""
    assert W % 2 == 0
    L, R, _ = temporal_clip(W, H, n_frames, **kw)

    def squeeze(a):
        a = a.astype(np.uint16)
        return ((a[..., 0::2] + a[..., 1::2] + 1) >> 1).astype(np.uint8)

    sbs = np.concatenate([squeeze(L), squeeze(R)], axis=2)
    return np.ascontiguousarray(np.repeat(sbs[..., None], 3, axis=3))


def temporal_pan_clip(W, H, n_frames, pan, **kw):
    """temporal_clip under a camera pan of `pan` pixels per frame: the clip at width W + |pan| (n_frames - 1) with both eyes
    and the ground truth cropped to W columns at offset pan * t (from the right end backward for a negative pan), so the whole
    scene moves by -pan pixels per frame while its disparity stays what it was"""
    pan, span = int(pan), abs(int(pan)) * (n_frames - 1)
    L, R, G = temporal_clip(W + span, H, n_frames, **kw)
    off = [pan * t if pan >= 0 else span + pan * t for t in range(n_frames)]

    def crop(a):
        return np.stack([a[t][:, off[t]:off[t] + W] for t in range(n_frames)])

    return crop(L), crop(R), crop(G)


def temporal_pan_sbs_clip(W, H, n_frames, pan, **kw):
    """temporal_pan_clip as side-by-side BGR frames [n,H,W,3] u8, squeezed like temporal_sbs_clip"""
    assert W % 2 == 0
    L, R, _ = temporal_pan_clip(W, H, n_frames, pan, **kw)

    def squeeze(a):
        a = a.astype(np.uint16)
        return ((a[..., 0::2] + a[..., 1::2] + 1) >> 1).astype(np.uint8)

    sbs = np.concatenate([squeeze(L), squeeze(R)], axis=2)
    return np.ascontiguousarray(np.repeat(sbs[..., None], 3, axis=3))


# ---- a left eye and a "4K" frame of one scene in different framings (spatial registration: register.py, its tests) ----
# The scene is a piecewise-constant master over the eye's normalised coordinates sigma in [-1/2, 3/2] on both axes, REG_SUPER master
# pixels per eye pixel.  Both planes are exact area averages of it in float64: eye pixel x covers sigma in [x, x + 1) / We, guide
# pixel X covers xi in [X, X + 1) / Wg and with it sigma = A xi + B.  The guide is graded differently (gain, offset, noise).
REG_SUPER = 4


def _area_means(M, edges, axis):
    """means of the piecewise-constant M between consecutive `edges` (master pixel units, float64) along `axis`"""
    c = np.concatenate([np.zeros_like(np.take(M, [0], axis)), np.cumsum(M, axis=axis)], axis=axis)
    i = np.clip(np.floor(edges).astype(np.int64), 0, M.shape[axis] - 1)
    at = np.take(c, i, axis) + np.take(M, i, axis) * np.expand_dims(edges - i, tuple(k for k in range(M.ndim) if k != axis))
    w = np.expand_dims(np.diff(edges), tuple(k for k in range(M.ndim) if k != axis))
    return np.diff(at, axis=axis) / w


def registered_pair(eye_size, guide_size, amap, index=0, bars=False):
    """(left-eye gray u8 [He,We], guide gray u8 [Hg,Wg]) of scene `index`, related by amap = (Ax, Bx, Ay, By); bars: the eye is
    black outside the picture the guide shows (a letterboxed or pillarboxed disc)"""
    (We, He), (Wg, Hg), (Ax, Bx, Ay, By) = eye_size, guide_size, amap
    rng = np.random.default_rng(4321 + index)
    S = REG_SUPER
    hm, wm = 2 * He * S, 2 * We * S
    M = 0.55 * _gray_texture(rng, hm, wm, sigma=1.5 * S) + 0.45 * _gray_texture(rng, hm, wm, sigma=6.0 * S, gain=12.0)
    M = M.astype(np.float64)

    def plane(n_x, n_y, ax, bx, ay, by):
        ex = ((ax * np.arange(n_x + 1) / n_x + bx) + 0.5) * We * S
        ey = ((ay * np.arange(n_y + 1) / n_y + by) + 0.5) * He * S
        return _area_means(_area_means(M, ey, 0), ex, 1)

    eye = plane(We, He, 1.0, 0.0, 1.0, 0.0)
    if bars:
        sx, sy = (np.arange(We) + 0.5) / We, (np.arange(He) + 0.5) / He
        eye[(sy < By) | (sy > Ay + By), :] = 0.0
        eye[:, (sx < Bx) | (sx > Ax + Bx)] = 0.0
    guide = plane(Wg, Hg, Ax, Bx, Ay, By) * 0.9 + 8.0 + rng.normal(0.0, 1.0, (Hg, Wg))
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to_u8(eye), to_u8(guide)
