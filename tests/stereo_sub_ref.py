"""NumPy restatement of the sub-pixel DIBR contract (v3d_render_stereo_subpixel_batch; DESIGN.md §4, "Sub-pixel DIBR").
All integer arithmetic: the GPU must match it bit for bit.  Inputs, layouts and gains are those of tests/stereo_ref.py.

For each row y and each eye with gain g, D = depth[y] (u16), F = frame[y] (BGR u8); every floor, >> and ceil is the mathematical one:
  1. position in 1/16 px: s16(x) = floor((g * (D[x] - conv) + 2^19) / 2^20), p(x) = 16 x + s16(x) (may be negative);
  2. span of source x: L' = p(x+1) - p(x) if x + 1 < W.  Connected iff x + 1 < W and 0 < L' <= TEAR16 (stretched to at most 2 px):
     L = L', colours between F[x] and F[x+1].  Otherwise (last column, fold L' <= 0, tear L' > TEAR16) a point: L = 16, colour F[x].
     The span covers the integer targets t with p(x) <= 16 t < p(x) + L: the first is (p(x) + 15) >> 4, at most two, none for a
     compressed connected span;
  3. z-buffer: Z[t] = max over the spans that cover t, 0 <= t < W, of (D[x] << 16) | (x + 1) (u32); other targets are dropped;
  4. colour of a hit target, x = (Z[t] & 0xFFFF) - 1: F[x] for a point; for a connected span w = 16 t - p(x) and per channel
     c = floor((2 ((L - w) F[x] + w F[x+1]) + L) / (2 L)) (round-half-up linear interpolation);
  5. holes (Z[t] = 0): the nearest non-zero keys left (a) and right (b): the farther one, (Z[a] >> 16) <= (Z[b] >> 16) -> a; the
     only one if one side has none; black if the row has no key.  The hole takes the rendered colour E[a] / E[b];
  6. layout: full SBS [H][2W][3] (left eye first); half SBS [H][W][3], eye pixel x' = (E[2x'] + E[2x'+1] + 1) >> 1.

Every function also returns the counts of the case classes (COUNT_KEYS), summed over rows and eyes: the tests use them to show that
the scenes they render reach every branch of the contract.
"""
import numpy as np

from stereo_ref import FULL_SBS, HALF_SBS, stereo_gains  # noqa: F401  (the same layouts and host mapping)

TEAR16 = 32                        # V3D_STEREO_TEAR16
COUNT_KEYS = ("connected0", "connected1", "connected2", "folds", "tears", "out_of_range", "z_conflicts", "holes_left",
              "holes_right", "empty_rows")

# the division of step 4 as a multiply: floor(n / (2L)) == (n * DIV_MUL[L]) >> 20 for every n <= 16352, L <= 32
DIV_MUL = [0] + [-((-(1 << 20)) // (2 * L)) for L in range(1, TEAR16 + 1)]          # ceil(2^20 / 2L)


def _zero_counts():
    return dict.fromkeys(COUNT_KEYS, 0)


def _add(a, b):
    for k in COUNT_KEYS:
        a[k] += int(b[k])
    return a


def eye_image(frame, depth, gain, conv):
    """BGR u8 [H,W,3] + u16 depth [H,W] -> (the eye image [H,W,3] u8, the case counts)"""
    F = np.asarray(frame, np.uint8).astype(np.int64)
    D = np.asarray(depth).astype(np.int64)
    H, W = D.shape
    x = np.arange(W, dtype=np.int64)[None, :]
    p = 16 * x + ((int(gain) * (D - int(conv)) + (1 << 19)) >> 20)                   # >> on int64 is floor division
    Lp = np.zeros_like(p)
    Lp[:, :-1] = p[:, 1:] - p[:, :-1]
    inner = np.broadcast_to(x + 1 < W, p.shape)
    conn = inner & (Lp > 0) & (Lp <= TEAR16)
    L = np.where(conn, Lp, 16)
    t0 = (p + 15) >> 4
    hits = [(t0 + k, 16 * (t0 + k) < p + L) for k in (0, 1)]
    key = (D << 16) | (x + 1)
    rows = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], p.shape)
    Z = np.zeros(H * W, np.int64)
    cnt = _zero_counts()
    nhit = hits[0][1].astype(np.int64) + hits[1][1]
    for k in (0, 1, 2):
        cnt[f"connected{k}"] = int((conn & (nhit == k)).sum())
    cnt["folds"] = int((inner & (Lp <= 0)).sum())
    cnt["tears"] = int((inner & (Lp > TEAR16)).sum())
    landed = 0
    for t, hit in hits:
        keep = hit & (t >= 0) & (t < W)
        cnt["out_of_range"] += int((hit & ~keep).sum())
        landed += int(keep.sum())
        np.maximum.at(Z, (rows * W + t)[keep], key[keep])
    Z = Z.reshape(H, W)
    nz = Z != 0
    cnt["z_conflicts"] = landed - int(nz.sum())
    cnt["empty_rows"] = int((~nz.any(axis=1)).sum())

    # step 4: the colour of every hit target
    src = np.clip((Z & 0xFFFF) - 1, 0, W - 1)
    nxt = np.minimum(src + 1, W - 1)
    ps, Ls, cs = (np.take_along_axis(a, src, axis=1) for a in (p, L, conn))
    F0 = np.take_along_axis(F, src[..., None], axis=1)
    F1 = np.take_along_axis(F, nxt[..., None], axis=1)
    w = np.where(cs, 16 * x - ps, 0)[..., None]
    Ls = Ls[..., None]
    E = np.where(cs[..., None], (2 * ((Ls - w) * F0 + w * F1) + Ls) // (2 * Ls), F0)

    # step 5: holes copy the rendered colour of the neighbour the integer contract would choose
    a = np.maximum.accumulate(np.where(nz, x, -1), axis=1)
    b = np.minimum.accumulate(np.where(nz, x, W)[:, ::-1], axis=1)[:, ::-1]
    Za = np.where(a >= 0, np.take_along_axis(Z, np.clip(a, 0, W - 1), axis=1), 0)
    Zb = np.where(b < W, np.take_along_axis(Z, np.clip(b, 0, W - 1), axis=1), 0)
    left = (Za != 0) & ((Zb == 0) | ((Za >> 16) <= (Zb >> 16)))
    right = ~left & (Zb != 0)
    cnt["holes_left"] = int((~nz & left).sum())
    cnt["holes_right"] = int((~nz & right).sum())
    pick = np.clip(np.where(left, a, b), 0, W - 1)
    E = np.take_along_axis(E, pick[..., None], axis=1)
    E = np.where((left | right)[..., None], E, 0)
    return E.astype(np.uint8), cnt


def _pack(eyes, W, layout):
    if layout == HALF_SBS:
        if W % 2:
            raise ValueError("half SBS needs an even width")
        eyes = [((e[:, 0::2].astype(np.uint16) + e[:, 1::2] + 1) >> 1).astype(np.uint8) for e in eyes]
    elif layout != FULL_SBS:
        raise ValueError(f"layout {layout}")
    return np.concatenate(eyes, axis=1)


def render_counts(frame, depth, gain_left, gain_right, conv, layout=FULL_SBS):
    """one frame: BGR u8 [H,W,3], u16 depth [H,W] -> (u8 [H,2W,3] (full SBS) or [H,W,3] (half SBS), the case counts of both eyes)"""
    F = np.asarray(frame, np.uint8)
    D = np.asarray(depth, np.uint16)
    if F.shape[:2] != D.shape or F.ndim != 3 or F.shape[2] != 3:
        raise ValueError(f"frame {F.shape} and depth {D.shape} disagree")
    cnt = _zero_counts()
    eyes = []
    for g in (gain_left, gain_right):
        e, c = eye_image(F, D, g, conv)
        eyes.append(e)
        _add(cnt, c)
    return _pack(eyes, D.shape[1], layout), cnt


def render(frame, depth, gain_left, gain_right, conv, layout=FULL_SBS):
    return render_counts(frame, depth, gain_left, gain_right, conv, layout)[0]


def render_loop(frame, depth, gain_left, gain_right, conv, layout=FULL_SBS):
    """the same contract as a literal per-pixel loop (small inputs only): what the vectorised form is checked against.
    Returns (image, counts) like render_counts."""
    F = np.asarray(frame, np.uint8)
    D = np.asarray(depth, np.uint16)
    H, W = D.shape
    cnt = _zero_counts()
    out = []
    for g in (gain_left, gain_right):
        E = np.zeros((H, W, 3), np.uint8)
        for y in range(H):
            p = [16 * x + (g * (int(D[y, x]) - conv) + (1 << 19)) // (1 << 20) for x in range(W)]
            span = []                                                   # (L, connected) per source
            Z = [0] * W
            for x in range(W):
                L, connected = 16, False
                if x + 1 < W:
                    Lp = p[x + 1] - p[x]
                    if Lp <= 0:
                        cnt["folds"] += 1
                    elif Lp > TEAR16:
                        cnt["tears"] += 1
                    else:
                        L, connected = Lp, True
                span.append((L, connected))
                targets = [t for t in range(p[x] // 16 - 1, p[x] // 16 + 4) if p[x] <= 16 * t < p[x] + L]
                assert len(targets) <= 2 and (not targets or targets[0] == (p[x] + 15) >> 4)
                if connected:
                    cnt[f"connected{len(targets)}"] += 1
                for t in targets:
                    if 0 <= t < W:
                        if Z[t]:
                            cnt["z_conflicts"] += 1
                        Z[t] = max(Z[t], (int(D[y, x]) << 16) | (x + 1))
                    else:
                        cnt["out_of_range"] += 1
            if not any(Z):
                cnt["empty_rows"] += 1
            hit = np.zeros((W, 3), np.uint8)
            for t in range(W):
                if Z[t]:
                    x = (Z[t] & 0xFFFF) - 1
                    L, connected = span[x]
                    if connected:
                        w = 16 * t - p[x]
                        assert 0 <= w < L
                        for c in range(3):
                            hit[t, c] = (2 * ((L - w) * int(F[y, x, c]) + w * int(F[y, x + 1, c])) + L) // (2 * L)
                    else:
                        hit[t] = F[y, x]
            for t in range(W):
                if Z[t]:
                    E[y, t] = hit[t]
                    continue
                a = next((i for i in range(t - 1, -1, -1) if Z[i]), None)
                b = next((i for i in range(t + 1, W) if Z[i]), None)
                if a is not None and (b is None or (Z[a] >> 16) <= (Z[b] >> 16)):
                    E[y, t] = hit[a]
                    cnt["holes_left"] += 1
                elif b is not None:
                    E[y, t] = hit[b]
                    cnt["holes_right"] += 1
        if layout == HALF_SBS:
            h = np.zeros((H, W // 2, 3), np.uint8)
            for y in range(H):
                for x in range(W // 2):
                    for c in range(3):
                        h[y, x, c] = (int(E[y, 2 * x, c]) + int(E[y, 2 * x + 1, c]) + 1) >> 1
            E = h
        out.append(E)
    return np.concatenate(out, axis=1), cnt


# ------------------------------------------------------------------------------------------------------------------------
# the scenes and parameters the GPU tests render (tests/test_stereo_sub_gpu.py); tests/test_stereo_sub_ref.py shows on the CPU
# that together they reach every case class
# ------------------------------------------------------------------------------------------------------------------------
SCENES = ("noise", "planar", "steep", "shallow", "fractional")
GMAX = (1 << 24) - 1


def scene_depth(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    x = np.arange(W)[None, :]
    if kind == "noise":                                             # dense collisions, folds and tears
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    if kind == "planar":                                            # piecewise planar: ramps with steps between them
        cuts = np.sort(rng.integers(0, max(W, 1), 3))
        seg = (x >= cuts[0]).astype(int) + (x >= cuts[1]) + (x >= cuts[2])
        d = rng.integers(0, 65536, 4)[seg] + rng.integers(-400, 400, 4)[seg] * x + rng.integers(-3000, 3000, (H, 1))
        return np.clip(d, 0, 65535).astype(np.uint16)
    if kind in ("steep", "shallow"):
        # a sawtooth of 1365 levels per pixel: at the default gain (6144) a source moves 8/16 px against its neighbour, so one eye
        # sees stretched spans (L = 24, in 17..32) and the other compressed ones (L = 8 < 16); the teeth fold and tear
        slope = 1365 if kind == "steep" else -1365
        return ((slope * x + rng.integers(0, 65536, (H, 1))) % 65536).astype(np.uint16)
    if kind == "fractional":                                        # constant depth: s16 = 6144 * 5000 / 2^20 = 29.3 -> 29 = 16 + 13
        return np.full((H, W), 32768 + 5000, np.uint16)
    raise ValueError(kind)


def scene_params(W):
    """(gain_left, gain_right, conv): zero, the defaults, eye_split 0 and 1, +-255 px, shifts >= W, conv at both ends"""
    return [(0, 0, 32768), stereo_gains(), stereo_gains(48, 0.5, 0.0), stereo_gains(48, 0.5, 1.0),
            stereo_gains(510, 0.5, 0.5), stereo_gains(510, 0.0, 0.5), stereo_gains(510, 1.0, 0.5),
            (GMAX, -GMAX, 0), (-GMAX, GMAX, 65535), (W * 256 + 77, -(W * 256 + 77), 0)]
