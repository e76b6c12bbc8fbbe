"""Float64 reference of the correlation lookup (csrc/v3d_corr.hip) and the interval its float32 outputs must lie in.

Inputs are channel-last, as the kernels read them: fl, fr [h, w, C] holding bf16 values (as any float array), flow [2, h, w]
float32.  interval() returns, per output element [G*9, rows, w], an interval [lo, hi] that the kernel's output must lie in.
Plane order is g*9 + k; pattern 0 is the 1x9 window (dx = k - 4, dy = 0), pattern 1 the 3x3 window (dx = k % 3 - 1,
dy = k // 3 - 1); window positions are clamped into the image (replicate).  Nothing here is shared with oracle/.

Write u = 2^-24 (float32) and u64 = 2^-53 (float64).

Coordinates and weights
-----------------------
They are part of the operation's definition, and all three kernels (k_corr_warp, k_corr_gather, k_corr_fused0) compute them
the same way in float32, which NumPy float32 arithmetic reproduces bit for bit (weights()):
    sx = f32(x' + flow_x[y', x']),  sy = f32(y' + flow_y[y', x'])       with (x', y') the clamped window position,
    wx = f32(sx - floor(sx)),  wy likewise                               (exact, except for some sx in (-1/2, 0)),
    w_t = f32(a_t * b_t) with a = (1 - wx | wx), b = (1 - wy | wy)       taps t = (y0,x0) (y0,x1) (y1,x0) (y1,x1),
and a tap outside the image has weight 0.

Blend and its admissible bf16 values
------------------------------------
Per channel c of a warped position the kernels form the float32 sum of the in-image products fr_t,c * w_t in tap order and
round it once to bf16 (round to nearest even).  Each product is exact in float64 (8 x 24 significant bits), so
    v64 = sum_t fr_t * w_t   (float64, three roundings of at most u64 * sum|p| each),
and the kernel's float32 blend (four product roundings and three additions without FMA, four roundings with it) lies within
    delta = 8 u * sum_t |fr_t * w_t|
of v64; 8 u covers the kernel's at most 7 u (plus O(u^2)) and the float64 roundings of v64.  delta = 0 where nothing rounds:
every product and every partial sum in tap order is a float32 (partial sums are checked exactly, by TwoSum).  The float32 blend
is a float32 in [v64 - delta, v64 + delta], so in [f32_up(v64 - delta), f32_down(v64 + delta)], and rounding to bf16 is
monotonic: the warped value B lies in
    [Blo, Bhi] = [bf16(f32_up(v64 - delta)), bf16(f32_down(v64 + delta))].
For almost every value Blo = Bhi; an output whose window position has a channel with Blo != Bhi is "ambiguous".

Output interval
---------------
out = (sum_c fl_c * B_c) / 64 over the 64 channels of the group.  The bf16 x bf16 products are exact in float32; the MFMA
sums them in an order the documentation does not give, so no order is assumed: 64 roundings (the accumulator starts at 0), each
of at most u times a partial sum, which is at most A = sum_c |fl_c| max(|Blo_c|, |Bhi_c|).  The scale by 1/64 is exact.  With
Smin, Smax the extreme values of sum_c fl_c B_c over the admissible B (per channel the smaller / larger of fl_c Blo_c and
fl_c Bhi_c),
    out in [Smin / 64 - E, Smax / 64 + E],    E = (gamma_64 + 128 u64) A / 64,    gamma_n = n u / (1 - n u),
where 128 u64 A covers the float64 sums that form Smin, Smax and A here.  E is ~u A: one float32 ulp of the typical output.
Where every B is 0 (all four taps of the position outside) the interval is exactly [0, 0].

The fp32 C oracle (oracle.corr_lookup, channel-first) is the same operation with the bf16 step left out and a different
rounding pattern: interval(..., bf16_step=False, sum_roundings=128) models it -- the warped value is any float32 within delta of v64
(its per-tap fr * wx * wy rounds twice instead of once against the float32 weight: within 8 u too), and its sequential
float32 sum rounds every product as well as every partial sum (128 roundings).
"""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(n, u=U):
    return n * u / (1.0 - n * u)


# ------------------------------------------------------------------ float32 / bf16 rounding helpers

def bf16(x):
    """float32 -> bf16 (round to nearest, ties to even), returned as float32 values; finite inputs"""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def f32_up(x):
    """the smallest float32 >= x (float64 input)"""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def f32_down(x):
    """the largest float32 <= x (float64 input)"""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def two_sum(a, b):
    """s = fl64(a + b) and the exact error e = (a + b) - s"""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def is_f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64) == x


# ------------------------------------------------------------------ the operation

def window(pattern, k):
    """(dy, dx) of plane k"""
    return (0, k - 4) if pattern == 0 else (k // 3 - 1, k % 3 - 1)


def weights(flow):
    """float32 tap coordinates and weights of every pixel, computed as the kernels do: (ix, iy) int64 [h, w] of tap (y0,x0),
    w float32 [4, h, w] in tap order with zeros outside the image"""
    flow = np.asarray(flow, np.float32)
    _, h, w = flow.shape
    one = np.float32(1.0)
    sx = np.arange(w, dtype=np.float32)[None, :] + flow[0]
    sy = np.arange(h, dtype=np.float32)[:, None] + flow[1]
    fx, fy = np.floor(sx), np.floor(sy)
    with np.errstate(invalid="ignore"):                    # inf - inf: such a position has no tap inside the image anyway
        wx, wy = sx - fx, sy - fy
    # a tap whose coordinate is not inside the plane contributes 0, and a NaN, an infinity or a value no integer holds is not
    # inside: decided on the floats, so that only coordinates near the image are ever converted ((-2, -2) has all taps outside)
    near = (fx >= -1) & (fx <= w) & (fy >= -1) & (fy <= h)
    ix, iy = np.where(near, fx, -2).astype(np.int64), np.where(near, fy, -2).astype(np.int64)
    wt = np.stack([(one - wx) * (one - wy), wx * (one - wy), (one - wx) * wy, wx * wy])
    for t in range(4):
        xx, yy = ix + (t & 1), iy + (t >> 1)
        wt[t][(xx < 0) | (xx >= w) | (yy < 0) | (yy >= h)] = 0
    return ix, iy, wt


def blend(fr, flow, rows=None, ix_iy_wt=None):
    """v64, delta, exact [len(rows), w, C]: the float64 blend of every channel of the warped rows, its bound and whether
    nothing rounds in float32 (delta is already 0 there)"""
    fr = np.asarray(fr, np.float64)
    h, w, C = fr.shape
    rows = np.arange(h) if rows is None else np.asarray(rows)
    ix, iy, wt = ix_iy_wt if ix_iy_wt is not None else weights(flow)
    ix, iy, wt = ix[rows], iy[rows], wt[:, rows].astype(np.float64)
    s = np.zeros((len(rows), w, C))
    mag = np.zeros_like(s)
    exact = np.ones(s.shape, bool)
    for t in range(4):
        xx = np.clip(ix + (t & 1), 0, w - 1)
        yy = np.clip(iy + (t >> 1), 0, h - 1)
        p = fr[yy, xx] * wt[t][..., None]               # exact; zero outside the image
        s, e = two_sum(s, p)
        exact &= is_f32(p) & (e == 0) & is_f32(s)
        mag += np.abs(p)
    delta = np.where(exact, 0.0, 8 * U * mag)
    return s, delta, exact


def warped(fr, flow, rows=None, bf16_step=True, ix_iy_wt=None):
    """admissible warped values [Blo, Bhi] (float64) of the given rows, all columns and channels"""
    v, d, _ = blend(fr, flow, rows, ix_iy_wt)
    lo, hi = f32_up(v - d), f32_down(v + d)
    if bf16_step:
        lo, hi = bf16(lo), bf16(hi)
    return lo.astype(np.float64), hi.astype(np.float64)


def interval(fl, fr, flow, G, pattern, rows=None, bf16_step=True, sum_roundings=64, chunk=16):
    """(lo, hi, amb, zero) [G*9, len(rows), w]: the interval each output must lie in (module docstring), whether the window
    position has an ambiguous warped value, and whether every warped value there is exactly 0"""
    fl = np.asarray(fl, np.float64)
    h, w, C = fl.shape
    assert C == 64 * G and np.asarray(fr).shape == (h, w, C)
    rows = np.arange(h) if rows is None else np.asarray(rows)
    n = len(rows)
    lo, hi = np.empty((G * 9, n, w)), np.empty((G * 9, n, w))
    amb, zero = np.empty((G * 9, n, w), bool), np.empty((G * 9, n, w), bool)
    geo = weights(flow)
    e = (gamma(sum_roundings) + 128 * U64) / 64
    xs = np.arange(w)
    for c0 in range(0, n, chunk):
        rr = rows[c0:c0 + chunk]
        need = np.unique(np.clip(np.concatenate([rr + d for d in ((0,) if pattern == 0 else (-1, 0, 1))]), 0, h - 1))
        Blo, Bhi = warped(fr, flow, need, bf16_step, geo)
        where = {int(r): i for i, r in enumerate(need)}
        a = fl[rr]                                                         # [m, w, C]
        for k in range(9):
            dy, dx = window(pattern, k)
            yi = np.array([where[int(np.clip(r + dy, 0, h - 1))] for r in rr])
            xi = np.clip(xs + dx, 0, w - 1)
            bl, bh = Blo[yi][:, xi], Bhi[yi][:, xi]
            pl, ph = a * bl, a * bh
            smin = np.minimum(pl, ph).reshape(len(rr), w, G, 64).sum(-1)
            smax = np.maximum(pl, ph).reshape(len(rr), w, G, 64).sum(-1)
            A = (np.abs(a) * np.maximum(np.abs(bl), np.abs(bh))).reshape(len(rr), w, G, 64).sum(-1)
            am = (bl != bh).reshape(len(rr), w, G, 64).any(-1)
            z = ((bl == 0) & (bh == 0)).reshape(len(rr), w, G, 64).all(-1)
            for g in range(G):
                lo[g * 9 + k, c0:c0 + len(rr)] = smin[..., g] / 64 - e * A[..., g]
                hi[g * 9 + k, c0:c0 + len(rr)] = smax[..., g] / 64 + e * A[..., g]
                amb[g * 9 + k, c0:c0 + len(rr)] = am[..., g]
                zero[g * 9 + k, c0:c0 + len(rr)] = z[..., g]
    return lo, hi, amb, zero


# ------------------------------------------------------------------ test inputs

FLOWS = ("random", "integer", "half", "large", "edge", "tiny_neg", "neg_frac", "outside", "mixed")
_BORDER = ("edge", "tiny_neg", "neg_frac", "outside")


def _coords(kind, pos, extent, rng):
    """target sample coordinates of class `kind` for pixels at `pos` (float64) along an axis of `extent` pixels"""
    n = pos.shape
    if kind == "random":
        return pos + rng.uniform(-4, 4, n)
    if kind == "integer":
        return pos + rng.integers(-4, 5, n)
    if kind == "half":
        return pos + rng.integers(-4, 5, n) + 0.5 * rng.integers(0, 2, n)
    if kind == "large":                                     # |flow| log-uniform in [1, 1e4]
        return pos + rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(0, np.log(1e4), n))
    if kind == "edge":                                      # the last row / column: the second tap is outside
        return np.full(n, extent - 1.0)
    if kind == "tiny_neg":                                  # the first tap is outside, the second weighs 1 - 2^-20
        return np.full(n, -2.0 ** -20)
    if kind == "neg_frac":
        return -rng.uniform(2.0 ** -24, 1, n)
    if kind == "outside":                                   # all four taps outside, exact -1 and extent included
        c = rng.integers(0, 4, n)
        return np.select([c == 0, c == 1, c == 2], [-1.0 - rng.uniform(0, 3, n), extent + rng.uniform(0, 3, n),
                                                    np.full(n, -1.0)], np.full(n, float(extent)))
    raise ValueError(kind)


def flow_field(kind, h, w, rng):
    """float32 flow [2, h, w] whose sample coordinates x' + flow_x, y' + flow_y are of class `kind` (FLOWS): border classes
    hit x, y or both (the other coordinate random +-4); "mixed" draws the class of each coordinate of each pixel.  The target
    coordinate is exact where it is representable next to x' (the float32 sum x' + flow rounds for large x')"""
    X = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    Y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    if kind == "mixed":
        kinds = FLOWS[:-1]
        cx, cy = rng.integers(0, len(kinds), (h, w)), rng.integers(0, len(kinds), (h, w))
        tx, ty = X + rng.uniform(-4, 4, (h, w)), Y + rng.uniform(-4, 4, (h, w))
        for i, k in enumerate(kinds):
            tx = np.where(cx == i, _coords(k, X, w, rng), tx)
            ty = np.where(cy == i, _coords(k, Y, h, rng), ty)
    elif kind in _BORDER:
        mode = rng.integers(0, 3, (h, w))                   # 0: x, 1: y, 2: both
        tx = np.where(mode != 1, _coords(kind, X, w, rng), X + rng.uniform(-4, 4, (h, w)))
        ty = np.where(mode != 0, _coords(kind, Y, h, rng), Y + rng.uniform(-4, 4, (h, w)))
    else:
        tx, ty = _coords(kind, X, w, rng), _coords(kind, Y, h, rng)
    return np.stack([tx - X, ty - Y]).astype(np.float32)


def features(kind, shape, rng):
    """bf16 values as float32: "normal" N(0, 1), "spread" random sign and magnitude 2^U(-20, 20) (blends of very different
    magnitudes, sums that cancel)"""
    if kind == "normal":
        x = rng.normal(0, 1, shape)
    elif kind == "spread":
        x = rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.uniform(-20, 20, shape)
    else:
        raise ValueError(kind)
    return bf16(x.astype(np.float32))


# ------------------------------------------------------------------ checking

def ratio(got, lo, hi):
    """|got - mid| / half-width per element (0 where the interval is a point and got equals it, inf where it does not)"""
    got = np.asarray(got, np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    err = np.abs(got - mid)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(half > 0, err / np.where(half > 0, half, 1), np.where(err == 0, 0.0, np.inf))


def check(got, lo, hi, amb, what=""):
    """assert lo <= got <= hi everywhere; returns the worst |got - mid| / half-width over outputs without and with an
    ambiguous warped value"""
    got = np.asarray(got, np.float64)
    assert got.shape == lo.shape, f"{what}: shape {got.shape} vs {lo.shape}"
    bad = ~((got >= lo) & (got <= hi))
    q = ratio(got, lo, hi)
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} outputs outside the interval, first at (plane, row, x) = "
                             f"{k}: got {got[k]!r}, allowed [{lo[k]!r}, {hi[k]!r}] (err/half-width {q[k]:.4g}, "
                             f"ambiguous {bool(amb[k])})")
    w0 = float(q[~amb].max()) if (~amb).any() else 0.0
    w1 = float(q[amb].max()) if amb.any() else 0.0
    return w0, w1
