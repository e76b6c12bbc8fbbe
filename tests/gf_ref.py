"""Float64 reference of the guided-filter upscaler and the error bound its float32 / u16 outputs must meet.

Every route of csrc/v3d_guided.hip forms the window sums, a, b and the stage-2 algebra in float64 and rounds once, to float32
(or to the u16 sample through that float32).  So a float32 output q must satisfy

    |q - want| <= ulp32(want) + F

where want is the oracle (oracle.guided_upscale, float64) and F bounds the float64 error of the kernel AND of the oracle
against the exact result.  The rounding to float32 costs half an ulp; a whole one leaves room for a result that crosses a
power of two.  F is a per-pixel absolute floor, derived below to first order in u = 2^-53.  The tests assert the sharper
form of the same statement, check_f32: q is float32(x) for some x within F of want, i.e. float32(want - F) <= q <=
float32(want + F) -- rounding to nearest is monotonic.  An extra float32 rounding anywhere in a kernel breaks it.

eps reaches the kernels as float32 (the C ABI) and is widened exactly to double there, so the reference is fed
float(np.float32(eps)): at eps = 1e-3 the double 1e-3 differs from it by 4.7e-8 relative.

Derivation of F
---------------
Notation: n = 2r + 1 (window width), P = max |p| over the frame (p is a bilinear blend of depth_lo, so P = max |depth_lo|),
I = g / 255 in [0, 1], v = var(I) over the clipped window of a pixel, c = min(H, W, r + 1) (the fewest rows or columns a
clipped window can hold).

1. A window mean m = S / cnt of a quantity x with |x| <= X.  The marching kernels keep each column's vertical sum as a
   RUNNING sum, updated per row by "+ entering - leaving" (two roundings, or two fmas), over the whole band: M steps, where
   M = gf_band + 4r for k_gff (band plus both stages' warm-up), gf_band1/2 + 2r for k_gfm and 2r + 1 + 7 for k_gf (whose
   sliding runs are eight columns / four rows).  A partial of a column that holds cy in-image rows is at most (cy + 1) X, so
   a column carries <= M (2 cy + 2) u X; a window adds cx columns and (n + 6) more roundings (the sliding runs of four or
   eight), and the sum is divided by cx * cy (reciprocal: two roundings more).  Per unit of u X:

       K(M) = 2 M (1 + 1/c) + n + 10.

   The error of a running sum is NOT local: the rounding error picked up in a large-valued region stays in the sum after the
   window has left it, so X is the maximum over the frame, never over the window.  The oracle sums each window from scratch,
   row by row and then column by column (2n roundings per term, no carry-over): K_o = 2n + 4.
   Sums of p and I*p use K_p = K(M); sums of I and I*I are exact integers on k_gff / k_gfm (then only the scaling by
   1/(255 cnt) rounds: K_I = 6) and f64 only on k_gf (K_I = K(n + 8)); the oracle's I = g/255 is rounded once more: 2n + 5.
2. cov = m(Ip) - m(I) m(p), var = m(II) - m(I)^2:
       dcov <= (2 K_p + K_I + 3) u P,          dvar <= (3 K_I + 3) u.
3. a = cov / (var + eps), with |cov| <= sqrt(v) sd(p) <= sqrt(v) S (Cauchy-Schwarz; S = half the range of p bounds its
   standard deviation) and its own rounding (reciprocal + product):
       da <= u [ (2 K_p + K_I + 3) P / (v + eps) + S (3 K_I + 3) sqrt(v) / (v + eps)^2 + 4 S sqrt(v) / (v + eps) ],
       |a| <= A = S sqrt(v) / (v + eps)   (<= S / (2 sqrt(eps))).
4. b = m(p) - a m(I):  db <= K_p u P + da + A K_I u + 2 u (P + A).
5. q = mean(a) I + mean(b).  The a and b errors of the window's pixels k enter as mean(da_k (I - m_k(I))) + mean(dm_k(p)) +
   ...: |I - m_k(I)| <= 1, so they cost at most max_window(da) + K_p u P + K_I u A + 2 u (P + A).  Stage 2's own sums are
   running sums again (X = max |a|, max |b| <= P + max |a| over the frame), and the final algebra rounds three times:
       F = max_window(da) + u [ (K_p + 2) P + (K_I + 2) A* + (K_p + 3) (2 A* + P) ],      A* = max over the frame of A.

F is evaluated once with the route's K (chains(); route None takes the largest of the three families) and once with the
oracle's, and the two are added.  At the product's eps = 1e-3 and r = 8, k_gff's M = 464 gives K_p ~ 1060: a pixel over a
flat guide (v = 0) gets F ~ 2.1e6 u P ~ 2.4e-10 P, a textured one (v ~ 0.05) ~ 1e-11 P -- both far below ulp32 of a typical q
(6e-8 .. 1.2e-7 relative).  A u16 output of want is one of clip(rint(float32(want +- F)), 0, 65535):
rounding to float32, rint and clip are monotonic.
"""
import numpy as np

U = 2.0 ** -53
GF_BAND = 432           # the fused kernel's default band (v3d_api.cpp)


def eps32(eps):
    """eps as the kernels see it: rounded to float32 at the C ABI, widened exactly to double"""
    return float(np.float32(eps))


def reference(depth_lo, guide, r, eps):
    """the float64 oracle, fed the float32 eps the kernels use"""
    from oracle import oracle as O
    return O.guided_upscale(np.asarray(depth_lo, np.float32), guide, r, eps32(eps))


def ulp32(x):
    """spacing of float32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def box_sum(x, r):
    """sum over the (2r+1)^2 window clipped at the border (exact for integer input)"""
    x = np.asarray(x)
    H, W = x.shape
    c = np.zeros((H + 1, W + 1), x.dtype)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def guide_var(guide, r):
    """var(I) over each clipped window, from exact integer sums of g and g^2"""
    g = np.asarray(guide, np.int64)
    cnt, s1, s2 = box_sum(np.ones_like(g), r), box_sum(g, r), box_sum(g * g, r)
    return np.maximum(cnt * s2 - s1 * s1, 0) / (cnt * cnt * 65025.0)


def _K(M, n, c):
    return 2.0 * M * (1.0 + 1.0 / c) + n + 10


def chains(route, r, c, band=GF_BAND, band12=270):
    """(K_p, K_I) of a route: "gff" (k_gff, M = band + 4r, integer I sums), "gfm" (k_gfm, M = max(gf_band1, gf_band2) + 2r,
    integer I sums), "gf" (k_gf, M = 2r + 1 + 8, float64 I sums); None: the largest of the three"""
    n = 2 * r + 1
    if route is None:
        return max(chains(x, r, c, band, band12)[0] for x in ("gff", "gfm", "gf")), _K(n + 8, n, c)
    M = {"gff": band + 4 * r, "gfm": band12 + 2 * r, "gf": n + 8}[route]
    return _K(M, n, c), (_K(n + 8, n, c) if route == "gf" else 6.0)


def floor(depth_lo, guide, r, eps, route=None, band=GF_BAND, parts=False):
    """per-pixel absolute floor F of the float64 error (module docstring) for a route of chains(); parts=True returns
    (kernel part, oracle part)"""
    from scipy.ndimage import maximum_filter
    H, W = np.asarray(guide).shape
    n, c, e = 2 * r + 1, min(H, W, r + 1), eps32(eps)
    d = np.asarray(depth_lo, np.float64)
    P, S = float(np.abs(d).max()), float(d.max() - d.min()) / 2          # max |p|, and sd(p) <= half the range of p
    v = guide_var(guide, r)
    s = np.sqrt(v) * (1 + 1e-12)
    den = v * (1 - 1e-12) + e
    A_star = float((S * s / den).max())

    def part(Kp, KI):
        da = U * ((2 * Kp + KI + 3) * P / den + S * ((3 * KI + 3) * s / den ** 2 + 4 * s / den))
        return maximum_filter(da, size=n, mode="nearest") + U * ((Kp + 2) * P + (KI + 2) * A_star + (Kp + 3) * (2 * A_star + P))

    kern = part(*chains(route, r, c, band))
    orc = part(2 * n + 4, 2 * n + 5)
    return (kern, orc) if parts else kern + orc


def bound(want, F):
    """|got - want| allowed for a float32 output"""
    return ulp32(want) + F


def ratio(got, want, F):
    """err / bound per pixel"""
    return np.abs(np.asarray(got, np.float64) - want) / bound(want, F)


def worst(got, want, F, what=""):
    """(max err/bound, message naming the worst pixel)"""
    q = ratio(got, want, F)
    k = np.unravel_index(int(q.argmax()), q.shape)
    got = np.asarray(got, np.float64)
    return float(q[k]), (f"{what}: max err/bound {q[k]:.3g} at {k}: got {got[k]!r} want {want[k]!r} "
                         f"err {abs(got[k] - want[k]):.3e} bound {bound(want, F)[k]:.3e} (F {F[k]:.3e})")


def f32_window(want, F):
    """the float32 values a kernel whose float64 q lies within F of want may store (round to nearest is monotonic)"""
    return (want - F).astype(np.float32), (want + F).astype(np.float32)


def check_f32(got, want, F, what=""):
    """assert that got is a float32 rounding of a value within F of want (which implies |got - want| <= ulp32 + F);
    returns the worst err / (ulp32 + F)"""
    w, msg = worst(got, want, F, what)
    lo, hi = f32_window(want, F)
    g = np.asarray(got, np.float32)
    out = (g < lo) | (g > hi)
    if out.any():
        k = tuple(np.argwhere(out)[0])
        msg += (f"; {int(out.sum())} pixels are no float32 rounding of a value within F of want, first at {k}: "
                f"got {g[k]!r}, allowed {lo[k]!r} .. {hi[k]!r}")
    assert w <= 1.0 and not out.any(), msg
    return w


def u16_window(want, F):
    """the u16 samples a kernel whose float64 q lies within F of want may store: [lo, hi]"""
    lo = np.clip(np.rint((want - F).astype(np.float32)), 0, 65535).astype(np.int64)
    hi = np.clip(np.rint((want + F).astype(np.float32)), 0, 65535).astype(np.int64)
    return lo, hi
