"""GPU: every route of the guided-filter upscaler (csrc/v3d_guided.hip) against the float64 oracle at the float64 error bound.

Each route forms sums, a, b and q in float64 and rounds once, so a float32 output must lie within ulp32(want) + F of the oracle
and a u16 output must be one of clip(rint(float32(want +- F))), F being the per-pixel floor derived in tests/gf_ref.py (the
oracle is fed the float32 eps the kernels get).  That is ~1e-7 relative where the older tests allow 1e-3.

Routes (v3d_set_option): k_gff (fused, the default for r in {4, 8}; strips of 256 or -- int16 disparity at exact 2x with the
integer first stage -- 512 columns), k_gfm (gf_fused 0, two marching sweeps), k_gf (gf_tiled 1, and every other radius: LDS
tiles of 16 rows for r <= 8, 8 rows above).  Inputs: float32 depth, int16 disparity (integer or float64 first stage), the
u16 samples as float32, and the u16 route with u16 output.

Each test prints `ACC <name> <worst err/bound>`, err/bound = |q - want| / (ulp32(want) + F).  Measured on an MI355X: every float32
test's worst value lies in 0.4985 .. 0.5000 (the half ulp of the final rounding; the float64 part of the error is far inside F),
the constant-depth cases are exact (0), the affine case stays below 0.45 of its eps-derived bound, and the u16 tests see at
most 4.1e-6 ambiguous samples (4K) and no sample outside the window.

What these tests catch that the older ones did not (scratch builds, one kernel family at a time, measured on an MI355X):
eps * (1 + 1e-4) and a float32 stage 2 (mean(a) I + mean(b)) fail test_routes_and_input_types, test_geometry_edges,
test_batch_of_three_strided_guides and test_u16_samples_against_the_oracle in k_gff, k_gfm and k_gf alike, plus
test_every_radius_default_route and test_eps_range where the family is on the default route; with these two changes in
k_gfm or k_gf every older test still passes (in k_gff two benchmark-batch tests fail too).  A float32 bilinear x coordinate
shows at the non-integer scales of test_every_radius_default_route (k_gff, k_gf) and test_geometry_edges (all three; exact
2x computes it exactly in float32 too); in k_gf no older test notices it."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import gf_ref

pytestmark = pytest.mark.gpu

ROUTES = {                 # name -> options
    "gff256": {"gf_fused": 1, "gf_tiled": 0, "gf_cols": 256},
    "gff512": {"gf_fused": 1, "gf_tiled": 0, "gf_cols": 512},
    "gfm": {"gf_fused": 0, "gf_tiled": 0},
    "gf": {"gf_tiled": 1},
}
_KEYS = ("gf_fused", "gf_tiled", "gf_cols", "gf_int1", "gf_band", "gf_band1", "gf_band2")


@contextlib.contextmanager
def _options(native, **opts):
    saved = {k: native.get_option(k) for k in _KEYS}
    try:
        for k, v in opts.items():
            native.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            native.set_option(k, v)


def _family(route, r):
    """kernel family a route name runs at radius r (the fused and marching kernels exist for r in {4, 8} only)"""
    if r not in (4, 8) or route == "gf":
        return "gf"
    return "gfm" if route == "gfm" else "gff"


def _report(name, ratios):
    w = max(ratios) if ratios else 0.0
    print(f"\nACC {name} {w:.4g}")
    return w


def _depth(rng, Hlo, Wlo, scale=63.0):
    """smooth depth with steps and a sprinkling of exact zeros (invalid disparities)"""
    from scipy.ndimage import gaussian_filter
    d = gaussian_filter(rng.uniform(0, scale, (Hlo, Wlo)), 2.0)
    d[: Hlo // 3, : Wlo // 3] *= 0.25
    d[rng.random(d.shape) < 0.05] = 0.0
    return d.astype(np.float32)


def _guide(rng, H, W):
    """smooth texture clipped to 0 / 255 in places: flat patches (var = 0, where 1/eps amplifies) next to edges and texture"""
    from scipy.ndimage import gaussian_filter
    g = gaussian_filter(rng.uniform(0, 255, (H, W)), 1.5) * 3.0 - 255
    return np.clip(g, 0, 255).astype(np.uint8)


def _frames(seed, n, Wlo, Hlo, W, H):
    rng = np.random.default_rng(seed)
    return np.stack([_depth(rng, Hlo, Wlo) for _ in range(n)]), np.stack([_guide(rng, H, W) for _ in range(n)])


def _check(got, depth, guide, r, eps, what, route):
    """got: float32 frame of `route`; returns its worst err/bound and asserts it is <= 1"""
    want = gf_ref.reference(depth, guide, r, eps)
    F = gf_ref.floor(depth, guide, r, eps, _family(route, r))
    assert got.shape == want.shape
    return gf_ref.check_f32(got, want, F, what)


# ------------------------------------------------------------------ every radius on the default dispatch

GEOMS = [(131, 67, 262, 134),       # exact 2x, sizes that are multiples of neither 64, 16 nor 8
         (100, 61, 229, 151),       # non-integer scale
         (11, 4, 21, 5)]            # a guide shorter (r >= 3) and narrower (r >= 11) than the window


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", range(1, 17))
def test_every_radius_default_route(native, r):
    """r = 1..16 as the library dispatches them (k_gff for 4 and 8, k_gf<*,4> for the other r <= 8, k_gf<*,2> above)."""
    ratios = []
    for i, (Wlo, Hlo, W, H) in enumerate(GEOMS):
        d, g = _frames(100 * r + i, 1, Wlo, Hlo, W, H)
        got = native.guided_upscale(native.to_device(d[0]), native.to_device(g[0]), r, 1e-3).cpu().numpy()
        ratios.append(_check(got, d[0], g[0], r, 1e-3, f"r={r} {Wlo}x{Hlo}->{W}x{H}", "default"))
    _report(f"every_radius r={r}", ratios)


# ------------------------------------------------------------------ r in {4, 8}: every route and input type

@functools.lru_cache(maxsize=None)
def _route_data(r):
    """two frames, exact 2x of 133x71 (the integer first stage needs exact 2x): int16 disparities x16 with invalid (-16) and
    zero entries, and u16 samples over the whole range"""
    rng = np.random.default_rng(40 + r)
    disp = (_depth(rng, 71, 133, 60.0)[None].repeat(2, 0) * 16).astype(np.int16) + rng.integers(0, 16, (2, 71, 133)).astype(np.int16)
    disp[rng.random(disp.shape) < 0.05] = -16
    u16 = np.clip(disp.astype(np.int64) * 64 + rng.integers(0, 64, disp.shape), 0, 65535).astype(np.uint16)
    guide = np.stack([_guide(rng, 142, 266) for _ in range(2)])
    return disp, u16, guide


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["f32", "i16_int1", "i16_f64", "u16_as_f32"])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("r", [4, 8])
def test_routes_and_input_types(native, oracle, r, route, kind):
    """every kernel family and input type at r = 4 and 8 (gff512 differs from gff256 on the int16 integer route only)"""
    disp, u16, guide = _route_data(r)
    g = native.to_device(guide)
    if kind == "f32":
        depth = np.stack([oracle.disp_to_depth(x) for x in disp])
        src = native.to_device(depth)
    elif kind.startswith("i16"):
        depth = np.stack([oracle.disp_to_depth(x) for x in disp])
        src = native.to_device(disp)
    else:
        depth = u16.astype(np.float32)
        src = (torch.from_numpy(u16.view(np.int16)).cuda().to(torch.int32) & 0xFFFF).float().contiguous()
    with _options(native, gf_int1=0 if kind == "i16_f64" else 1, **ROUTES[route]):
        got = native.guided_upscale_batch(src, g, r, 1e-3).cpu().numpy()
    ratios = [_check(got[f], depth[f], guide[f], r, 1e-3, f"{route} {kind} r={r} frame {f}", route) for f in range(2)]
    _report(f"routes r={r} {route} {kind}", ratios)


# ------------------------------------------------------------------ geometry edges on every route

EDGES = [(1, 1, 1, 1),              # 1x1 guide
         (5, 1, 37, 1),             # one row
         (1, 6, 1, 41),             # one column
         (97, 61, 45, 29),          # downscale (Wlo > Whi)
         (53, 37, 53, 37),          # identity scale
         (120, 45, 240, 90)]        # exact 2x, run with bands that end partway through a four-row step
EDGES_2X = [(1, 1, 2, 2), (9, 1, 18, 2), (1, 7, 2, 14), (120, 45, 240, 90)]     # int16 integer route (exact 2x only)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", [4, 8])
@pytest.mark.parametrize("route", ["gff256", "gfm", "gf"])
def test_geometry_edges(native, r, route):
    """tiny and degenerate guides, down and identity scale, bands of 37 / 38 rows (k_gff / k_gfm) that end partway through a
    four-row step, on each kernel family with float32 input"""
    ratios = []
    for i, (Wlo, Hlo, W, H) in enumerate(EDGES):
        d, g = _frames(7 * i + r, 1, Wlo, Hlo, W, H)
        band = 37 if i == len(EDGES) - 1 else gf_ref.GF_BAND
        with _options(native, gf_band=band, gf_band1=37, gf_band2=38, **ROUTES[route]):
            got = native.guided_upscale(native.to_device(d[0]), native.to_device(g[0]), r, 1e-3).cpu().numpy()
        ratios.append(_check(got, d[0], g[0], r, 1e-3, f"{route} r={r} {Wlo}x{Hlo}->{W}x{H}", route))
    _report(f"edges {route} r={r}", ratios)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("cols", [256, 512])
@pytest.mark.parametrize("r", [4, 8])
def test_geometry_edges_integer_route(native, oracle, r, cols):
    """the same edges where the int16 integer first stage applies (exact 2x): 2x2, 18x2, 2x14 guides and a band of 39 rows"""
    ratios = []
    for i, (Wlo, Hlo, W, H) in enumerate(EDGES_2X):
        rng = np.random.default_rng(300 + 10 * i + r)
        disp = rng.integers(-16, 1024, (1, Hlo, Wlo)).astype(np.int16)
        guide = _guide(rng, H, W)[None]
        band = 39 if i == len(EDGES_2X) - 1 else gf_ref.GF_BAND
        with _options(native, gf_band=band, gf_int1=1, gf_cols=cols):
            got = native.guided_upscale_batch(native.to_device(disp), native.to_device(guide), r, 1e-3).cpu().numpy()
        ratios.append(_check(got[0], oracle.disp_to_depth(disp[0]), guide[0], r, 1e-3, f"int1 cols={cols} r={r} {W}x{H}", "gff"))
    _report(f"edges_int1 cols={cols} r={r}", ratios)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", [4, 8, 5])
@pytest.mark.parametrize("route", ["gff256", "gfm", "gf"])
def test_batch_of_three_strided_guides(native, r, route):
    """three frames whose guides lie in a [3, 2, H, W] buffer (a strided view), each frame against the oracle"""
    d, g = _frames(500 + r, 3, 67, 43, 134, 86)
    buf = torch.zeros((3, 2, 86, 134), dtype=torch.uint8, device="cuda")
    buf[:, 1] = native.to_device(g)
    with _options(native, **ROUTES[route]):
        got = native.guided_upscale_batch(native.to_device(d), buf[:, 1], r, 1e-3).cpu().numpy()
    _report(f"batch3 {route} r={r}", [_check(got[f], d[f], g[f], r, 1e-3, f"{route} r={r} frame {f}", route) for f in range(3)])


# ------------------------------------------------------------------ eps

@pytest.mark.timeout(300)
@pytest.mark.parametrize("eps", [1e-6, 1e-4, 1e-3, 1e-1, 1.0])
@pytest.mark.parametrize("route,r", [("default", 8), ("default", 3), ("gf", 8)])
def test_eps_range(native, route, r, eps):
    d, g = _frames(600 + r, 1, 131, 67, 262, 134)
    with _options(native, **ROUTES.get(route, {})):
        got = native.guided_upscale(native.to_device(d[0]), native.to_device(g[0]), r, eps).cpu().numpy()
    _report(f"eps {route} r={r} eps={eps:g}", [_check(got, d[0], g[0], r, eps, f"{route} r={r} eps={eps:g}", route)])


# ------------------------------------------------------------------ known answers at the tight bound

ALL_ROUTES = [("gff256", 4), ("gff256", 8), ("gfm", 4), ("gfm", 8), ("gf", 4), ("gf", 8), ("gf", 3), ("gf", 13)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route,r", ALL_ROUTES)
def test_constant_depth_gives_itself(native, route, r):
    """p = c with any guide: cov = 0, a = 0, b = c, q = c; only rounding (F with P = c) separates q from c"""
    rng = np.random.default_rng(700 + r)
    c = np.float32(37.3)
    depth = np.full((67, 131), c, np.float32)
    guide = _guide(rng, 134, 262)
    with _options(native, **ROUTES[route]):
        got = native.guided_upscale(native.to_device(depth), native.to_device(guide), r, 1e-3).cpu().numpy()
    F = gf_ref.floor(depth, guide, r, 1e-3, _family(route, r))
    w = gf_ref.check_f32(got, np.full(guide.shape, float(c)), F, f"{route} r={r} constant p")
    _report(f"const_p {route} r={r}", [w])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route,r", ALL_ROUTES)
def test_constant_guide_gives_double_box(native, oracle, route, r):
    """I = const: var = 0, a = 0 (up to rounding), b = box(p), q = box(box(p)) with the clipped count (computed here in
    float64 from prefix sums, independently of the oracle)"""
    rng = np.random.default_rng(800 + r)
    depth = _depth(rng, 50, 80)
    guide = np.full((100, 160), 77, np.uint8)
    with _options(native, **ROUTES[route]):
        got = native.guided_upscale(native.to_device(depth), native.to_device(guide), r, 1e-3).cpu().numpy()
    p = oracle.bilinear_resize(depth, 160, 100)
    cnt = gf_ref.box_sum(np.ones((100, 160)), r)
    want = gf_ref.box_sum(gf_ref.box_sum(p, r) / cnt, r) / cnt
    F = gf_ref.floor(depth, guide, r, 1e-3, _family(route, r))
    w = gf_ref.check_f32(got, want, F, f"{route} r={r} constant guide")
    _report(f"const_guide {route} r={r}", [w])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("route,r", ALL_ROUTES)
def test_affine_depth_is_reproduced(native, route, r):
    """p = alpha I + beta exactly (p = g / 4 + 5 in float32: alpha = 255 / 4) at identity scale.  In exact arithmetic
    a_k = alpha (1 - e_k) with e_k = eps / (var_k + eps), and q - p = -alpha mean_k(e_k (I - mI_k)), so
    |q - p| <= alpha max_window(e) max_window|I - mI| -- plus ulp32 + F for the rounding"""
    rng = np.random.default_rng(900 + r)
    guide = rng.integers(0, 256, (70, 133)).astype(np.uint8)
    guide[:8, :8] = 128                                     # one flat corner: e ~ 1 there, the bound follows it
    p = (guide.astype(np.float32) * np.float32(0.25) + np.float32(5.0)).astype(np.float32)
    eps = 1e-9
    with _options(native, **ROUTES[route]):
        got = native.guided_upscale(native.to_device(p), native.to_device(guide), r, eps).cpu().numpy().astype(np.float64)
    from scipy.ndimage import maximum_filter
    I = guide / 255.0
    cnt = gf_ref.box_sum(np.ones(I.shape), r)
    mI = gf_ref.box_sum(I, r) / cnt
    e = gf_ref.eps32(eps) / (gf_ref.guide_var(guide, r) + gf_ref.eps32(eps))
    dev = 63.75 * maximum_filter(e, size=2 * r + 1, mode="nearest") * np.maximum(
        maximum_filter(mI, size=2 * r + 1, mode="nearest") - I, I - (-maximum_filter(-mI, size=2 * r + 1, mode="nearest")))
    lim = dev * (1 + 1e-9) + gf_ref.bound(p, gf_ref.floor(p, guide, r, eps, _family(route, r)))
    q = np.abs(got - p) / lim
    k = np.unravel_index(int(q.argmax()), q.shape)
    assert q[k] <= 1.0, f"{route} r={r}: |q - p| = {abs(got[k] - p[k]):.3e} at {k}, bound {lim[k]:.3e}"
    assert np.median(dev) < 1e-6                            # the bound is tight where the guide is textured
    _report(f"affine {route} r={r}", [float(q[k])])


# ------------------------------------------------------------------ the u16 product samples

def _overshoot_case(seed, n, Wlo, Hlo, W, H):
    """u16 depth in blocks of 0, 65535 and mid values, and a guide with the same edges plus texture: at those edges a is
    large and a (I - mean I) carries q above 65535.5 and below -0.5 (the clamp must saturate, not wrap)"""
    rng = np.random.default_rng(seed)
    lo = np.zeros((n, Hlo, Wlo), np.int64)
    gl = np.zeros((n, Hlo, Wlo))
    for f in range(n):
        lo[f] = 30000
        gl[f] = 120
        for k in range(12):
            bw, bh = int(rng.integers(Wlo // 12, Wlo // 4)), int(rng.integers(Hlo // 12, Hlo // 4))
            x, y = int(rng.integers(0, Wlo - bw)), int(rng.integers(0, Hlo - bh))
            hi = k % 2 == 0
            lo[f, y:y + bh, x:x + bw] = 65535 if hi else 0
            gl[f, y:y + bh, x:x + bw] = 220 if hi else 20
        for (x, y, v, gv) in ((Wlo // 10, Hlo // 4, 65535, 220), (Wlo // 2, Hlo // 2, 0, 20)):    # one of each for sure
            lo[f, y:y + Hlo // 3, x:x + Wlo // 5] = v
            gl[f, y:y + Hlo // 3, x:x + Wlo // 5] = gv
    lo += (rng.integers(-600, 601, lo.shape) * (lo == 30000))
    guide = np.repeat(np.repeat(gl, H // Hlo + 1, 1)[:, :H], W // Wlo + 1, 2)[:, :, :W]
    guide = np.clip(guide + rng.normal(0, 25, guide.shape), 0, 255).astype(np.uint8)
    return np.clip(lo, 0, 65535).astype(np.uint16), guide


def _check_u16(got_u16, lo_u16, guide, r, eps, what, route):
    """got within [lo, hi] = clip(rint(float32(want -+ F))); ambiguous pixels (lo != hi) < 1e-4; saturation where want
    leaves [-0.5, 65535.5].  Returns (worst err / bound of the float value behind got, over, under)"""
    depth = lo_u16.astype(np.float32)
    want = gf_ref.reference(depth, guide, r, eps)
    F = gf_ref.floor(depth, guide, r, eps, _family(route, r))
    lo, hi = gf_ref.u16_window(want, F)
    got = got_u16.astype(np.int64)
    bad = (got < lo) | (got > hi)
    if bad.any():
        k = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} samples outside the window, first at {k}: got {got[k]} want {want[k]!r} "
                             f"(F {F[k]:.3e}, allowed {lo[k]}..{hi[k]})")
    amb = float((lo != hi).mean())
    assert amb < 1e-4, f"{what}: {amb:.2e} of the samples are ambiguous"
    over, under = want > 65535.5, want < -0.5
    assert (got[over] == 65535).all() and (got[under] == 0).all()
    return amb, int(over.sum()), int(under.sum())


U16_CASES = [(1, "default"), (3, "default"), (9, "default"), (16, "default")] + [(r, rt) for r in (4, 8) for rt in ("gff256", "gfm", "gf")]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r,route", U16_CASES)
def test_u16_samples_against_the_oracle(native, r, route):
    """v3d_guided_upscale_u16_batch at r in {1, 3, 4, 8, 9, 16} on every route, exact 2x (two frames, strided guides)"""
    lo, guide = _overshoot_case(1000 + r, 2, 232, 110, 464, 220)
    buf = torch.zeros((2, 464 * 220 + 40), dtype=torch.uint8, device="cuda")
    buf[:, :464 * 220] = native.to_device(guide.reshape(2, -1))
    g = buf[:, :464 * 220].view(2, 220, 464)
    with _options(native, **ROUTES.get(route, {})):
        got = native.guided_upscale_u16_batch(torch.from_numpy(lo.view(np.int16)).cuda(), g, r, 1e-3).cpu().numpy().view(np.uint16)
    over = under = 0
    for f in range(2):
        amb, o, u = _check_u16(got[f], lo[f], guide[f], r, 1e-3, f"u16 {route} r={r} frame {f}", route)
        over, under = over + o, under + u
    assert over > 0 and under > 0, f"the case must overshoot both ends (over {over}, under {under})"
    print(f"\nACC u16 {route} r={r} ambiguous<{1e-4} over={over} under={under}")


@pytest.mark.timeout(600)
def test_u16_product_geometry(native):
    """1920x1080 -> 3840x2160, two frames, r = 8, eps = 1e-3: the pipeline's u16 output"""
    lo, guide = _overshoot_case(77, 2, 1920, 1080, 3840, 2160)
    got = native.guided_upscale_u16_batch(torch.from_numpy(lo.view(np.int16)).cuda(), native.to_device(guide), 8, 1e-3)
    got = got.cpu().numpy().view(np.uint16)
    for f in range(2):
        amb, o, u = _check_u16(got[f], lo[f], guide[f], 8, 1e-3, f"4K u16 frame {f}", "default")
        assert o > 0 and u > 0
        print(f"\nACC u16_4k frame={f} ambiguous={amb:.2e} over={o} under={u}")
