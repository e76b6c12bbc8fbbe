"""GPU: every route of the correlation lookup (csrc/v3d_corr.hip) against the float64 reference of tests/corr_ref.py.

The kernels' arithmetic is fully determined up to the MFMA's summation order: float32 bilinear weights, each 8-channel chunk
of a warped position blended in float32 and rounded once to bf16, 64 exact bf16 x bf16 products summed in float32, an exact
1/64.  corr_ref.interval() turns that into a per-output interval about one float32 ulp of the output's scale wide (plus the
rare warped value with two admissible bf16 roundings); the older tests allow 2e-2 of the scale.

Routes (v3d_set_option): "default" (k_corr_fused0 for the 1x9 pattern while its LDS fits, i.e. G <= 17; k_corr_warp +
k_corr<1> for the 3x3 pattern), "two_kernel" (corr_fused 0: k_corr_warp + k_corr<pattern>), "gather" (corr_gather 1:
k_corr_gather<pattern>).  Group counts G in {1, 2, 3, 4, 5, 8, 17, 18}: odd ones do not divide k_corr_fused0's 256 staging
threads evenly, G >= 5 needs more than one staging pass, G = 17 is the largest fused launch and G = 18 falls back.

Each test prints `ACC <name> <worst> <worst ambiguous>`: the worst |got - mid| / half-width over outputs without and with an
ambiguous warped value.  Measured on an MI355X: at most 0.088 without (every route, pattern and G alike: the MFMA's sums sit
well inside their 64-rounding allowance), at most 0.999 with (the output took one of the two admissible bf16 values).

What these tests catch that the older ones did not (scratch builds, one kernel at a time, measured on an MI355X): a truncating
or round-half-away bf16 conversion of the warped value, or bilinear weights rounded to bf16, in k_corr_warp, k_corr_gather or
k_corr_fused0 fails test_group_counts, test_geometry_sweep, test_flow_classes and test_configs3_sampled_rows on the routes
that run the kernel (and test_ties_round_to_even for the two conversions).  Of the older tests only the cross-route bit-identity
checks fail, and only because the other route was left correct (round-half-away in k_corr_gather passes them all); none of
their oracle comparisons fails.  k_corr_fused0 staging by a constant 72
positions (right for G = 4 only) fails test_group_counts at G = 5, 8, 17, test_geometry_sweep at G = 5, and the two exact
tests, and every older test passes."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import corr_ref as R

pytestmark = pytest.mark.gpu

ROUTES = {"default": {"corr_fused": 1, "corr_gather": 0},
          "two_kernel": {"corr_fused": 0, "corr_gather": 0},
          "gather": {"corr_fused": 1, "corr_gather": 1}}
GROUPS = [1, 2, 3, 4, 5, 8, 17, 18]
WIDTHS = [1, 2, 15, 16, 17, 63, 64, 65, 72, 127, 129, 200]
HEIGHTS = [1, 2, 3, 7]


@contextlib.contextmanager
def _options(native, route):
    saved = {k: native.get_option(k) for k in ("corr_fused", "corr_gather")}
    try:
        for k, v in ROUTES[route].items():
            native.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            native.set_option(k, v)


def _run(native, route, fl, fr, flow, G, pattern):
    """fl, fr [h, w, C] bf16 values as float32, flow [2, h, w] -> the route's output as float64 [G*9, h, w]"""
    fl_d = torch.from_numpy(fl).to("cuda", torch.bfloat16)
    fr_d = torch.from_numpy(fr).to("cuda", torch.bfloat16)
    with _options(native, route):
        out = native.corr_lookup(fl_d, fr_d, torch.from_numpy(flow).cuda(), G, pattern)
    return out.cpu().numpy().astype(np.float64)


def _report(name, pairs):
    w0 = max(p[0] for p in pairs)
    w1 = max(p[1] for p in pairs)
    print(f"\nACC {name} {w0:.4g} {w1:.4g}")


def _inputs(seed, h, w, G, flow, feat):
    rng = np.random.default_rng(seed)
    fl, fr = R.features(feat, (h, w, 64 * G), rng), R.features(feat, (h, w, 64 * G), rng)
    return fl, fr, R.flow_field(flow, h, w, rng)


@functools.lru_cache(maxsize=None)
def _interval(seed, h, w, G, pattern, flow, feat):
    """the reference interval of one case (shared by the three routes)"""
    return R.interval(*_inputs(seed, h, w, G, flow, feat), G, pattern)


def _check_case(native, route, seed, h, w, G, pattern, flow, feat):
    fl, fr, fw = _inputs(seed, h, w, G, flow, feat)
    lo, hi, amb, zero = _interval(seed, h, w, G, pattern, flow, feat)
    got = _run(native, route, fl, fr, fw, G, pattern)
    what = f"{route} pattern {pattern} G={G} {h}x{w} {flow} {feat}"
    assert (got[zero] == 0).all(), f"{what}: {int((got[zero] != 0).sum())} outputs of all-outside positions are not 0"
    return R.check(got, lo, hi, amb, what)


# ------------------------------------------------------------------ every group count on every route

GROUP_SHAPES = [(3, 65, "normal"), (2, 17, "spread"), (7, 129, "normal")]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("G", GROUPS)
def test_group_counts(native, G, route, pattern):
    pairs = [_check_case(native, route, 10 * G + i, h, w, G, pattern, "mixed", feat) for i, (h, w, feat) in enumerate(GROUP_SHAPES)]
    _report(f"groups G={G} {route} pattern {pattern}", pairs)


# ------------------------------------------------------------------ every geometry at G in {1, 4, 5}

@pytest.mark.timeout(300)
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("G", [1, 4, 5])
def test_geometry_sweep(native, G, route, pattern):
    """h in {1, 2, 3, 7} x w in {1, 2, 15, 16, 17, 63, 64, 65, 72, 127, 129, 200}: the 16-pixel MFMA tile and the 64-pixel
    fused block, ragged and narrower than either, the 3x3 clamp at one and two rows"""
    pairs = []
    for i, h in enumerate(HEIGHTS):
        for j, w in enumerate(WIDTHS):
            feat = "spread" if (i + j) % 3 == 2 else "normal"
            pairs.append(_check_case(native, route, 1000 * G + 20 * i + j, h, w, G, pattern, "mixed", feat))
    _report(f"geometry G={G} {route} pattern {pattern}", pairs)


# ------------------------------------------------------------------ every flow class

@pytest.mark.timeout(300)
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("flow", R.FLOWS)
def test_flow_classes(native, flow, route, pattern):
    """each class of sample coordinate on its own (G = 3), with N(0, 1) features and with magnitudes spread over 2^+-20"""
    pairs = [_check_case(native, route, 500 + i, h, w, 3, pattern, flow, feat)
             for i, (h, w, feat) in enumerate([(7, 72, "normal"), (3, 129, "spread")])]
    _report(f"flows {flow} {route} pattern {pattern}", pairs)


# ------------------------------------------------------------------ BASELINE configs[3]

@functools.lru_cache(maxsize=None)
def _configs3(pattern):
    h, w, G = 270, 480, 4
    rng = np.random.default_rng(3270 + pattern)
    fl, fr = R.features("normal", (h, w, 64 * G), rng), R.features("normal", (h, w, 64 * G), rng)
    fw = R.flow_field("mixed", h, w, rng)
    rows = np.unique(np.concatenate([[0, 1, 2, 15, 16, 135, h - 3, h - 2, h - 1], rng.choice(h, 16, replace=False)]))
    return fl, fr, fw, rows, R.interval(fl, fr, fw, G, pattern, rows=rows)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_configs3_sampled_rows(native, route, pattern):
    """270 x 480 x 256 features, G = 4, mixed flows: the whole lookup on the device, the reference on ~25 rows (0, 1, h-2 and
    h-1 among them; the 3x3 pattern's interval uses the warp of the neighbouring rows)"""
    fl, fr, fw, rows, (lo, hi, amb, zero) = _configs3(pattern)
    got = _run(native, route, fl, fr, fw, 4, pattern)[:, rows]
    assert (got[zero] == 0).all()
    _report(f"configs3 {route} pattern {pattern} rows={len(rows)}", [R.check(got, lo, hi, amb, f"configs3 {route} pattern {pattern}")])


# ------------------------------------------------------------------ exact answers

@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_all_outside_gives_exact_zeros(native, route, pattern):
    """every sample coordinate <= -1 or >= w (>= h): all four taps outside, every output exactly 0 (G = 3 and G = 17)"""
    for G, h, w in ((3, 7, 72), (17, 3, 65)):
        rng = np.random.default_rng(G)
        fl, fr = R.features("normal", (h, w, 64 * G), rng), R.features("normal", (h, w, 64 * G), rng)
        X = np.broadcast_to(np.arange(w, dtype=np.float64), (h, w))
        Y = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
        tx = np.where(rng.random((h, w)) < 0.5, R._coords("outside", X, w, rng), X + rng.uniform(-4, 4, (h, w)))
        ty = np.where(tx > -1, R._coords("outside", Y, h, rng), Y + rng.uniform(-4, 4, (h, w)))
        tx = np.where((tx > -1) & (tx < w) & (ty > -1) & (ty < h), -1.0, tx)
        fw = np.stack([tx - X, ty - Y]).astype(np.float32)
        got = _run(native, route, fl, fr, fw, G, pattern)
        assert (got == 0).all(), f"G={G}: {int((got != 0).sum())} nonzero outputs, max {np.abs(got).max()!r}"


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_integer_flows_give_the_exact_dot(native, route, pattern):
    """integer flows (weights exactly 0 or 1), features small integers: every sum is exact, out = dot / 64 to the bit (computed in
    integers here), at G = 5 and G = 2, positions outside the image included"""
    for G, h, w in ((5, 7, 129), (2, 3, 200)):
        rng = np.random.default_rng(70 + G)
        C = 64 * G
        fl = rng.integers(-8, 9, (h, w, C)).astype(np.float32)
        fr = rng.integers(-8, 9, (h, w, C)).astype(np.float32)
        fx, fy = rng.integers(-5, 6, (h, w)), rng.integers(-3, 4, (h, w))
        fw = np.stack([fx, fy]).astype(np.float32)
        got = _run(native, route, fl, fr, fw, G, pattern)
        sx, sy = np.arange(w)[None, :] + fx, np.arange(h)[:, None] + fy
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        warp = np.where(inside[..., None], fr[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)], 0).astype(np.int64)
        a = fl.astype(np.int64)
        for k in range(9):
            dy, dx = R.window(pattern, k)
            yy = np.clip(np.arange(h) + dy, 0, h - 1)[:, None]
            xx = np.clip(np.arange(w) + dx, 0, w - 1)[None, :]
            dot = (a * warp[yy, xx]).reshape(h, w, G, 64).sum(-1)
            for g in range(G):
                want = dot[..., g] / 64.0
                bad = got[g * 9 + k] != want
                assert not bad.any(), (f"G={G} plane {g * 9 + k}: {int(bad.sum())} outputs differ, first at "
                                       f"{tuple(np.argwhere(bad)[0])}: got {got[g * 9 + k][bad][0]!r} want {want[bad][0]!r}")


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(ROUTES))
def test_ties_round_to_even(native, route, pattern):
    """flow (0.5, 0): the blend of adjacent columns holding ADJACENT bf16 values is their midpoint, exact in float32 (delta = 0),
    and must round to the even one of the two; one-hot fl picks one channel per group, so out = B / 64 exactly.  Even and odd
    lower neighbours, both signs, exponents from 2^-20 to 2^20."""
    G, h, w = 3, 3, 72
    C = 64 * G
    rng = np.random.default_rng(11)
    base = (rng.integers(0x3580, 0x4980, (h, 1, C)) | (rng.integers(0, 2, (h, 1, C)) << 15)).astype(np.uint32)
    bits = base + ((np.arange(w)[None, :, None] + np.arange(C)[None, None, :]) & 1).astype(np.uint32)
    fr = (bits << 16).view(np.float32)
    fl = np.zeros((h, w, C), np.float32)
    sel = (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 3) % 64
    for g in range(G):
        np.put_along_axis(fl[..., 64 * g:64 * (g + 1)], sel[..., None], 1.0, axis=2)
    fw = np.stack([np.full((h, w), 0.5), np.zeros((h, w))]).astype(np.float32)
    got = _run(native, route, fl, fr, fw, G, pattern)
    # the warped value at every position, by hand: (a + b) / 2 rounded to even (the last column has one tap: a / 2, exact)
    a = fr.astype(np.float64)
    b = np.concatenate([a[:, 1:], np.zeros((h, 1, C))], axis=1)
    B = R.bf16(((a + b) / 2).astype(np.float32)).astype(np.float64)
    assert (((a + b) / 2 != B)[:, :-1].mean()) > 0.99            # (almost) every blend is a tie
    for k in range(9):
        dy, dx = R.window(pattern, k)
        yy = np.clip(np.arange(h) + dy, 0, h - 1)[:, None]
        xx = np.clip(np.arange(w) + dx, 0, w - 1)[None, :]
        for g in range(G):
            want = np.take_along_axis(B[yy, xx][..., 64 * g:64 * (g + 1)], sel[..., None], axis=2)[..., 0] / 64
            bad = got[g * 9 + k] != want
            assert not bad.any(), (f"plane {g * 9 + k}: {int(bad.sum())} ties rounded wrongly, first at {tuple(np.argwhere(bad)[0])}: "
                                   f"got {got[g * 9 + k][bad][0]!r} want {want[bad][0]!r}")
