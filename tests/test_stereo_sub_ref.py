"""The sub-pixel DIBR contract (tests/stereo_sub_ref.py) on the CPU: the vectorised restatement against the literal loop, rows
computed by hand, the properties the contract promises, the exactness of the division the kernel uses, the quality case on the
two references, and the coverage of the scenes the GPU tests render."""
import numpy as np
import pytest

import stereo_ref as R
import stereo_sub_ref as S


def _frame(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def test_vectorised_equals_the_loop_on_random_cases():
    rng = np.random.default_rng(1)
    total = dict.fromkeys(S.COUNT_KEYS, 0)
    for case in range(60):
        W, H = int(rng.integers(1, 51)), int(rng.integers(1, 4))
        F = _frame(H, W, case)
        D = rng.integers(0, 65536, (H, W)).astype(np.uint16)
        if case % 3 == 0:
            D = (D // 64 + 20000).astype(np.uint16)                                 # gentle depth: connected spans
        gl, gr = (int(v) for v in rng.integers(-30000, 30001, 2))
        if case % 7 == 0:
            gl, gr = int(rng.integers(-S.GMAX, S.GMAX + 1)), int(rng.integers(-S.GMAX, S.GMAX + 1))
        conv = int(rng.integers(0, 65536))
        for layout in (S.FULL_SBS,) + ((S.HALF_SBS,) if W % 2 == 0 else ()):
            got, cg = S.render_counts(F, D, gl, gr, conv, layout)
            want, cw = S.render_loop(F, D, gl, gr, conv, layout)
            assert np.array_equal(got, want), (case, W, H, gl, gr, conv, layout)
            assert cg == cw, (case, cg, cw)
        S._add(total, cg)
    assert all(total[k] > 0 for k in S.COUNT_KEYS), total


def test_hand_computed_rows():
    F = np.array([[[10, 20, 30], [50, 60, 70], [90, 100, 110], [130, 140, 150]]], np.uint8)
    conv = 0
    g = 1 << 10                                                     # s16 = floor((1024 D + 2^19) / 2^20) = round-half-up(D / 1024)
    # p = 16x + s16: 0+4, 16+8, 32+40, 48+40 -> 4, 24, 72, 88; L' = 20, 48 (tear), 16; last column a point
    D = np.array([[4096, 8192, 40960, 40960]], np.uint16)
    E, cnt = S.eye_image(F, D, g, conv)
    # x=0: [4, 24) covers t=1 (16), w=12, L=20: floor((2 (8 a + 12 b) + 20) / 40); x=1: point [24, 40) covers t=2, colour F[1];
    # x=2: [72, 88) covers t=5 (out of range); x=3: point [88, 104) covers t=6 (out of range)
    # t=0: hole, left none -> right neighbour t=1; t=3: hole, left t=2 only
    t1 = [(2 * (8 * a + 12 * b) + 20) // 40 for a, b in zip(F[0, 0].tolist(), F[0, 1].tolist())]
    assert t1 == [34, 44, 54]
    assert E[0].tolist() == [t1, t1, [50, 60, 70], [50, 60, 70]]
    assert (cnt["connected1"], cnt["connected0"], cnt["connected2"], cnt["tears"], cnt["folds"]) == (2, 0, 0, 1, 0)
    assert (cnt["out_of_range"], cnt["holes_left"], cnt["holes_right"], cnt["z_conflicts"], cnt["empty_rows"]) == (2, 1, 1, 0, 0)

    # a fold: the near pixel (x=0) lands on the far one's (x=1) target and wins by depth; a stretched span covers two targets
    D = np.array([[16384 + 1024 * 24, 16384, 16384, 16384 + 1024 * 16]], np.uint16)
    conv = 16384
    # s16 = 24, 0, 0, 16: p = 24, 16, 32, 64; L' = -8 (fold), 16, 32; x=0 point [24, 40): t=2; x=1 [16, 32): t=1, w=0;
    # x=2 [32, 64): t=2 (w=0), t=3 (w=16, L=32: the midpoint); x=3 point [64, 80): t=4 out of range
    E, cnt = S.eye_image(F, D, g, conv)
    mid = [(2 * (16 * a + 16 * b) + 32) // 64 for a, b in zip(F[0, 2].tolist(), F[0, 3].tolist())]
    assert mid == [110, 120, 130]
    assert E[0].tolist() == [[50, 60, 70], [50, 60, 70], [10, 20, 30], mid]      # t=0: hole, only a right neighbour (t=1)
    assert (cnt["folds"], cnt["connected1"], cnt["connected2"], cnt["z_conflicts"], cnt["out_of_range"]) == (1, 1, 1, 1, 1)
    assert (cnt["holes_left"], cnt["holes_right"]) == (0, 1)

    # a compressed span with no target: p = 17, 25, ... -> [17, 25) holds no multiple of 16
    D = np.array([[1024 * 17, 1024 * 9, 1024 * 9, 1024 * 9]], np.uint16)
    E, cnt = S.eye_image(F, D, g, 0)
    assert cnt["connected0"] == 1 and cnt["connected1"] == 2
    # everything shifted off the row: black
    E, cnt = S.eye_image(F, np.full((1, 4), 65535, np.uint16), S.GMAX, 0)
    assert not E.any() and cnt["empty_rows"] == 1 and cnt["out_of_range"] == 4


def test_gain_zero_reproduces_the_frame():
    F = _frame(3, 40, 2)
    D = np.random.default_rng(2).integers(0, 65536, (3, 40)).astype(np.uint16)
    out = S.render(F, D, 0, 0, 12345)
    assert np.array_equal(out[:, :40], F) and np.array_equal(out[:, 40:], F)


def test_whole_pixel_shift_equals_the_integer_renderer():
    F = _frame(2, 37, 3)
    gl, gr, conv = 6144, -6144, 32768
    for k in (0, 1, 3, 5):
        # s16 = floor((6144 (D - conv) + 2^19) / 2^20) = 16 k exactly for D - conv = ceil(16 k 2^20 / 6144)
        d = conv + -((-16 * k << 20) // 6144)
        assert (gl * (d - conv) + (1 << 19)) >> 20 == 16 * k and (gr * (d - conv) + (1 << 19)) >> 20 == -16 * k
        D = np.full((2, 37), d, np.uint16)
        assert np.array_equal(S.render(F, D, gl, gr, conv), R.render(F, D, gl, gr, conv)), k


@pytest.mark.parametrize("s16", [13, 29, -3, -20, 1, 15])
def test_fractional_constant_shift_is_the_two_tap_interpolation(s16):
    H, W = 2, 31
    F = _frame(H, W, 4)
    g, conv = 1 << 10, 30000
    D = np.full((H, W), conv + 1024 * s16, np.uint16)
    E, _ = S.eye_image(F, D, g, conv)
    k, r = s16 >> 4, s16 & 15                                       # p = 16 (x + k) + r, r in 1..15: target x + k + 1, w = 16 - r
    Fi = F.astype(np.int64)
    want = np.zeros_like(Fi)
    hit = np.zeros(W, bool)
    for x in range(W - 1):
        t = x + k + 1
        if 0 <= t < W:
            want[:, t] = (2 * (r * Fi[:, x] + (16 - r) * Fi[:, x + 1]) + 16) // 32
            hit[t] = True
    t = W - 1 + k + 1                                               # the last column is a point
    if 0 <= t < W:
        want[:, t], hit[t] = Fi[:, W - 1], True
    idx = np.flatnonzero(hit)
    for t in range(W):                                              # equal depths: a hole takes its left neighbour if it has one
        if not hit[t]:
            left = idx[idx < t]
            want[:, t] = want[:, left[-1]] if len(left) else want[:, idx[idx > t][0]]
    assert np.array_equal(E, want.astype(np.uint8))


def test_a_frame_does_not_depend_on_its_batch():
    """the reference is a function of one frame: the GPU test holds the batch entry to exactly these per-frame bits"""
    F, D = _frame(3, 20, 5), S.scene_depth("planar", 3, 20, 5)
    a = S.render(F, D, *S.stereo_gains())
    b = S.render(np.ascontiguousarray(F[::-1])[::-1], D.copy(order="F"), *S.stereo_gains())      # other strides, same values
    assert np.array_equal(a, b)
    rows = np.concatenate([S.render(F[y:y + 1], D[y:y + 1], *S.stereo_gains()) for y in range(3)])
    assert np.array_equal(a, rows)                                  # rows are independent


def test_division_as_multiply_is_exact():
    """the kernel's form of step 4's division: (n * ceil(2^20 / 2L)) >> 20 == n // 2L for every numerator <= 16352 and every even
    divisor <= 64; its products stay below 2^32 for the numerators a span of length L can produce (<= 511 L)"""
    n = np.arange(16353, dtype=np.int64)
    for L in range(1, S.TEAR16 + 1):
        m = S.DIV_MUL[L]
        assert m == ((1 << 20) + 2 * L - 1) // (2 * L)              # the kernel's table
        assert np.array_equal((n * m) >> 20, n // (2 * L)), L
        assert 511 * L * m < 1 << 32
    assert 2 * 32 * 255 + 32 == 16352


def test_shift_without_the_64_bit_product_is_exact():
    """the kernel's form of step 1: with g = 2^12 gh + gl, floor((g dd + 2^19) / 2^20) == (dd gh + ((dd gl + 2^19) >> 12)) >> 8,
    every product and sum inside 32 bits (24-bit operands)"""
    rng = np.random.default_rng(6)
    g = np.concatenate([rng.integers(-S.GMAX, S.GMAX + 1, 200000), [S.GMAX, -S.GMAX, 0, 1, -1, 4095, 4096, -4096, -4097, 6144, -6144]])
    dd = np.concatenate([rng.integers(-65535, 65536, 200000), [65535, -65535, 0, 1, -1, 65535, -65535, 65535, -65535, 5000, -5000]])
    for gg, d in ((g, dd), (g, dd[::-1]), (g[-11:, None], np.arange(-65535, 65536)[None, :])):
        gh, gl = gg >> 12, gg & 4095
        a, b = d * gh, d * gl + (1 << 19)
        assert np.abs(d).max() < 1 << 23 and np.abs(gh).max() < 1 << 23 and np.abs(a).max() < 1 << 30 and np.abs(b).max() < 1 << 30
        assert np.array_equal((a + (b >> 12)) >> 8, (gg * d + (1 << 19)) >> 20)


def _quality_errors():
    W = 400
    x = np.arange(W, dtype=np.float64)
    Df = 10000 + 45000 * x / 399
    D = np.rint(Df).astype(np.uint16)[None]
    tex = lambda u: 127.5 + 100 * np.sin(u / 7)
    F = np.repeat(np.rint(tex(x)).astype(np.uint8)[None, :, None], 3, axis=2)
    gl, gr, conv = R.stereo_gains()
    assert (gl, gr, conv) == (6144, -6144, 32768)
    xs = np.arange(0, 399 * 64 + 1, dtype=np.float64) / 64          # the continuous warp on a 64x dense grid
    out = {}
    sub, integer = S.render(F, D, gl, gr, conv), R.render(F, D, gl, gr, conv)
    for e, g in enumerate((gl, gr)):
        u = xs + g / 256 * ((10000 + 45000 * xs / 399) - conv) / 65536
        assert (np.diff(u) > 0).all()
        t = np.arange(W, dtype=np.float64)
        inside = (t >= u[0]) & (t <= u[-1])                         # targets outside the warped range are left out
        truth = tex(np.interp(t[inside], u, xs))
        err = [np.abs(img[0, e * W:(e + 1) * W, 0][inside].astype(np.float64) - truth) for img in (sub, integer)]
        out[e] = (err[0].mean(), err[1].mean(), err[0].max(), err[1].max())
    return out


def test_quality_subpixel_error_is_at_most_a_quarter_of_the_integer_renderers():
    """W = 400 ramp over a sinusoidal texture at the default gains, against the float-exact warp: mean absolute error per eye"""
    for e, (sub, integer, sub_max, int_max) in _quality_errors().items():
        print(f"eye {e}: sub-pixel mean {sub:.3f} max {sub_max:.2f}; integer mean {integer:.3f} max {int_max:.2f}; ratio {sub / integer:.3f}")
        assert sub <= integer / 4, (e, sub, integer)


def gpu_scene_counts():
    """the case counts of the small scenes tests/test_stereo_sub_gpu.py renders (its widths 7, 255 and 257)"""
    total = dict.fromkeys(S.COUNT_KEYS, 0)
    per = {}
    for W, H in ((7, 4), (255, 5), (257, 4)):
        F = _frame(H, W, W)
        for kind in S.SCENES:
            D = S.scene_depth(kind, H, W, W + H)
            for (gl, gr, conv) in S.scene_params(W):
                _, c = S.render_counts(F, D, gl, gr, conv)
                S._add(total, c)
                S._add(per.setdefault(kind, dict.fromkeys(S.COUNT_KEYS, 0)), c)
    return total, per


def test_gpu_scenes_reach_every_case_class():
    total, per = gpu_scene_counts()
    assert all(total[k] > 0 for k in S.COUNT_KEYS), total
    # the scenes do what their names say at the default gain
    D = S.scene_depth("steep", 1, 257, 0)
    _, c = S.eye_image(_frame(1, 257, 0), D, 6144, 32768)
    assert c["connected2"] > 100                                    # L = 24: every other span covers two targets
    _, c = S.eye_image(_frame(1, 257, 0), S.scene_depth("shallow", 1, 257, 0), 6144, 32768)
    assert c["connected0"] > 100                                    # L = 8: every other span covers none
    assert per["noise"]["folds"] and per["noise"]["tears"] and per["noise"]["z_conflicts"]
