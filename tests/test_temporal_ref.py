"""The NumPy reference of the temporal stabilisation (tests/temporal_ref.py) against a literal per-pixel, per-tap loop, hand-
computed pixels, and the properties the contract promises.  CPU only; the GPU entries are pinned to this reference in
test_temporal_gpu.py."""
import numpy as np
import pytest

import temporal_ref as TR


def _clip(rng, T, H, W, invalid=0.2, blend=False):
    if blend:
        depth = rng.uniform(0.0, 64.0, (T, H, W)).astype(np.float32)
    else:
        depth = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
    depth[rng.random((T, H, W)) < invalid] = 0.0
    base = rng.integers(0, 256, (H, W))
    gray = np.clip(base[None] + rng.integers(-20, 21, (T, H, W)), 0, 255).astype(np.uint8)
    return depth, gray


@pytest.mark.parametrize("seed", range(12))
def test_vectorised_reference_equals_the_literal_loop(seed):
    rng = np.random.default_rng(seed)
    T, H, W = int(rng.integers(1, 7)), int(rng.integers(1, 6)), int(rng.integers(1, 8))
    if seed == 0:
        H = W = 1
    R = (0, 1, 2, 3, 8, 5, 4, 2, 1, 8, 6, 7)[seed]
    tau = (1, 12, 255)[seed % 3]
    fill = seed % 2
    depth, gray = _clip(rng, T, H, W, blend=seed % 4 == 3)
    cut = (rng.random(T) < 0.3).astype(np.uint8)
    cut[0] = 0
    got = TR.filter_clip(depth, gray, R, tau, cut, fill)
    want = TR.filter_loops(depth, gray, R, tau, cut, fill)
    assert np.array_equal(got, want)


def test_one_pixel_by_hand():
    """1x1 frames, R = 1, tau = 12: rw = 256 - floor(256 * 9|dY| / 108) (all nine neighbours are the pixel itself)"""
    gray = np.array([100, 103, 109], np.uint8).reshape(3, 1, 1)
    depth = np.array([10.0, 11.0, 20.0], np.float32).reshape(3, 1, 1)              # d16 = 160, 176, 320
    # target 1: k=-1: s = 27, rw = 256 - 64 = 192, tw = 1 -> 192; k=0: 2 * 256 = 512; k=+1: s = 54, rw = 128 -> 128
    Wsum, Dsum = 192 + 512 + 128, 192 * 160 + 512 * 176 + 128 * 320
    assert TR.filter_clip(depth, gray, 1, 12)[1, 0, 0] == ((2 * Dsum + Wsum) // (2 * Wsum)) / 16.0
    # rounding half up: two equal weights, d16 = 160 and 161 -> 160.5 -> 161
    out = TR.filter_clip(np.array([160, 161], np.float32).reshape(2, 1, 1) / 16, np.zeros((2, 1, 1), np.uint8), 1, 12)
    # target 0: weights 2*256 (own) and 1*256: (2*(512*160 + 256*161) + 768) // 1536 = 160; target 1: 161
    assert out[0, 0, 0] * 16 == (2 * (512 * 160 + 256 * 161) + 768) // 1536 == 160
    d = np.array([160, 0, 161], np.float32).reshape(3, 1, 1) / 16
    out = TR.filter_clip(d, np.zeros((3, 1, 1), np.uint8), 1, 12)                  # centre invalid, neighbours 160 and 161
    assert out[1, 0, 0] * 16 == (2 * 256 * 321 + 512) // 1024 == 161               # 160.5 rounds up
    assert TR.filter_clip(d, np.zeros((3, 1, 1), np.uint8), 1, 12, fill=0)[1, 0, 0] == 0
    # Wsum = 0: every frame of the window invalid, or every neighbour too different and the centre invalid
    assert TR.filter_clip(np.zeros((3, 1, 1), np.float32), np.zeros((3, 1, 1), np.uint8), 1, 12)[1, 0, 0] == 0
    g = np.array([0, 200, 0], np.uint8).reshape(3, 1, 1)
    assert TR.filter_clip(d, g, 1, 12)[1, 0, 0] == 0
    # rint is half to even: 0.03125 * 16 = 0.5 -> 0 (invalid), 0.09375 * 16 = 1.5 -> 2
    assert list(TR.d16_of(np.array([0.03125, 0.09375, -1.0], np.float32))) == [0, 2, 0]       # invalid is 0, whatever it rounds to


def test_radius_zero_is_the_identity_and_the_per_frame_range():
    rng = np.random.default_rng(1)
    depth, gray = _clip(rng, 4, 5, 7)
    assert np.array_equal(TR.filter_clip(depth, gray, 0, 12), depth)
    cut = TR.cuts(gray, 20)
    mm = TR.minmax(depth)
    assert np.array_equal(TR.ranges(mm, cut, 0), mm)
    from oracle import oracle as O
    assert np.array_equal(TR.stabilize(depth, gray, 0), np.stack([O.depth_to_u16(d) for d in depth]))


def test_own_range_reproduces_depth_to_u16():
    from oracle import oracle as O
    rng = np.random.default_rng(2)
    depth = rng.uniform(0, 64, (3, 9, 11)).astype(np.float32)
    depth[2] = 7.0                                                                  # constant frame -> 0
    got = TR.to_u16_range(depth, TR.minmax(depth))
    assert np.array_equal(got, np.stack([O.depth_to_u16(d) for d in depth])) and not got[2].any()
    # a value 1/32 outside the range is clamped, in float32, before the conversion
    lohi = np.array([[1.0, 2.0]], np.float32)
    d = np.array([[[1.0 - 1 / 32, 1.0, 2.0, 2.0 + 1 / 32]]], np.float32)
    assert list(TR.to_u16_range(d, lohi)[0, 0]) == [0, 0, 65535, 65535]


def test_frozen_clip_comes_back_unchanged():
    rng = np.random.default_rng(3)
    depth, gray = _clip(rng, 1, 6, 9)
    depth, gray = np.repeat(depth, 5, 0), np.repeat(gray, 5, 0)
    for R in (1, 2, 8):
        for fill in (0, 1):
            assert np.array_equal(TR.filter_clip(depth, gray, R, 12, fill=fill), depth)


def test_frames_on_two_sides_of_a_cut_never_mix():
    rng = np.random.default_rng(4)
    dA, gA = _clip(rng, 4, 6, 8)
    dB, gB = _clip(rng, 3, 6, 8)
    gB = (255 - gB // 3).astype(np.uint8)
    gA = (gA // 3).astype(np.uint8)                                                  # scenes A and B differ by > 20 levels
    depth, gray = np.concatenate([dA, dB]), np.concatenate([gA, gB])
    cut = TR.cuts(gray, 20)
    assert list(cut) == [0, 0, 0, 0, 1, 0, 0]
    for R in (1, 2, 8):
        whole = TR.stabilize(depth, gray, R)
        assert np.array_equal(whole[:4], TR.stabilize(dA, gA, R)) and np.array_equal(whole[4:], TR.stabilize(dB, gB, R))
        f = TR.filter_clip(depth, gray, R, 12, cut)
        assert np.array_equal(f[:4], TR.filter_clip(dA, gA, R, 12)) and np.array_equal(f[4:], TR.filter_clip(dB, gB, R, 12))


def test_cut_thresholds():
    g = np.zeros((3, 4, 5), np.uint8)
    g[1] = 20                                               # mean difference exactly 20: not a cut at c = 20 (strict >)
    g[2] = 20
    g[2, 0, 0] = 21                                         # frames 1 -> 2 differ in one pixel by 1
    assert list(TR.cuts(g, 20)) == [0, 0, 0] and list(TR.cuts(g, 19)) == [0, 1, 0]
    assert list(TR.cuts(g, 0)) == [0, 1, 1] and list(TR.cuts(g, 256)) == [0, 0, 0]
    g[1, 0, 0] = 21                                         # sum = 20 * 20 + 1 > 20 * 20
    assert list(TR.cuts(g, 20)) == [0, 1, 0]


def test_int32_is_enough_at_radius_8():
    """d16 = 32767 everywhere, identical frames, R = 8: the largest numerator the kernel's int32 ever holds"""
    T = 17
    depth = np.full((T, 2, 2), 32767 / 16.0, np.float32)
    gray = np.full((T, 2, 2), 9, np.uint8)
    out = TR.filter_clip(depth, gray, 8, 12)
    assert np.array_equal(out, depth)
    Wsum = 256 * sum(9 - abs(k) for k in range(-8, 9))
    assert Wsum == 81 * 256 and 2 * Wsum * 32767 + Wsum < 2 ** 31


def test_multiply_shift_is_exact_for_every_s_and_tau():
    """the kernel's floor(256 s / (9 tau)) = (256 s * ceil(2^32 / (9 tau))) >> 32, s in 0..2295, tau in 1..255; mul fits 32 bits"""
    s = np.arange(TR.S_MAX + 1, dtype=np.uint64)
    for tau in range(1, 256):
        mul = TR.rw_magic(tau)
        assert mul < 2 ** 32
        q = ((s * np.uint64(256)) * np.uint64(mul)) >> np.uint64(32)
        assert np.array_equal(q.astype(np.int64), (256 * s.astype(np.int64)) // (9 * tau)), tau
        assert np.array_equal(TR.range_weight(s, tau), np.maximum(0, 256 - q.astype(np.int64)))


def test_stabilised_blend_stays_within_a_thirty_second_of_the_range():
    rng = np.random.default_rng(5)
    depth, gray = _clip(rng, 5, 8, 8, invalid=0.0, blend=True)
    cut = np.zeros(5, np.uint8)
    f = TR.filter_clip(depth, gray, 2, 255, cut)
    lohi = TR.ranges(TR.minmax(depth), cut, 2)
    assert (f >= lohi[:, :1, None] - 1 / 32).all() and (f <= lohi[:, 1:, None] + 1 / 32).all()
    stereo = np.rint(depth * 16).astype(np.float32) / 16                                  # exact multiples of 1/16 stay inside
    f = TR.filter_clip(stereo, gray, 2, 255, cut)
    lohi = TR.ranges(TR.minmax(stereo), cut, 2)
    assert (f >= lohi[:, :1, None]).all() and (f <= lohi[:, 1:, None]).all()


# ---------------------------------------------------------------- NaN, infinities and depths above the fixed point's range

def _special_clips(rng, T, H, W, blend=False):
    """(label, depth, gray): every placement of tests/nonfinite.py in the middle frame of a clip, and one in every frame"""
    import nonfinite as NF
    depth, gray = _clip(rng, T, H, W, blend=blend)
    for label, where in NF.placements(H * W):
        d = depth.copy()
        d[T // 2] = NF.put(d[T // 2], where)
        yield label, d, gray
    d = depth.copy()
    for t in range(T):
        d[t] = NF.put(d[t], {(7 * t + 1) % (H * W): list(NF.SPECIALS.values())[t % len(NF.SPECIALS)]})
    yield "one per frame", d, gray


def test_vectorised_reference_equals_the_literal_loop_on_specials():
    import nonfinite as NF
    rng = np.random.default_rng(40)
    i = 0
    with NF.cast_warnings_are_errors():
        for label, depth, gray in _special_clips(rng, 4, 2, 5):
            R, tau, fill = (1, 2, 8)[i % 3], (1, 12, 255)[i % 3], (i // 3) % 2
            i += 1
            cut = np.zeros(4, np.uint8)
            cut[3] = i % 4 == 0
            got = TR.filter_clip(depth, gray, R, tau, cut, fill)
            assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= TR.D16_MAX / 16
            assert np.array_equal(got, TR.filter_loops(depth, gray, R, tau, cut, fill)), label


def test_d16_rule_by_hand():
    """valid iff 1 <= rint(16 D), decided on the float; NaN, -inf, -0.0 and a denormal are invalid; above the range saturates"""
    import nonfinite as NF
    with NF.cast_warnings_are_errors():
        got = TR.d16_of(np.float32(list(NF.SPECIALS.values())))
        assert dict(zip(NF.NAMES, got.tolist())) == {"nan+": 0, "nan-": 0, "+inf": 32767, "-inf": 0, "-0.0": 0, "denormal": 0,
                                                      "FLT_MAX": 32767, "2048": 32767, "2047.9375": 32767, "1e9": 32767}
        assert [TR.d16_loop(v) for v in NF.SPECIALS.values()] == got.tolist()
        # a +inf neighbour is an ordinary tap of 32767; a NaN or -inf neighbour has weight 0 and leaves the centre alone
        g = np.zeros((3, 1, 1), np.uint8)
        for v, want in ((np.inf, (2 * (256 * 32767 + 512 * 160 + 256 * 160) + 1024) // 2048), (np.nan, 160), (-np.inf, 160)):
            d = np.float32([v, 10.0, 10.0]).reshape(3, 1, 1)
            assert TR.filter_clip(d, g, 1, 12)[1, 0, 0] * 16 == want, v
        # an invalid centre: filled from its neighbours, or 0 without fill
        d = np.float32([10.0, np.nan, 12.0]).reshape(3, 1, 1)
        assert TR.filter_clip(d, g, 1, 12)[1, 0, 0] == 11.0 and TR.filter_clip(d, g, 1, 12, fill=0)[1, 0, 0] == 0.0


def test_a_nan_bound_makes_the_range_nan_wherever_it_sits_in_the_window():
    import nonfinite as NF
    T = 9
    rng = np.random.default_rng(41)
    base = np.sort(rng.uniform(0, 50, (T, 2)).astype(np.float32), axis=1)
    for R in (0, 1, 2, 8):
        for pos in range(T):
            for cut_at in (None, max(pos - 1, 1), pos, min(pos + 1, T - 1)):
                cut = np.zeros(T, np.uint8)
                if cut_at:
                    cut[cut_at] = 1
                for col, v in ((0, NF.SPECIALS["nan-"]), (1, NF.SPECIALS["nan+"]), (0, NF.SPECIALS["nan+"])):
                    mm = base.copy()
                    mm[pos, col] = v
                    got, clean = TR.ranges(mm, cut, R), TR.ranges(base, cut, R)
                    for t in range(T):
                        lo, hi = TR.admissible(cut, T, t, R)
                        if lo <= pos <= hi:
                            assert np.isnan(got[t]).all(), (R, pos, cut_at, t)
                        else:
                            assert np.array_equal(got[t], clean[t]), (R, pos, cut_at, t)
    # infinities are ordinary extrema
    mm = base.copy()
    mm[4] = (-np.inf, np.inf)
    assert np.array_equal(TR.ranges(mm, np.zeros(T, np.uint8), 1)[3:6], np.float32([[-np.inf, np.inf]] * 3))


def test_normalisation_writes_zero_for_a_nan_or_infinite_range_and_a_nan_sample():
    import nonfinite as NF
    d = np.float32([[0.0, 1.0, 2.5, np.nan, np.inf, -np.inf, 3.4e38, -0.0]])
    with NF.cast_warnings_are_errors():
        for lohi in ((-np.inf, np.inf), (np.nan, 2.0), (0.0, np.nan), (np.inf, np.inf), (0.0, np.inf), (-np.inf, 3.0), (3.0, 1.0), (np.nan, np.nan)):
            assert not TR.to_u16_range(d[None], np.float32([lohi])).any(), lohi
        got = TR.to_u16_range(d[None], np.float32([[0.0, 2.5]]))[0, 0]
        assert got.tolist() == [0, 26214, 65535, 0, 65535, 0, 65535, 0]
        # a frame's own range: one NaN anywhere makes the frame 0, one infinity too (finite pixels 0, the infinite one NaN -> 0)
        for v in (np.nan, np.inf, -np.inf):
            f = np.float32([[1.0, 2.0, v, 4.0]])
            assert not TR.to_u16_range(f[None], TR.minmax(f[None])).any(), v
        assert np.isnan(TR.minmax(np.float32([[[1.0, np.nan]], [[1.0, 2.0]]]))[0]).all()
