"""The robust depth range contract on CPU: tests/range_ref.py's vectorised form against a literal per-pixel loop, the two
properties the contract implies, and every edge case the contract names."""
import numpy as np
import pytest

import range_ref as RR
import temporal_ref as TR

QS = (5000, 9000, 9800, 9999, 10000)


def _frames():
    rng = np.random.default_rng(0)
    out = {}
    d = (rng.integers(1, 1024, (9, 13)) / 16.0).astype(np.float32)
    d[rng.random(d.shape) < 0.2] = 0.0
    out["stereo"] = d
    out["blend"] = np.where(rng.random((7, 11)) < 0.1, 0.0, rng.uniform(0.0, 64.0, (7, 11))).astype(np.float32)
    out["negatives"] = rng.uniform(-3.0, 20.0, (5, 8)).astype(np.float32)
    out["outliers"] = np.where(rng.random((16, 16)) < 0.01, 57.5, rng.integers(16, 320, (16, 16)) / 16.0).astype(np.float32)
    out["saturating"] = (rng.integers(0, 4000, (6, 9)) / 16.0).astype(np.float32)
    out["one pixel"] = np.float32([[12.5]])
    return out


@pytest.mark.parametrize("q", QS)
def test_vectorised_form_equals_the_loop(q):
    for name, f in _frames().items():
        got = RR.robust_minmax(f[None], q)[0]
        want = RR.white_point_loops(f, q)
        assert got.dtype == np.float32 and got[0] == want[0] and got[1] == want[1], (name, q, got, want)
        hist = RR.histogram(f)
        assert hist[0] == 0 and hist.sum() == (TR.d16_of(f) >= 1).sum() and len(hist) == RR.NB


@pytest.mark.parametrize("q", QS)
def test_at_most_the_stated_share_lies_above_the_white_point(q):
    for name, f in _frames().items():
        n_valid, k, _ = RR.select(RR.histogram(f), q)
        mn, hi = RR.robust_minmax(f[None], q)[0]
        assert hi >= mn
        assert RR.above(f, hi) <= n_valid - k, (name, q)
        assert (n_valid - k) * 10000 <= n_valid * (10000 - q), (name, q)          # n_valid - k <= n_valid (1 - q / 10000), exactly


def test_off_returns_the_maximum_on_fixed_point_depths():
    rng = np.random.default_rng(1)
    for trial in range(20):
        d = (rng.integers(0, 2047, (3, 10, 12)) / 16.0).astype(np.float32)
        d[:, 0, 0] = (0.0, 2046 / 16.0, 1 / 16.0)
        d[2, 1:] = 0.0
        assert np.array_equal(RR.robust_minmax(d, 10000), TR.minmax(d))
        assert np.array_equal(RR.to_u16(d, 10000), TR.to_u16_range(d, TR.minmax(d)))


def test_rank_is_exact_in_64_bits():
    assert RR.rank_of(5000, 1) == 1 and RR.rank_of(5000, 2) == 1 and RR.rank_of(5000, 3) == 2
    assert RR.rank_of(9800, 100) == 98 and RR.rank_of(9801, 100) == 99 and RR.rank_of(10000, 7) == 7
    n = 2 ** 32 - 1
    assert RR.rank_of(9999, n) == -(-9999 * n // 10000) and RR.rank_of(10000, n) == n       # q n needs more than 32 bits
    assert RR.rank_of(5000, 0) == 1


def test_ties_round_half_to_even():
    # 16 D an odd multiple of 1/2: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 (invalid), 1.5 -> 2
    f = np.float32([[2.5 / 16, 3.5 / 16, 0.5 / 16, 1.5 / 16]])
    hist = RR.histogram(f)
    assert hist[2] == 2 and hist[4] == 1 and hist.sum() == 3
    assert RR.robust_minmax(f[None], 5000)[0][1] == np.float32(2 / 16)            # k = 2: the second of (2, 2, 4)
    assert RR.robust_minmax(f[None], 10000)[0][1] == np.float32(4 / 16)           # the bin's value, not the float max 3.5/16


def test_all_invalid_frame():
    for v in (0.0, -1.0, 0.03):                                                     # 0.03 * 16 rounds to 0
        f = np.full((4, 5), v, np.float32)
        for q in QS:
            mn, hi = RR.robust_minmax(f[None], q)[0]
            assert mn == hi == np.float32(v)
        assert not RR.to_u16(f[None], 9800).any()                                   # hi == lo -> 0
    f = np.float32([[0.0, -2.0, 0.0]])
    assert tuple(RR.robust_minmax(f[None], 9800)[0]) == (np.float32(-2.0), np.float32(0.0))


def test_constant_frame():
    f = np.full((6, 7), 7.25, np.float32)
    for q in QS:
        assert tuple(RR.robust_minmax(f[None], q)[0]) == (np.float32(7.25), np.float32(7.25))
    assert not RR.to_u16(f[None], 9800).any()
    g = np.full((6, 7), 7.26, np.float32)                                           # the bin's value 7.25 lies below the min: hi = mn
    assert tuple(RR.robust_minmax(g[None], 9800)[0]) == (np.float32(7.26), np.float32(7.26))


def test_one_valid_pixel():
    f = np.zeros((5, 5), np.float32)
    f[2, 3] = 33.0
    for q in QS:
        assert tuple(RR.robust_minmax(f[None], q)[0]) == (np.float32(0.0), np.float32(33.0))     # k = 1 whatever q is
    u = RR.to_u16(f[None], 5000)[0]
    assert u[2, 3] == 65535 and u.sum() == 65535


def test_saturating_values():
    f = np.zeros((10, 10), np.float32)
    f[:5] = 200.0                                                                   # d16 = 3200: the last bin
    f[5:] = 10.0
    assert RR.histogram(f)[RR.NB - 1] == 50
    assert tuple(RR.robust_minmax(f[None], 5000)[0]) == (np.float32(10.0), np.float32(10.0))     # k = 50: the 10.0 bin; max(., mn)
    assert tuple(RR.robust_minmax(f[None], 5001)[0]) == (np.float32(10.0), np.float32(200.0))    # k = 51: the last bin -> mx
    f[0, 0] = 2047 / 16.0                                                           # exactly the last bin's lower edge
    f[0, 1] = 2046 / 16.0
    h = RR.histogram(f)
    assert h[RR.NB - 1] == 49 and h[RR.NB - 2] == 1
    f[:5] = 2046 / 16.0                                                             # the largest value that does not saturate
    assert RR.robust_minmax(f[None], 10000)[0][1] == np.float32(2046 / 16.0)


def test_blend_like_frame_in_one_bin():
    rng = np.random.default_rng(3)
    f = (np.float32(20.0) + rng.uniform(-0.03, 0.03, (8, 9))).astype(np.float32)    # every value rounds to d16 = 320
    assert set(TR.d16_of(f).reshape(-1)) == {320}
    for q in QS:
        mn, hi = RR.robust_minmax(f[None], q)[0]
        assert mn == f.min() and hi == max(np.float32(20.0), f.min())
        assert RR.above(f, hi) == 0
    u = RR.to_u16(f[None], 9800)[0]                                                 # values above hi clamp to 65535, nothing wraps
    assert u.max() == 65535 and u.min() == 0


def test_stabilize_with_the_option_off_is_the_temporal_contract():
    rng = np.random.default_rng(4)
    depth = (rng.integers(0, 1024, (7, 6, 9)) / 16.0).astype(np.float32)
    gray = rng.integers(0, 256, (7, 6, 9)).astype(np.uint8)
    assert np.array_equal(RR.stabilize(depth, gray, 2, q=10000), TR.stabilize(depth, gray, 2))
    assert (RR.stabilize(depth, gray, 2, q=9000) != TR.stabilize(depth, gray, 2)).any()
    with pytest.raises(ValueError):
        RR.robust_minmax(depth, 4999)


# ---------------------------------------------------------------- NaN, infinities and depths above the fixed point's range

@pytest.mark.parametrize("q", (5000, 9800, 10000))
def test_vectorised_form_equals_the_loop_on_specials(q):
    import nonfinite as NF
    with NF.cast_warnings_are_errors():
        for name, f in _frames().items():
            for label, where in NF.placements(f.size):
                g = NF.put(f, where)
                got, want = RR.robust_minmax(g[None], q)[0], np.float32(RR.white_point_loops(g, q))
                assert NF.same_floats(got, want), (name, label, q, got, want)
                if np.isnan(g).any():
                    assert np.isnan(got).all(), (name, label)
                    assert not RR.to_u16(g[None], q).any()
                hist = RR.histogram(g)
                assert hist[0] == 0 and hist.sum() == (TR.d16_of(g) >= 1).sum()


def test_specials_in_the_histogram_by_hand():
    import nonfinite as NF
    f = np.float32([[1.0, 2.0, 3.0, 4.0]])
    with NF.cast_warnings_are_errors():
        # NaN -> 0 (not counted), and the frame's range is (NaN, NaN) whatever the NaN's sign
        for v in (NF.SPECIALS["nan+"], NF.SPECIALS["nan-"]):
            g = NF.put(f, {2: v})
            assert RR.histogram(g).sum() == 3 and np.isnan(RR.robust_minmax(g[None], 9800)).all()
        # -inf, -0.0 and a denormal are invalid and ordinary minima; +inf and everything from 2047/16 up land in the last bin
        for v, mn in ((-np.inf, -np.inf), (-0.0, 0.0), (1e-45, 1e-45)):
            g = NF.put(f, {0: v})
            assert RR.histogram(g).sum() == 3 and RR.robust_minmax(g[None], 10000)[0].tolist() == [np.float32(mn), 4.0]
        for v in (np.inf, NF.FLT_MAX, 1e9, 2048.0, 2047.9375):
            g = NF.put(f, {3: v})
            assert RR.histogram(g)[RR.NB - 1] == 1
            assert RR.robust_minmax(g[None], 10000)[0].tolist() == [1.0, np.float32(v)]          # hi16 == 2047 -> the float max
            assert RR.robust_minmax(g[None], 5000)[0].tolist() == [1.0, 2.0]                     # below the outlier: the percentile
