"""tests/quality_ref.py holds itself to its own contract on the CPU: the vectorised forms against the literal per-pixel loops, the
hand-computed row of its docstring, and the extremes of both measures against Python integers."""
import numpy as np
import pytest

import quality_ref as QR


def _case(H, W, seed, n=1):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    d = rng.integers(-40, 16 * W + 40, (n, H, W)).astype(np.int16)
    d[rng.random((n, H, W)) < 0.2] = -16
    d[rng.random((n, H, W)) < 0.1] = 0
    return L, R, d


@pytest.mark.parametrize("H,W,seed", [(1, 1, 0), (3, 7, 1), (5, 33, 2), (2, 65, 3)])
def test_reproj_vectorised_equals_the_loop(H, W, seed):
    L, R, d = _case(H, W, seed)
    d[0, 0, 0] = 32767
    for thr in (0, 16, 255):
        assert QR.reproj_frame(L[0], R[0], d[0], thr).tolist() == QR.reproj_loops(L[0], R[0], d[0], thr)
    assert np.array_equal(QR.reproj(L, R, d, 16)[0], QR.reproj_frame(L[0], R[0], d[0], 16))


@pytest.mark.parametrize("T,H,W,seed", [(2, 1, 1, 0), (3, 4, 9, 1), (5, 3, 17, 2)])
def test_flicker_vectorised_equals_the_loop(T, H, W, seed):
    rng = np.random.default_rng(seed)
    depth = (rng.integers(-8, 1024, (T, H, W)) / 16).astype(np.float32)
    depth[rng.random((T, H, W)) < 0.1] = np.nan
    depth[0, 0, 0] = 0.03125                                   # 16 D = 0.5 -> rint 0 (half to even): invalid
    gray = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-6, 7, (T, H, W)), 0, 255).astype(np.uint8)
    for still, jump in ((0, 0), (4, 16), (255, 32767)):
        assert QR.flicker(depth, gray, still, jump).tolist() == QR.flicker_loops(depth, gray, still, jump)


def test_the_hand_computed_row():
    L, R = np.array([[10, 20, 30, 40]], np.uint8), np.array([[12, 24, 36, 48]], np.uint8)
    d = np.array([[16, 8, -16, 40]], np.int16)
    want = [3, 2, 384, 124928, 2, 192, 20480, 2]
    assert QR.reproj_frame(L, R, d, 1).tolist() == want == QR.reproj_loops(L, R, d, 1)
    assert dict(zip(QR.REPROJ_FIELDS, want))["ssd0"] == 64 ** 2 + 128 ** 2


def test_all_4080_extreme():
    """L = 255, R = 0, d = 16 everywhere: every compared pixel has e = e0 = 4080; column 0 is valid but out of view"""
    H, W = 6, 50
    L, R, d = np.full((H, W), 255, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 16, np.int16)
    n = H * (W - 1)
    want = [H * W, n, QR.E_MAX * n, QR.E_MAX ** 2 * n, n, QR.E_MAX * n, QR.E_MAX ** 2 * n, n]
    assert QR.reproj_frame(L, R, d, 254).tolist() == want
    want[4] = want[7] = 0
    assert QR.reproj_frame(L, R, d, 255).tolist() == want      # e > 16 * 255 never holds
    assert QR.E_MAX ** 2 == 16646400 and (2 ** 32 - 1) // QR.E_MAX ** 2 == 258
    assert 8192 * 65535 * QR.E_MAX ** 2 < 2 ** 53


def test_32766_jump_extreme():
    """d16 jumping 1 <-> 32767 under a luma step of 255 with still = 255: every pixel is still and moves 32766"""
    H, W = 4, 11
    depth = np.empty((3, H, W), np.float32)
    depth[0::2], depth[1] = 1 / 16, 32767 / 16
    gray = np.zeros((3, H, W), np.uint8)
    gray[1] = 255
    n = H * W
    assert QR.flicker(depth, gray, 255, 32765).tolist() == [[255 * n, n, 32766 * n, n]] * 2
    assert QR.flicker(depth, gray, 255, 32766).tolist() == [[255 * n, n, 32766 * n, 0]] * 2
    assert QR.flicker(depth, gray, 254, 0).tolist() == [[255 * n, 0, 0, 0]] * 2


def test_identical_frames_and_invalid_depth():
    rng = np.random.default_rng(5)
    depth = (rng.integers(-4, 300, (1, 5, 9)) / 16).astype(np.float32).repeat(3, axis=0)
    depth[:, 0, :3] = np.nan
    gray = rng.integers(0, 256, (1, 5, 9), dtype=np.uint8).repeat(3, axis=0)
    nv = int((QR.d16_of(depth[0]) >= 1).sum())
    assert 0 < nv < 45 and QR.flicker(depth, gray, 0, 0).tolist() == [[0, nv, 0, 0]] * 2
    assert QR.d16_of(np.array([np.nan, -1.0, 0.03125, 0.09375, 0.1], np.float32)).tolist() == [0, 0, 0, 2, 2]


def test_flicker_vectorised_equals_the_loop_on_specials():
    """NaN of both signs, infinities and depths above the fixed point's range: NaN and -inf are invalid, +inf and the like
    count as 32767 (tests/temporal_ref.py d16_of); no astype of a non-finite value (the NumPy warning is an error here)"""
    import nonfinite as NF
    rng = np.random.default_rng(9)
    T, H, W = 4, 3, 17
    depth = (rng.integers(-8, 1024, (T, H, W)) / 16).astype(np.float32)
    gray = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-6, 7, (T, H, W)), 0, 255).astype(np.uint8)
    with NF.cast_warnings_are_errors():
        for label, where in NF.placements(H * W):
            d = depth.copy()
            d[1] = NF.put(d[1], where)
            for still, jump in ((0, 0), (4, 16), (255, 32766)):
                assert QR.flicker(d, gray, still, jump).tolist() == QR.flicker_loops(d, gray, still, jump), label
        assert QR.d16_of(np.float32(list(NF.SPECIALS.values()))).tolist() == [0, 0, 32767, 0, 0, 0, 32767, 32767, 32767, 32767]
        # +inf next to 1/16 on still luma: one still pixel that moves 32766
        d = np.float32([1 / 16, np.inf, -np.inf, np.nan]).reshape(4, 1, 1)
        assert QR.flicker(d, np.zeros((4, 1, 1), np.uint8), 0, 32765).tolist() == [[0, 1, 32766, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
