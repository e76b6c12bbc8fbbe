"""tests/tb_ref.py against itself: the NumPy restatement of the top-bottom split and the oracle's horizontal split on the transposed
frame are two statements of one arithmetic and must agree byte for byte; the borders and the seam behave as the header says."""
import numpy as np
import pytest

import tb_ref

SIZES = [(2, 5), (4, 7), (8, 64), (18, 33), (46, 322)]        # H x W


@pytest.mark.parametrize("H,W", SIZES)
def test_restatement_equals_the_transposed_oracle(oracle, H, W):
    tb = tb_ref.content(1, H, W, 7 * H + W)[0]
    for got, want, name in zip(tb_ref.split(tb, True), tb_ref.split_by_transposition(tb), ("left", "right")):
        assert got.shape == (H, W, 3) and np.array_equal(got, want), name
    for got, want, name in zip(tb_ref.to_gray(tb, True), tb_ref.to_gray_by_transposition(tb), ("left gray", "right gray")):
        assert got.shape == (H, W) and np.array_equal(got, want), name
    assert (tb_ref.split(tb, True)[0] == 255).any() and (tb_ref.split(tb, True)[1] == 0).any()      # the saturation is reached


def test_plain_split_is_the_rows(oracle):
    tb = tb_ref.content(1, 18, 33, 3)[0]
    L, R = tb_ref.split(tb, False)
    assert np.array_equal(L, tb[:9]) and np.array_equal(R, tb[9:])
    gl, gr = tb_ref.to_gray(tb, False)
    assert np.array_equal(gl, oracle.bgr_to_gray(tb[:9])) and np.array_equal(gr, oracle.bgr_to_gray(tb[9:]))


def test_a_single_row_eye_is_returned_twice(oracle):
    """H = 2: every tap reads the eye's one row, and the taps sum to 2048"""
    assert int(oracle.lanczos4_taps(0.75).sum()) == 2048 and int(oracle.lanczos4_taps(0.25).sum()) == 2048
    tb = np.random.default_rng(5).integers(0, 256, (2, 5, 3), dtype=np.uint8)
    L, R = tb_ref.split(tb, True)
    assert np.array_equal(L, np.stack([tb[0], tb[0]])) and np.array_equal(R, np.stack([tb[1], tb[1]]))


def test_nothing_leaks_across_the_seam(oracle):
    """a top eye that ends in 255 rows over a bottom eye that starts with 0 rows: every row, the ones nearest the seam included,
    is what the eye gives when it is processed alone (over a copy of itself, so the other half cannot matter)"""
    H, W = 24, 16
    tb = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    tb[H // 2 - 4:H // 2] = 255
    tb[H // 2:H // 2 + 4] = 0
    L, R = tb_ref.split(tb, True)
    alone_top = tb_ref.split(np.concatenate([tb[:H // 2], tb[:H // 2]]), True)
    alone_bottom = tb_ref.split(np.concatenate([tb[H // 2:], tb[H // 2:]]), True)
    assert np.array_equal(L, alone_top[0]) and np.array_equal(L, alone_top[1])
    assert np.array_equal(R, alone_bottom[0]) and np.array_equal(R, alone_bottom[1])
    assert (L[-1] == 255).all() and (R[0] == 0).all()             # the window of the last / first output row holds one value only
