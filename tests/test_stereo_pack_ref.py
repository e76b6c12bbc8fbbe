"""tests/stereo_pack_ref.py against itself: the vectorised packings equal the literal per-pixel loop, codes 0 / 1 equal the two
older restatements, and the answers that can be worked out by hand."""
import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_ref as R
import stereo_sub_ref as S

SIZES = [(1, 1), (1, 2), (7, 3), (6, 4)]                      # W x H


def _allowed(packing, W, H):
    return not (packing == P.HALF_SBS and W % 2) and not (packing == P.HALF_TB and H % 2)


@pytest.mark.parametrize("packing", P.PACKINGS)
@pytest.mark.parametrize("W,H", SIZES)
def test_vectorised_equals_loop(W, H, packing):
    rng = np.random.default_rng(100 * W + 10 * H + packing)
    EL, ER = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    if not _allowed(packing, W, H):
        with pytest.raises(ValueError):
            P.pack(EL, ER, packing)
        return
    got = P.pack(EL, ER, packing)
    assert got.shape == P.output_size(packing, W, H)[::-1] + (3,) and got.dtype == np.uint8
    assert np.array_equal(got, P.pack_loop(EL, ER, packing))


def test_extreme_eyes_equal_loop():
    """0 and 255 in every combination of the six Dubois inputs: the clamp on both sides"""
    v = np.array(np.meshgrid(*[[0, 255]] * 6, indexing="ij"), np.uint8).reshape(6, -1).T           # 64 x 6
    EL, ER = v[None, :, :3].copy(), v[None, :, 3:].copy()
    assert np.array_equal(P.pack(EL, ER, P.ANAGLYPH_DUBOIS), P.pack_loop(EL, ER, P.ANAGLYPH_DUBOIS))


@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("layout", [P.FULL_SBS, P.HALF_SBS])
def test_codes_0_and_1_are_the_older_contracts(layout, subpixel):
    W, H = 38, 5
    F = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    D = S.scene_depth("planar", H, W, 4)
    gl, gr, conv = R.stereo_gains(24.0, 0.4, 0.5)
    want = (S.render if subpixel else R.render)(F, D, gl, gr, conv, layout)
    assert np.array_equal(P.render(F, D, gl, gr, conv, layout, subpixel), want)


def test_unknown_packing_and_mismatched_inputs_are_refused():
    F, D = np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2), np.uint16)
    for bad in (-1, 7):
        with pytest.raises(ValueError):
            P.render(F, D, 0, 0, 0, bad)
    with pytest.raises(ValueError):
        P.render(F, D[:1], 0, 0, 0, P.FULL_TB)


@pytest.mark.parametrize("subpixel", [False, True])
def test_zero_gains_return_the_frame(subpixel):
    """nothing moves: both eyes are the frame, and every W x H packing of two equal opaque eyes is the frame.  Half top-bottom
    averages row pairs, so its frame has equal rows in each pair; Dubois keeps greys only, so its frame is grey"""
    W, H = 6, 4
    rng = np.random.default_rng(5)
    F = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    D = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    EL, ER = P.eyes(F, D, 0, 0, 32768, subpixel)
    assert np.array_equal(EL, F) and np.array_equal(ER, F)
    for packing in (P.ROWS, P.ANAGLYPH_COLOUR):
        assert np.array_equal(P.render(F, D, 0, 0, 32768, packing, subpixel), F)
    pairs = np.repeat(F[0::2], 2, axis=0)
    assert np.array_equal(P.render(pairs, D, 0, 0, 32768, P.HALF_TB, subpixel),
                          np.concatenate([pairs[0::2], pairs[0::2]], axis=0))
    grey = np.repeat(F[..., :1], 3, axis=2)
    assert np.array_equal(P.render(grey, D, 0, 0, 32768, P.ANAGLYPH_DUBOIS, subpixel), grey)
    assert np.array_equal(P.render(F, D, 0, 0, 32768, P.FULL_TB, subpixel), np.concatenate([F, F], axis=0))


def test_half_tb_is_the_row_pair_average():
    EL = np.array([[[0, 1, 255]], [[1, 2, 255]], [[10, 20, 30]], [[11, 23, 30]]], np.uint8)      # 1 x 4
    ER = 255 - EL
    want = np.array([[[1, 2, 255]], [[11, 22, 30]], [[255, 254, 0]], [[245, 234, 225]]], np.uint8)
    assert np.array_equal(P.pack(EL, ER, P.HALF_TB), want)


def test_rows_take_the_left_eye_first():
    EL, ER = np.full((5, 2, 3), 10, np.uint8), np.full((5, 2, 3), 200, np.uint8)
    assert P.pack(EL, ER, P.ROWS)[:, 0, 0].tolist() == [10, 200, 10, 200, 10]


def test_anaglyph_colour_channels():
    EL, ER = np.array([[[1, 2, 3]]], np.uint8), np.array([[[4, 5, 6]]], np.uint8)
    assert P.pack(EL, ER, P.ANAGLYPH_COLOUR).tolist() == [[[4, 5, 3]]]


def test_dubois_rows_sum_to_one():
    assert P.DUBOIS.sum(axis=1).tolist() == [65536, 65536, 65536]


def test_dubois_keeps_every_grey():
    g = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(P.pack(g, g, P.ANAGLYPH_DUBOIS), g)


def test_dubois_by_hand():
    white, black = np.full((1, 1, 3), 255, np.uint8), np.zeros((1, 1, 3), np.uint8)
    assert P.dubois_unclamped(white, black).tolist() == [[[-11, -24, 289]]]                      # B', G', R'
    assert P.pack(white, black, P.ANAGLYPH_DUBOIS).tolist() == [[[0, 0, 255]]]
    red = np.array([[[0, 0, 255]]], np.uint8)
    assert int(P.pack(red, black, P.ANAGLYPH_DUBOIS)[0, 0, 2]) == 116                            # (29891 * 255 + 32768) >> 16
