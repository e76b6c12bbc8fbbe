"""The hole-filling contract (tests/fill_ref.py): the vectorised reference against the literal loop, hand-computed answers and
the properties the header states.  CPU only."""
import numpy as np
import pytest

import fill_ref as FR

I = -16          # the matcher's invalid value


def random_frame(rng, H, W, rate, hole_values=(-16, -1, -32768), empty_rows=True):
    d = rng.integers(0, 1024, (H, W)).astype(np.int16)
    d[rng.random((H, W)) < 0.05] = 0                                    # zeros are valid disparities
    holes = rng.random((H, W)) < rate
    d[holes] = rng.choice(np.array(hole_values, np.int16), int(holes.sum()))
    if empty_rows:
        for y in np.flatnonzero(rng.random(H) < 0.3):
            d[y] = rng.choice(np.array(hole_values, np.int16), W)
    return d


@pytest.mark.parametrize("rate", [0.1, 0.5, 0.9, 1.0])
def test_vectorised_equals_the_literal_loop(rate):
    rng = np.random.default_rng(int(rate * 100))
    for _ in range(100):
        H, W = int(rng.integers(1, 9)), int(rng.integers(1, 41))
        d = random_frame(rng, H, W, rate)
        want = FR.fill_frame_loops(d)
        got = FR.fill_frame(d)
        assert got.dtype == np.int16 and np.array_equal(got, want), f"{H}x{W} rate {rate}\n{d}\n{got}\n{want}"


def test_one_row_strip_by_hand():
    d = np.array([[I, I, 40, I, I, 24, -1, 56, I, 8, I, I]], np.int16)
    want = np.array([[40, 40, 40, 24, 24, 24, 24, 56, 8, 8, 8, 8]], np.int16)
    assert np.array_equal(FR.fill_frame(d), want)
    assert np.array_equal(FR.fill_frame_loops(d), want)


def test_equal_neighbours_and_zero_is_valid():
    d = np.array([[32, I, I, 32, I, 0, I, 7]], np.int16)
    want = np.array([[32, 32, 32, 32, 0, 0, 0, 7]], np.int16)
    assert np.array_equal(FR.fill_frame(d), want)
    assert np.array_equal(FR.fill_frame_loops(d), want)


def test_the_input_row_decides_not_the_filled_one():
    """a hole's neighbours are the nearest NON-HOLE pixels of the input: a long run takes one value, not a cascade"""
    d = np.array([[100, I, I, I, I, 20, I, I, 60]], np.int16)
    want = np.array([[100, 20, 20, 20, 20, 20, 20, 20, 60]], np.int16)
    assert np.array_equal(FR.fill_frame(d), want)


def test_an_empty_row_between_two_rows_takes_the_one_above():
    d = np.array([[5, I, 9],
                  [I, I, I],
                  [7, 7, I]], np.int16)
    want = np.array([[5, 5, 9],
                     [5, 5, 9],
                     [7, 7, 7]], np.int16)
    assert np.array_equal(FR.fill_frame(d), want)
    assert np.array_equal(FR.fill_frame_loops(d), want)


def test_empty_rows_take_the_nearest_row():
    d = np.full((6, 2), I, np.int16)
    d[1] = (3, I)
    d[5] = (I, 11)
    want = np.array([[3, 3], [3, 3], [3, 3], [3, 3], [11, 11], [11, 11]], np.int16)      # row 3: |3-1| = |3-5| -> above
    assert np.array_equal(FR.fill_frame(d), want)
    assert np.array_equal(FR.fill_frame_loops(d), want)


def test_an_all_invalid_frame_is_unchanged():
    d = np.array([[I, -1], [-32768, I]], np.int16)
    assert np.array_equal(FR.fill_frame(d), d)
    assert np.array_equal(FR.fill_frame_loops(d), d)


def test_properties():
    rng = np.random.default_rng(7)
    for _ in range(200):
        H, W = int(rng.integers(1, 9)), int(rng.integers(1, 41))
        d = random_frame(rng, H, W, float(rng.choice([0.1, 0.5, 0.9])))
        out = FR.fill_frame(d)
        assert np.array_equal(FR.fill_frame(out), out), "not idempotent"
        assert np.array_equal(out[d >= 0], d[d >= 0]), "a valid pixel changed"
        if (d >= 0).any():
            assert (out >= 0).all(), "a hole survived although the frame has a valid pixel"
        else:
            assert np.array_equal(out, d)


def test_batches_are_filled_frame_by_frame():
    rng = np.random.default_rng(3)
    d = np.stack([random_frame(rng, 5, 17, 0.5) for _ in range(3)])
    d[1] = I
    out = FR.fill(d)
    assert out.shape == d.shape and out.dtype == np.int16
    for f in range(3):
        assert np.array_equal(out[f], FR.fill_frame(d[f]))
    with pytest.raises(ValueError):
        FR.fill_frame(d[0].astype(np.int32))
