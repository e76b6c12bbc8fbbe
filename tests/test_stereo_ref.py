"""The DIBR contract's NumPy restatement (tests/stereo_ref.py) against a literal per-pixel loop and hand-computed answers.
CPU only: the GPU tests (test_stereo_gpu.py) then pin v3d_render_stereo_batch to this restatement bit for bit."""
import numpy as np
import pytest

import stereo_ref as R


def _frame(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("layout", [R.FULL_SBS, R.HALF_SBS])
def test_vectorised_equals_the_loop(layout):
    rng = np.random.default_rng(11)
    for case in range(40):
        H = int(rng.integers(1, 4))
        W = int(rng.integers(1, 24)) * 2
        F = _frame(H, W, case)
        if case % 2:
            D = rng.integers(0, 65536, (H, W)).astype(np.uint16)                     # noise: dense collisions and cracks
        else:                                                                       # piecewise planar
            cut = int(rng.integers(0, W))
            D = np.where(np.arange(W)[None, :] < cut, rng.integers(0, 65536), rng.integers(0, 65536)).astype(np.int64)
            D = np.clip(D + np.arange(W)[None, :] * int(rng.integers(-900, 900)), 0, 65535).astype(np.uint16)
            D = np.repeat(D, H, axis=0)
        gmax = [256, 4096, 1 << 16, (1 << 24) - 1][case % 4]
        gl, gr = int(rng.integers(-gmax, gmax + 1)), int(rng.integers(-gmax, gmax + 1))
        conv = int(rng.choice([0, 65535, int(rng.integers(0, 65536))]))
        want = R.render_loop(F, D, gl, gr, conv, layout)
        got = R.render(F, D, gl, gr, conv, layout)
        assert np.array_equal(got, want), (case, H, W, gl, gr, conv)


def test_zero_gains_give_the_frame_twice():
    F = _frame(5, 33)
    D = np.random.default_rng(1).integers(0, 65536, (5, 33)).astype(np.uint16)
    assert np.array_equal(R.render(F, D, 0, 0, 12345), np.concatenate([F, F], axis=1))


def test_eye_split_zero_keeps_the_left_eye():
    F = _frame(4, 40, 2)
    D = np.random.default_rng(2).integers(0, 65536, (4, 40)).astype(np.uint16)
    gl, gr, conv = R.stereo_gains(48, 0.5, 0.0)
    assert gl == 0 and gr == -48 * 256 and conv == 32768
    out = R.render(F, D, gl, gr, conv)
    assert np.array_equal(out[:, :40], F) and not np.array_equal(out[:, 40:], F)


@pytest.mark.parametrize("s", [3, -5])
def test_constant_depth_is_a_uniform_shift(s):
    W = 20
    F = _frame(2, W, 3)
    D = np.full((2, W), 40000, np.uint16)
    g = s * (1 << 24) // (40000 - 1000)                # g * (d - conv) / 2^24 just below s ...
    while ((g * (40000 - 1000) + (1 << 23)) >> 24) != s:
        g += 1 if s > 0 else -1
    left = R.render(F, D, g, 0, 1000)[:, :W]
    if s > 0:                                          # vacated columns on the left replicate the first scattered one
        want = np.concatenate([np.repeat(F[:, :1], s, axis=1), F[:, :W - s]], axis=1)
    else:
        want = np.concatenate([F[:, -s:], np.repeat(F[:, -1:], -s, axis=1)], axis=1)
    assert np.array_equal(left, want)


def test_near_block_occludes_and_the_background_fills_the_disocclusion():
    """12 pixels, background at depth 0 (= convergence), a near block (65535) at x = 4..6; gain 512 shifts it by
    floor((512 * 65535 + 2^23) / 2^24) = 2 px: right in the left eye, left in the right eye"""
    F = np.zeros((1, 12, 3), np.uint8)
    F[0, :, 0] = np.arange(12) * 10                    # column x has blue 10 x
    D = np.zeros((1, 12), np.uint16)
    D[0, 4:7] = 65535
    out = R.render(F, D, 512, -512, 0)
    left, right = out[0, :12, 0] // 10, out[0, 12:, 0] // 10
    # left eye: the block covers 6..8 (background 6..8 occluded); 4, 5 are a hole between background 3 and the block:
    # the farther side (3) wins
    assert left.tolist() == [0, 1, 2, 3, 3, 3, 4, 5, 6, 9, 10, 11]
    # right eye: the block covers 2..4; the hole 5, 6 sits between the block and background 7: background wins
    assert right.tolist() == [0, 1, 4, 5, 6, 7, 7, 7, 8, 9, 10, 11]
    assert not out[..., 1:].any()


@pytest.mark.parametrize("dc, shift", [(32768, 1), (32767, 0), (-32768, 0), (-32769, -1)])
def test_rounding_edge(dc, shift):
    """g * (D - conv) = 256 * 32768 = 2^23 is exactly half a pixel: rounds up (to +1, and -2^23 to 0)"""
    W = 8
    conv = 32769 if dc < 0 else 0
    d = conv + dc
    F = _frame(1, W, 4)
    D = np.full((1, W), d, np.uint16)
    K = R.eye_keys(D, 256, conv)
    got = [int(k & 0xFFFF) - 1 for k in K[0]]
    assert got == [min(max(t - shift, 0), W - 1) if 0 <= t - shift < W else (0 if shift > 0 else W - 1) for t in range(W)]
    assert np.array_equal(R.render(F, D, 256, 0, conv)[:, W:], F)


def test_shift_beyond_the_width_gives_a_black_row():
    F = _frame(2, 16, 5)
    D = np.full((2, 16), 65535, np.uint16)
    out = R.render(F, D, (1 << 24) - 1, -((1 << 24) - 1), 0)
    assert not out.any()
    half = R.render(F, D, 16 * 256, 0, 0, R.HALF_SBS)                    # left eye: shift 16 px = W -> black; right eye: F
    assert not half[:, :8].any() and half[:, 8:].any()


def test_half_sbs_rounds_half_up():
    F = np.array([[[1, 255, 0], [2, 254, 1], [0, 7, 200], [0, 8, 201]]], np.uint8)
    D = np.zeros((1, 4), np.uint16)
    out = R.render(F, D, 0, 0, 0, R.HALF_SBS)
    assert out.shape == (1, 4, 3)
    assert out[0, :2].tolist() == [[2, 255, 1], [0, 8, 201]] and np.array_equal(out[0, 2:], out[0, :2])
    with pytest.raises(ValueError):
        R.render(_frame(1, 5), np.zeros((1, 5), np.uint16), 0, 0, 0, R.HALF_SBS)


def test_far_key_scene_has_the_gaps_it_promises():
    """the targets nothing lands on, per row and eye, straight from step 1 of the contract"""
    F, D, (gl, gr, conv) = R.far_key_scene()
    assert (gl, gr, conv) == (153600, -153600, 0) and D.shape == (2, 2048)
    x = np.arange(2048)
    def empty(y, g):
        t = x + ((g * (D[y].astype(np.int64) - conv) + (1 << 23)) >> 24)
        return np.setdiff1d(x, t[(t >= 0) & (t < 2048)]).tolist()
    assert empty(0, gl) == list(range(1024, 1624)) and empty(0, gr) == list(range(1448, 2048))
    assert empty(1, gl) == list(range(0, 600)) and empty(1, gr) == list(range(424, 1024))
    left = R.eye_keys(D, gl, conv)
    assert (left[0, 1024:1624] == left[0, 1023]).all()                   # between background 1023 and the block: the farther side
    assert (left[1, :600] == left[1, 600]).all()                         # no left neighbour: the only one
