"""The speckle filter and the stand-alone median of csrc/v3d_sgbm_post.hip themselves, without a GPU: v3d_filter_speckles and
sgbm_speckles (what run_sgbm calls, here with every plane of a size as one batch) run in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal oracle.filter_speckles bit for
bit: the planes of test_speckle_run_lists_extremes and every figure of tests/speckle_shapes.py that fits, under three thresholds.
The image ends on its heap block's last byte and starts 0, 2 or 8 bytes off a 16-byte boundary, the workspace (exactly
3 W H frames int32, its content after the call free) 0 or 4 bytes off one: k_ccl_runs' vector path and k_ccl_vmerge's 16-byte path
are each taken and each refused.  The workspace starts out as positive numbers -- far outside it in one configuration, random
indices into a frame in the other -- so that a stale run-list entry behind an end marker, if used, is a sanitizer report or a
wrong plane.  One fiber runs at a time: the union-find's races are the GPU test's part (test_speckle_merge_shapes)."""
import numpy as np
import pytest

import emu_case as E
import sgbm_post_emu as X
import speckle_shapes as SS

driver = X.fixture()
SIZES = [(1, 5), (257, 1), (64, 9), (300, 40), (516, 19), (640, 33), (64, 16), (64, 17), (72, 48)]
SKEWS = [(0, 0), (8, 0), (2, 0), (0, 4), (8, 4), (2, 4)]           # image, workspace: bytes off a 16-byte boundary
VEC_RUNS = lambda W, si, sw: W % 4 == 0 and si % 8 == 0 and sw % 16 == 0   # k_ccl_runs' `vec`, restated
VEC_MERGE = lambda W, si: W % 8 == 0 and si % 16 == 0                     # k_ccl_vmerge's 16-byte path


def _thresholds(H):
    return [(100, 512), (H, 100), (3, 1)]


def _planes(W, H, max_size, max_diff):
    planes = dict(SS.extremes(W, H))
    planes.update(SS.shapes(W, H, max_size, max_diff))
    return planes


def _ws(gp, n, W, H):
    """3 n W H int32, positive: huge in one configuration, indices into a frame in the other"""
    if gp == 0xA5:
        return np.full(3 * n * W * H, 0x7F7F7F7F, np.int32).view(np.uint8)
    return np.random.default_rng(W + H).integers(0, W * H, 3 * n * W * H).astype(np.int32).view(np.uint8)


def _i16(a):
    return np.ascontiguousarray(a, np.int16).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("W,H", SIZES)
def test_filter_speckles_single_frames(driver, tmp_path, oracle, W, H):
    k = 0
    for max_size, max_diff in _thresholds(H):
        for name, img in _planes(W, H, max_size, max_diff).items():
            si, sw = SKEWS[k % len(SKEWS)]
            k += 1
            want = oracle.filter_speckles(img, -16, max_size, max_diff)
            make = lambda gp: [E.exact("img", _i16(img), si, expect=_i16(want)), W, H, -16, max_size, max_diff,
                               E.exact("ws", _ws(gp, 1, W, H), sw, expect=None), 0]
            try:
                E.run_configs(driver, tmp_path, X.FILTER, make)
            except AssertionError as e:
                raise AssertionError(f"{name} size<={max_size} diff<={max_diff} skews {si}, {sw}: {e}") from None


@pytest.mark.parametrize("W,H", SIZES)
def test_the_handles_speckle_stage_on_a_batch(driver, tmp_path, oracle, W, H):
    """the handle takes speckleRange: maxDiff = 16 speckleRange, so the thresholds here are (100, 512) and (3, 16)"""
    for k, (max_size, rng16) in enumerate(((100, 32), (3, 1))):
        si, sw = SKEWS[(SIZES.index((W, H)) + 3 * k) % len(SKEWS)]
        planes = _planes(W, H, max_size, 16 * rng16)
        imgs = np.stack(list(planes.values())[::-1] if k else list(planes.values()))
        assert len(imgs) >= 2
        want = np.stack([oracle.filter_speckles(p, -16, max_size, 16 * rng16) for p in imgs])
        assert not np.array_equal(want, imgs)
        n = len(imgs)
        E.run_configs(driver, tmp_path, X.SPECKLES, lambda gp: [E.exact("img", _i16(imgs), si, expect=_i16(want)), n, W, H, 0, max_size, rng16,
                                                                 E.exact("ws", _ws(gp, n, W, H), sw, expect=None), 0])


def test_a_window_of_zero_switches_the_stage_off(driver, tmp_path):
    img = SS.extremes(64, 9)["sparse"]
    E.run_configs(driver, tmp_path, X.SPECKLES, lambda gp: [E.exact("img", _i16(img), 0), 1, 64, 9, 0, 0, 32, E.exact("ws", _ws(gp, 1, 64, 9), 0), 0])


def test_both_vector_paths_are_taken_and_refused():
    """test_filter_speckles_single_frames hands the skews round its planes: every size (but the two one-pixel-wide or -high ones,
    which have five planes a threshold) meets each of them"""
    seen = set()
    for W, H in SIZES:
        assert len(_planes(W, H, 100, 512)) >= (len(SKEWS) if min(W, H) > 1 else 5)
        for si, sw in SKEWS:
            seen |= {("runs", VEC_RUNS(W, si, sw), si, sw), ("merge", VEC_MERGE(W, si), si)}
    assert {("runs", True, 0, 0), ("runs", True, 8, 0), ("runs", False, 2, 0), ("runs", False, 0, 4), ("merge", True, 0), ("merge", False, 8), ("merge", False, 2)} <= seen
    assert any(W % 4 == 0 and W % 8 for W, _ in SIZES) and any(W % 4 for W, _ in SIZES)       # 516: runs' path without merge's; 257, 1


@pytest.mark.parametrize("W,H", [(1, 1), (2, 3), (257, 5)])
@pytest.mark.parametrize("skew", [0, 2])
def test_median3x3(driver, tmp_path, W, H, skew):
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(W + H)
    img = (rng.integers(-1, 64, (H, W)) * 16).astype(np.int16)
    want = median_filter(img, size=3, mode="nearest")
    E.run_configs(driver, tmp_path, X.MEDIAN, lambda gp: [E.exact("src", _i16(img), skew), W, H,
                                                          E.exact("dst", np.full(2 * W * H, gp, np.uint8), skew, expect=_i16(want)), 0])
