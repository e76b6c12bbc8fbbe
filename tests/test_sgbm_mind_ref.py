"""tests/sgbm_mind_ref.py (the minDisparity contract in NumPy) held to np_sgm and to the C oracle, the scene that motivates the
window, and the rule behind --min-disparity auto.  CPU only."""
import numpy as np
import pytest

import np_sgm
import sgbm_mind_ref as ref
from conftest import textured_pair

W, H = 200, 12


@pytest.fixture(scope="module")
def pair():
    return textured_pair(W, H, seed=77)


def test_m0_equals_np_sgm_and_the_oracle(oracle, pair):
    L, R = pair
    assert np.array_equal(ref.cost_volume(L, R, 0), np_sgm.cost_volume(L, R))
    assert np.array_equal(ref.cost_volume(L, R, 0), oracle.cost_volume(L, R))
    r0 = ref.raw(L, R, 0)
    S = np_sgm.aggregate(np_sgm.cost_volume(L, R))
    assert np.array_equal(r0, np_sgm.wta(S, W))
    assert np.array_equal(r0, oracle.sgbm_raw(L, R))
    assert np.array_equal(ref.finish(r0, 0, oracle), oracle.sgbm_compute(L, R))
    assert np.array_equal(ref.raw(L, R, 0, mode=1), oracle.sgbm_raw(L, R, oracle.default_params(mode=1)))


@pytest.mark.parametrize("m", [-1, -2, -17, -32, -62])
def test_identity_with_the_oracle(oracle, pair, m):
    """the window [m, m + 64) on (L, R) is the window [0, 64) on (L', R), L'(x) = L(x + m), once the columns that become L''s
    right border carry what the border rule gives them; without that band the two differ, so the test sees the rule"""
    L, R = pair
    Lb = ref.band_left(L, m)
    want = ref.from_oracle(oracle.sgbm_raw, Lb, R, m)
    got = ref.raw(Lb, R, m)
    assert np.array_equal(got, want)
    assert (got[:, :ref.D + m] == ref.invalid(m)).all() and (got[:, W + m:] == ref.invalid(m)).all()
    assert (got[:, ref.D + m:W + m] != ref.invalid(m)).mean() > 0.3
    n_diff = int((ref.raw(L, R, m) != ref.from_oracle(oracle.sgbm_raw, L, R, m)).sum())
    print(f"m={m}: {n_diff} pixels differ without the band")
    assert n_diff > 0


@pytest.mark.parametrize("m", [-63, -64])
def test_left_border_columns_are_the_restatement_alone(oracle, pair, m):
    """at m = -63 and -64 the left image's border column 0 (record = ftzero) is read: the shifted image cannot express it"""
    L, R = pair
    C = ref.cost_volume(L, R, m)
    Lb = ref.band_left(L, m)
    assert not np.array_equal(ref.cost_volume(Lb, R, m), oracle.cost_volume(ref.shift_left(Lb, m), R))
    assert C.shape == (H, W - 64, 64) and C.min() >= 2400 and C.max() <= 2400 + 25 * 93
    got = ref.raw(L, R, m)
    assert (got[:, W + m:] == ref.invalid(m)).all() and (got[:, :ref.D + m] == ref.invalid(m)).all()


def test_behind_screen_scene_needs_the_negative_window(oracle):
    """background at -20, object at +6: the share of pixels within one pixel of the truth at m = -32 is at least three times the
    share at m = 0"""
    L, R, truth = ref.behind_screen_pair()
    s0 = ref.share_within_one(ref.compute(L, R, 0, oracle), truth, 0)
    s32 = ref.share_within_one(ref.compute(L, R, -32, oracle), truth, -32)
    print(f"share within one pixel: m=0 {s0:.3f}, m=-32 {s32:.3f}")
    assert s32 >= 3 * s0 and s32 > 0.5


def test_auto_rule():
    from video_3d_pipeline.depth import MIN_DISPARITY_CANDIDATES, choose_min_disparity
    assert MIN_DISPARITY_CANDIDATES == (0, -16, -32, -48, -64)
    pick = lambda *s: choose_min_disparity(dict(zip(MIN_DISPARITY_CANDIDATES, s)))
    assert pick(560, 600, 1638, 1473, 863) == -32                   # the behind-screen scene of the issue
    assert pick(2011, 2016, 1848, 1400, 256) == 0                   # constant +12: 0 is within 2 % of the best
    assert pick(0, 0, 0, 0, 0) == 0                                 # nothing comparable anywhere
    assert pick(5, 5, 5, 5, 5) == 0 and pick(1, 7, 7, 7, 7) == -16  # ties go to the candidate nearest 0
    assert pick(98, 100, 0, 0, 0) == 0 and pick(97, 100, 0, 0, 0) == -16      # 100 * score >= 98 * best, integers
    assert pick(979, 0, 0, 0, 1000) == -64 and pick(980, 0, 0, 0, 1000) == 0
    assert pick(0, 0, 0, 0, 1) == -64
    assert choose_min_disparity({-64: 10, 0: 10, -32: 10}) == 0     # the order of the keys does not matter
