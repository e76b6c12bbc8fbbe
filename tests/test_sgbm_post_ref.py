"""tests/sgbm_post_ref.py (the record-level reference of the L-R check and the median) held to what exists, on the CPU: on the small
pairs of tests/test_oracle.py, in both SGM modes, it agrees bit for bit with np_sgm.wta + median and with the C oracle's pre-speckle
output for minDisparity 0, and with tests/sgbm_mind_ref.py for a negative minDisparity; on random records its vectorised key
minimum agrees with a per-pixel loop, and what the never-written columns hold does not move it."""
import numpy as np
import pytest

import np_sgm
import sgbm_mind_ref as M
import sgbm_post_ref as P
from conftest import textured_pair


@pytest.mark.parametrize("W,H,seed,max_disp", [(82, 7, 5, 15), (90, 5, 3, 20)])
@pytest.mark.parametrize("mode,dirs", [(0, np_sgm.DIRS5), (1, np_sgm.DIRS8)])
def test_three_ways_to_the_pre_speckle_plane_agree(oracle, mode, dirs, W, H, seed, max_disp):
    from scipy.ndimage import median_filter
    L, R = textured_pair(W, H, seed, max_disp=max_disp)
    S = np_sgm.aggregate(np_sgm.cost_volume(L, R), dirs=dirs)
    rec = P.records(S, W)
    assert P.in_domain(rec) and np.count_nonzero(rec) > rec[:, 64:].size // 4
    raw = oracle.sgbm_raw(L, R, oracle.default_params(mode=mode))
    assert np.array_equal(P.lrcheck(rec), np_sgm.wta(S, W).astype(np.int16))
    assert np.array_equal(P.lrcheck(rec), raw)
    got = P.lrcheck_median(rec)
    assert np.array_equal(got, median_filter(np_sgm.wta(S, W).astype(np.int16), size=3, mode="nearest"))
    assert np.array_equal(got, oracle.median3x3(raw))
    assert np.array_equal(got, oracle.sgbm_compute(L, R, oracle.default_params(mode=mode, speckleWindowSize=0)))


@pytest.mark.parametrize("m", [-1, -2, -31, -64])
@pytest.mark.parametrize("mode,dirs", [(0, np_sgm.DIRS5), (1, np_sgm.DIRS8)])
def test_a_negative_min_disparity_agrees_with_the_contract(oracle, mode, dirs, m):
    W, H = 84, 6
    L, R = M.window_pair(W, H, 7, m)
    S = np_sgm.aggregate(M.cost_volume(L, R, m), dirs=dirs)
    rec = P.records(S, W)
    assert P.in_domain(rec)
    raw = M.raw(L, R, m, mode)
    assert np.array_equal(P.lrcheck(rec, 1, m), raw)
    assert np.array_equal(P.lrcheck_median(rec, 1, m), M.finish(raw, m, oracle, speckle_window=0))


CASES = {"plain": {}, "few-costs": {"few_costs": True}, "best63": {"best63_at_64": True}, "subpix": {"subpix_extremes": True},
         "empty-rows": {"empty_rows": (0, 3)}, "all-rejected": {"reject": 1.0}}


@pytest.mark.parametrize("case", CASES)
def test_random_records_the_loop_and_the_vectorised_key_minimum_agree(case):
    rng = np.random.default_rng(len(case))
    W, H = 150, 5
    rec = P.random_records(rng, W, H, **CASES[case])
    assert P.in_domain(rec)
    k = P.keys(rec)
    assert np.array_equal(k, P.keys_loop(rec))
    if case == "best63":
        assert np.all(k[:, 1] != P.NONE) and np.all(k[:, 0] == P.NONE)     # column 1 is the leftmost target any source reaches
    if case == "few-costs":
        hits = np.zeros(rec.shape, np.int64)
        v, _, _, best = P.fields(rec)
        ys, xs = np.nonzero(v)
        np.add.at(hits, (ys, xs - best[ys, xs]), 1)
        assert (hits > 2).sum() > 20                            # targets with several sources among four costs: ties happen
    rel = P.lrcheck_rel(rec, 1)
    valid = P.fields(rec)[0][:, 64:]
    if case == "all-rejected":
        assert np.all(rel == -16)
    elif case != "empty-rows":
        kept = (rel[:, 64:] != -16).sum()
        assert 0 < kept < valid.sum()                           # the check both passes and rejects
    # what columns [0, 64) hold moves nothing
    for garbage in (0xA5A5A5A5, 0xFFFFFFFF, P.word(5, 16 * 63, 63)):
        dirty = rec.copy()
        dirty[:, :64] = garbage
        assert np.array_equal(P.lrcheck_median(dirty, 1, -31), P.lrcheck_median(rec, 1, -31))
