"""The frame-matching contract on the CPU: the NumPy restatement (tests/framematch_ref.py) against known answers and Python big
integers, and the product's host half (video_3d_pipeline.framematch: zncc, decide -- pure NumPy) against the restatement: every
tie rule, the three statuses, and the recovery of a planted shift on synthetic clips."""
import numpy as np
import pytest

import framematch_ref as FR
from video_3d_pipeline import framematch as FM

DECIDERS = {"restatement": FR.decide, "product": FM.decide}


def _big_scores(a, b):
    a, b = [int(v) for v in a], [int(v) for v in b]
    sa, sb = sum(a), sum(b)
    return (FR.G * sum(x * y for x, y in zip(a, b)) - sa * sb, FR.G * sum(x * x for x in a) - sa * sa,
            FR.G * sum(y * y for y in b) - sb * sb)


def test_constant_frame_is_uninformative():
    flat = np.full((72, 128), 77, np.uint8)
    tex = np.random.default_rng(0).integers(0, 256, (72, 128), dtype=np.uint8)
    s = FR.signature(np.stack([flat, tex]))
    assert (s[0] == 77 * 256).all()
    num, va, vb = FR.scores(s, s)
    assert va[0] == 0 and vb[0] == 0 and va[1] > 0 and (num[0] == 0).all()
    for Z in (FR.zncc(num, va, vb), FM.zncc(num, va, vb)):
        assert np.isnan(Z[0]).all() and np.isnan(Z[:, 0]).all() and Z[1, 1] == 1.0


def test_exact_double_gives_doubled_signatures_and_unit_correlation():
    """128 x 72: every cell is 2 x 2 pixels, so floor(256 * 2S / 4) = 2 * floor(256 * S / 4) and num^2 == var_a * var_b exactly"""
    a = np.random.default_rng(1).integers(0, 128, (72, 128), dtype=np.uint8)
    sa, sb = FR.signature(a), FR.signature((2 * a).astype(np.uint8))
    assert np.array_equal(sb.astype(np.int64), 2 * sa.astype(np.int64))
    num, va, vb = FR.scores(sa[None], sb[None])
    assert int(num[0, 0]) ** 2 == int(va[0]) * int(vb[0]) and num[0, 0] > 0
    assert abs(FM.zncc(num, va, vb)[0, 0] - 1.0) < 1e-15


def test_signature_cells_on_uneven_grids():
    """65 x 37: cells of 1 and 2 pixels per side; the value is the floor of the mean in 8.8 fixed point"""
    g = np.random.default_rng(2).integers(0, 256, (37, 65), dtype=np.uint8)
    s = FR.signature(g).reshape(36, 64)
    for cy, cx in ((0, 0), (35, 63), (17, 31), (35, 0)):
        y0, y1, x0, x1 = cy * 37 // 36, (cy + 1) * 37 // 36, cx * 65 // 64, (cx + 1) * 65 // 64
        cell = g[y0:y1, x0:x1].astype(np.int64)
        assert cell.size in (1, 2, 4) and s[cy, cx] == 256 * int(cell.sum()) // cell.size
    assert FR.signature(np.full((8192, 64), 255, np.uint8)).max() == 65280


def test_headroom_against_big_integers():
    hi = np.full(FR.G, 65280, np.uint16)
    alt = np.where(np.arange(FR.G) % 2 == 0, 0, 65280).astype(np.uint16)
    sigs = np.stack([hi, alt, alt[::-1].copy()])
    num, va, vb = FR.scores(sigs, sigs)
    for i in range(3):
        for j in range(3):
            n, v1, v2 = _big_scores(sigs[i], sigs[j])
            assert (int(num[i, j]), int(va[i]), int(vb[j])) == (n, v1, v2)
    assert FR.G ** 2 * 65280 ** 2 < 2 ** 63 and va[0] == 0 and va[1] == FR.G ** 2 * 65280 ** 2 // 4
    assert int(num[1, 2]) == -int(va[1])                       # the alternating pattern against its mirror: Z = -1 exactly
    assert FM.zncc(num, va, vb)[1, 2] == -1.0


def _probe(values, search, w=4):
    """a probe whose m(d) is exactly values[d + search]: every row carries the same value per shift, all pairs in range"""
    nb = w + 2 * search
    Z = np.full((w, nb), np.nan)
    for a in range(w):
        for d in range(-search, search + 1):
            Z[a, search + a + d] = values[d + search]
    return Z, search


@pytest.mark.parametrize("which", sorted(DECIDERS))
def test_every_tie_rule(which):
    decide = DECIDERS[which]
    S = 2
    # all equal: d = 0 wins (smaller |d|); margin 0 -> undetermined
    r = decide([_probe([.5, .5, .5, .5, .5], S)], S, 0.1, 0.01)
    assert (r["best_shift"], r["status"], r["shift"], r["margin"]) == (0, "undetermined", 0, 0.0)
    # +1 and -1 tie above the rest: the negative one wins
    r = decide([_probe([.2, .7, .3, .7, .1], S)], S, 0.1, 0.0)
    assert r["best_shift"] == -1 and r["probe_shifts"] == [-1] and r["status"] == "refined" and r["shift"] == -1
    # -2 and +1 tie: the smaller |d| wins
    r = decide([_probe([.7, .2, .3, .7, .1], S)], S, 0.1, 0.0)
    assert r["best_shift"] == 1
    # the same rules for M(d) across probes: probe 0 peaks at +2, probe 1 at -2 with equal height -> M ties at +-2 -> -2; the
    # probes disagree with each other -> inconsistent
    r = decide([_probe([.1, .1, .1, .1, .9], S), _probe([.9, .1, .1, .1, .1], S)], S, 0.1, 0.0)
    assert r["best_shift"] == -2 and r["probe_shifts"] == [2, -2] and r["status"] == "inconsistent" and r["shift"] == 0
    # thresholds are inclusive
    r = decide([_probe([.1, .1, .6, .1, .1], S)], S, 0.6, 0.5)
    assert r["status"] == "refined" and r["score"] == 0.6 and r["margin"] == 0.5
    assert decide([_probe([.1, .1, .6, .1, .1], S)], S, 0.61, 0.5)["status"] == "undetermined"
    assert decide([_probe([.1, .1, .6, .1, .1], S)], S, 0.6, 0.51)["status"] == "undetermined"


@pytest.mark.parametrize("which", sorted(DECIDERS))
def test_half_window_rule_and_uninformative_pairs(which):
    decide = DECIDERS[which]
    S, w = 1, 4
    Z, col0 = _probe([.2, .8, .3], S, w)
    Z[0, :] = np.nan                                            # one flat SBS frame: 3 of 4 pairs remain -> still defined
    assert decide([(Z, col0)], S, 0.1, 0.0)["best_shift"] == 0
    Z[1, :] = np.nan
    Z[2, col0 + 2] = np.nan                                     # d = 0 keeps 1 of 4 pairs: undefined; d = -1, +1 keep 2: defined
    r = decide([(Z, col0)], S, 0.1, 0.0)
    assert np.isnan(r["M"][S]) and r["best_shift"] == 1
    # columns outside the 4K clip: col0 = -1 puts d = -1 .. 0 of the first rows off the left edge
    Z2 = np.full((2, 2), 0.5)
    r = decide([(Z2, -1)], S, 0.1, 0.0)
    assert np.isnan(r["M"][0]) and r["M"][1] == 0.5 and r["M"][2] == 0.5      # d=-1: no pair; d=0: 1 of 2; d=+1: 2 of 2
    r = decide([], S, 0.1, 0.0)
    assert (r["status"], r["shift"], r["score"]) == ("undetermined", 0, None)


@pytest.mark.parametrize("which", sorted(DECIDERS))
def test_static_clip_is_undetermined_and_mixed_shifts_are_inconsistent(which):
    decide = DECIDERS[which]
    tex = np.random.default_rng(3).integers(0, 256, (72, 128), dtype=np.uint8)
    left = np.repeat(tex[None], 8, axis=0)
    guide = np.repeat(np.repeat(np.repeat(tex, 2, 0), 2, 1)[None], 16, axis=0)
    sl, sg = FR.signature(left), FR.signature(guide)
    Z = FR.zncc(*FR.scores(sl, sg))
    r = decide([(Z, 4)], 4, 0.5, 0.01)
    assert (r["status"], r["best_shift"], r["shift"]) == ("undetermined", 0, 0) and r["score"] > 0.99 and r["margin"] == 0.0
    # probes built from different shifts
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (20, 72, 128), dtype=np.uint8)
    s = FR.signature(frames)
    probes = []
    for true in (1, -2):
        Zp = FR.zncc(*FR.scores(s[6:10], s[3 - true:13 - true]))    # column c holds frame c + 3 - true
        probes.append((Zp, 3))                                  # so row a (frame 6 + a) meets itself at d = true
    r = decide(probes, 3, 0.5, 0.01)
    assert r["probe_shifts"] == [1, -2] and r["status"] == "inconsistent" and r["shift"] == 0


# (W, H, speed) -> M(d*), margin of the restatement on these clips, measured on the CPU: 256x144 speed 6: 0.9999 / 0.087;
# 256x144 speed 2: 0.9999 / 0.033; 128x72 speed 6: 0.9998 / 0.051; 322x182 speed 6: 0.9860 / 0.097.  The test passes
# min_score = 0.5 and min_margin = 0.01, which the restatement clears with room to spare; the figures are printed, not asserted.
RECOVERY = [(256, 144, 6), (256, 144, 2), (128, 72, 6), (322, 182, 6)]


@pytest.mark.parametrize("W,H,speed", RECOVERY)
def test_recovery_of_a_planted_shift(W, H, speed):
    left, guide = FR.match_clips(W, H, 24, speed=speed, delay=3)
    r = FR.refine_ref(left, guide, 0, search=4, window=12, probes=3, min_score=0.5, min_margin=0.01)
    print(f"{W}x{H} speed {speed}: M(d*) = {r['score']:.4f}, margin = {r['margin']:.4f}, probe shifts {r['probe_shifts']}")
    assert (r["status"], r["shift"], r["best_shift"]) == ("refined", 3, 3) and r["probe_shifts"] == [3, 3, 3]
    # the product's decision on the same integers
    plist = [(FM.zncc(*t), 0 + s - max(0, s - 4)) for t, s in zip(r["ints"], FR.probe_starts(24, 12, 3)[0])]
    p = FM.decide(plist, 4, 0.5, 0.01)
    assert (p["status"], p["shift"], p["probe_shifts"]) == ("refined", 3, [3, 3, 3])
    assert np.allclose(p["M"], r["M"], rtol=0, atol=1e-12, equal_nan=True)
    assert FM.probe_starts(24, 12, 3) == FR.probe_starts(24, 12, 3)
