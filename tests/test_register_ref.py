"""The NumPy restatement of the spatial registration entries (tests/register_ref.py) against brute force: sums, an exact rational
evaluation of the profile integral and the bin means, a per-pixel loop for the warp, and the rounding of the host's conversions
to Q16."""
from fractions import Fraction

import numpy as np
import pytest

import register_ref as RR

Q = RR.Q


def test_profiles_are_the_plane_sums():
    g = np.random.default_rng(0).integers(0, 256, (3, 37, 53), dtype=np.uint8)
    g[2] = 255
    col, row = RR.profiles(g)
    assert col.dtype == row.dtype == np.uint32 and col.shape == (3, 53) and row.shape == (3, 37)
    assert np.array_equal(col, g.astype(np.uint64).sum(axis=1)) and np.array_equal(row, g.astype(np.uint64).sum(axis=2))
    assert (col[2] == 255 * 37).all() and (row[2] == 255 * 53).all()


def _integral_exact(P, p):
    """the integral of the step function P from 0 to p / 65536 samples, times 65536"""
    x, total, i = Fraction(int(p), Q), Fraction(0), 0
    while i + 1 <= x:
        total += int(P[i])
        i += 1
    if i < len(P):
        total += (x - i) * int(P[i])
    return total * Q


def test_integral_and_bin_means_against_rationals():
    """a 23-sample profile, bins = 8, a 31-sample target: I(p) is exact (an integer), the bin mean its floor"""
    rng = np.random.default_rng(1)
    P = rng.integers(0, 1 << 21, 23).astype(np.uint32)
    pos = np.concatenate([[0, 1, 65535, 65536, 65537, 23 * Q - 1, 23 * Q], rng.integers(0, 23 * Q + 1, 200)])
    got = RR.integral(P, pos)
    for p, g in zip(pos, got):
        assert Fraction(int(g)) == _integral_exact(P, p), p
    t = RR.edges(31, 8)
    assert [int(v) for v in t] == [(j * 31 * Q) // 8 for j in range(9)] and t[-1] == 31 * Q
    for a, b in ((RR.rhu(Fraction(23 * Q, 31)) - 1, 0), (40000, 3 * Q + 17), (50000, -2 * Q - 5), (RR.A_MIN, 22 * Q), (RR.A_MAX, -Q)):
        s = ((a * t) >> 16) + b
        m, ok = RR.bin_means(P, s[None, :])
        for j in range(8):
            lo, hi = int(s[j]), int(s[j + 1])
            valid = lo >= 0 and hi <= 23 * Q
            assert bool(ok[0, j]) == valid
            if valid:
                exact = (_integral_exact(P, hi) - _integral_exact(P, lo)) / (hi - lo)
                assert int(m[0, j]) == exact.__floor__(), (a, b, j)


def test_match_record_against_a_loop():
    rng = np.random.default_rng(2)
    A, B = rng.integers(0, 1 << 21, (2, 23)).astype(np.uint32), rng.integers(0, 1 << 21, (2, 31)).astype(np.uint32)
    cand = np.array([(RR.rhu(Fraction(23 * Q, 31)) - 1, 0), (40000, 3 * Q + 17), (48000, -2 * Q), (RR.A_MIN, 30 * Q), (RR.A_MAX, 0)], dtype=np.int64)
    got = RR.match_scores(A, B, cand, 8)
    t = [(j * 31 * Q) // 8 for j in range(9)]
    for k in range(2):
        for c, (a, b) in enumerate(cand.tolist()):
            s = [((a * tj) >> 16) + b for tj in t]
            mean = lambda P, lo, hi: ((_integral_exact(P, hi) - _integral_exact(P, lo)) / (hi - lo)).__floor__()
            rec = [0] * 6
            for j in range(7):
                if s[j] >= 0 and s[j + 2] <= 23 * Q:
                    da = mean(A[k], s[j + 1], s[j + 2]) - mean(A[k], s[j], s[j + 1])
                    db = mean(B[k], t[j + 1], t[j + 2]) - mean(B[k], t[j], t[j + 1])
                    for i, v in enumerate((1, da, db, da * db, da * da, db * db)):
                        rec[i] += v
            assert got[k, c].tolist() == rec, (k, c)
    assert got[0, 0, 0] == 7 and got[0, 3, 0] == 0 and 0 < got[0, 2, 0] < 7
    with pytest.raises(ValueError):
        RR.match_scores(A, B, [(RR.A_MIN - 1, 0)], 8)
    with pytest.raises(ValueError):
        RR.match_scores(A, B, [(Q, RR.B_MAX + 1)], 8)


def test_wrapping_match_is_the_record_below_the_headroom_and_wraps_above():
    """match_scores_wrapping (Python integers, reduced mod 2^64 at the end) on the in-headroom inputs of tests/test_register_gpu.py,
    and one record worked out by hand: alternating 0 / 2^32 - 1 under the identity has da = db = +-(2^32 - 1) in all 7 pairs, each
    square is 2^64 - 2^33 + 1, each product of the two its negative"""
    import test_register_gpu as G
    for na, nb, bins in ((23, 31, 8), (256, 512, 8), (256, 512, 512)):
        cand = G._candidates(na, nb)
        for kind, kind_b in (("random", "random"), ("top", "top"), ("top", "random"), ("alt", "alt")):
            a, b = G._profiles(2, na, na + bins, kind), G._profiles(2, nb, nb + 7 * bins, kind_b)
            assert np.array_equal(RR.match_scores_wrapping(a, b, cand, bins), RR.match_scores(a, b, cand, bins)), (na, nb, bins, kind)
    alt = G._profiles(1, 8, 0, "alt32")
    assert alt.tolist() == [[0, 0xFFFFFFFF] * 4]
    rec = RR.match_scores_wrapping(alt, alt, [(Q, 0)], 8)[0, 0].tolist()
    assert rec == [7, (1 << 32) - 1, (1 << 32) - 1, 7 * (1 - (1 << 33)), 7 * (1 - (1 << 33)), 7 * (1 - (1 << 33))]
    assert RR.match_scores_wrapping(alt, 0xFFFFFFFF - alt, [(Q, 0)], 8)[0, 0, 3] == -7 * (1 - (1 << 33))


def test_zncc_from_the_six_sums():
    da, db = np.array([3, -4, 10, 0, 7]), np.array([6, -8, 21, 1, 13])
    rec = np.array([len(da), da.sum(), db.sum(), (da * db).sum(), (da * da).sum(), (db * db).sum()])
    assert abs(RR.zncc(rec, 8)[()] - np.corrcoef(da, db)[0, 1]) < 1e-12
    assert np.isnan(RR.zncc(rec, 12)[()])                                         # fewer than bins / 2 pairs
    assert np.isnan(RR.zncc(np.array([5, 10, 3, 6, 20, 9]), 8)[()])               # da constant: no variance
    assert np.isnan(RR.zncc(np.array([-1, 0, 0, 0, 0, 0]), 8)[()])                # the in-band refusal


def _warp_loop(s, ax, bx, ay, by, fill, Wo, Ho):
    n, Hs, Ws = s.shape
    out = np.zeros((n, Ho, Wo), np.uint16)
    for f in range(n):
        for y in range(Ho):
            for x in range(Wo):
                u, v = ax * x + bx, ay * y + by
                if not (0 <= u <= (Ws - 1) * Q and 0 <= v <= (Hs - 1) * Q):
                    out[f, y, x] = fill
                    continue
                i0, j0 = u >> 16, v >> 16
                i1, j1, fx, fy = min(i0 + 1, Ws - 1), min(j0 + 1, Hs - 1), (u >> 8) & 255, (v >> 8) & 255
                p = [[int(s[f, j, i]) for i in (i0, i1)] for j in (j0, j1)]
                out[f, y, x] = ((256 - fy) * ((256 - fx) * p[0][0] + fx * p[0][1]) + fy * ((256 - fx) * p[1][0] + fx * p[1][1]) + 32768) >> 16
    return out


def test_warp_against_a_pixel_loop():
    s = np.random.default_rng(3).integers(0, 65536, (2, 5, 7)).astype(np.uint16)
    s[0, 0, 0] = 65535
    for m in ((RR.rhu(Fraction(7 * Q, 9)), -Q // 3, RR.rhu(Fraction(5 * Q, 4)), -Q // 5), (Q, Q // 2, Q, Q // 2), (RR.A_MIN, 0, RR.A_MAX, -Q),
              (Q, 7 * Q, Q, 0), (50000, -123456, 70000, 54321)):
        assert np.array_equal(RR.warp(s, *m, 77, 9, 4), _warp_loop(s, *m, 77, 9, 4)), m


def test_warp_special_cases():
    s = np.random.default_rng(4).integers(0, 65536, (2, 5, 7)).astype(np.uint16)
    s[1] = 65535
    assert np.array_equal(RR.warp(s, Q, 0, Q, 0, 9, 7, 5), s)                     # the identity is a bit copy
    last = RR.warp(s, Q, 6 * Q, Q, 0, 9, 1, 5)                                    # u == (Ws - 1) * 65536 exactly: the last column
    assert np.array_equal(last[:, :, 0], s[:, :, 6])
    assert (RR.warp(s, Q, 6 * Q + 1, Q, 0, 9, 1, 5) == 9).all()                   # one Q16 unit beyond it: fill
    assert (RR.warp(s, Q, -1, Q, 0, 9, 1, 5) == 9).all()
    assert np.array_equal(RR.warp(s, Q, 0, Q, 4 * Q, 9, 7, 1)[:, 0], s[:, 4]) and (RR.warp(s, Q, 0, Q, 4 * Q + 1, 9, 7, 1) == 9).all()


def test_host_conversions_round_half_up():
    assert [RR.rhu(Fraction(v, 2)) for v in (-3, -1, 0, 1, 3)] == [-1, 0, 0, 1, 2]
    assert RR.map_to_q16(1.0, 0.0, 1920, 1920) == (Q, 0)                           # the identity at the exact-2x grid
    assert RR.map_to_q16(1.0, 0.0, 960, 1920) == (Q // 2, -Q // 4)                 # (xo + 1/2) / 2 - 1/2
    A, B = 0.875, 0.0625
    ax, bx = RR.map_to_q16(A, B, 144, 144)
    assert (ax, bx) == (57344, RR.rhu(Q * (Fraction(7, 16) + 9 - Fraction(1, 2))))
    assert RR.map_to_q16(0.1 + 0.2, 1e-3, 1080, 1080) == RR.map_to_q16(Fraction(0.1 + 0.2), Fraction(1e-3), 1080, 1080)   # floats are exact rationals
    assert RR.candidate(0, 23 * Q, 31) == (RR.rhu(Fraction(23 * Q, 31)), 0) and RR.candidate(-5, 7 * Q + 2, 2) == (RR.rhu(Fraction(7 * Q + 7, 2)), -5)
    a, b = RR.candidate(3 * Q, 250 * Q, 512)
    An, Bn = RR.normalised(a, b, 256, 512)
    assert An == a * 512 / (Q * 256) and Bn == 3 / 256
