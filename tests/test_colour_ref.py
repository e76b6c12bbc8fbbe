"""tests/colour_ref.py against itself: the vectorised forms against the loops that walk pixels and levels one by one, tables
worked out by hand, and the monotonicity the header promises.  lut_cases() is also what tests/test_colour_gpu.py runs on the device."""
import numpy as np
import pytest

import colour_ref as CR

M = (1 << 32) - 1


def _h(n=1):
    return np.zeros((n, 3, 256), np.uint64)


def _ident():
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def lut_cases():
    """-> [(name, hist_src, hist_dst, group, expected u8 [tables,3,256] or None)]; counts as uint64 below 2^32"""
    cases = []
    # both a single level: nothing of the source lies below 40, so Cs = 0 there and the smallest u with Cf[u] Ns >= 0 is 0;
    # from 40 on Cs = Ns and the first u with Cf[u] = Nf is 200
    s, d = _h(), _h()
    s[0, :, 40], d[0, :, 200] = 10, 7
    want = np.zeros((1, 3, 256), np.uint8)
    want[0, :, 40:] = 200
    cases.append(("single-level", s, d, 1, want))
    # identical histograms: an occupied level maps to itself (C[v - 1] < C[v]); an empty one has the C of the last occupied level
    # below it and maps there (the smallest u with C[u] >= C[v]); below the first occupied level C = 0 and the answer is 0
    s = _h()
    occ = [3, 4, 100, 101, 255]
    for c in range(3):
        s[0, c, occ] = [5, 1, 9, 2, 4 + c]
    want = np.zeros((1, 3, 256), np.uint8)
    for v in range(256):
        below = [u for u in occ if u <= v]
        want[0, :, v] = below[-1] if below else 0
    cases.append(("identical", s, s.copy(), 1, want))
    # an empty source, an empty target, both: the identity, per channel (channel 1 here has both and is matched)
    s, d = _h(), _h()
    s[0, 0, 17], d[0, 2, 99] = 4, 6
    s[0, 1, 8], d[0, 1, 80] = 2, 2
    want = np.stack([_ident()])
    want[0, 1, :8], want[0, 1, 8:] = 0, 80
    cases.append(("empty", s, d, 1, want))
    # an exact tie: Cs = (1, 2) of 2, Cf = 2 at level 10 and 4 at level 20 of 4: level 0 asks for Cf[u] * 2 >= 1 * 4, met with
    # equality at u = 10 (a strict compare would give 20)
    s, d = _h(), _h()
    s[0, :, 0], s[0, :, 1], d[0, :, 10], d[0, :, 20] = 1, 1, 2, 2
    want = np.zeros((1, 3, 256), np.uint8)
    want[0, :, 0], want[0, :, 1:] = 10, 20
    cases.append(("tie", s, d, 1, want))
    # counts of 2^32 - 1 over three frames: totals near 2^35, products near 2^69
    s, d = _h(3), _h(3)
    s[:, :, 10], s[:, :, 20], s[:, :, 30] = M, np.array([M, M, 5], np.uint64)[:, None], np.array([7, M, 1], np.uint64)[:, None]
    d[:, :, 40], d[:, :, 50], d[:, :, 60] = np.array([M, 3, M], np.uint64)[:, None], M, np.array([11, M, M], np.uint64)[:, None]
    cases.append(("wide", s, d, 3, None))
    # groups: 1, n, and one that does not divide n
    rng = np.random.default_rng(5)
    s, d = rng.integers(0, 1000, (5, 3, 256)).astype(np.uint64), rng.integers(0, 50, (5, 3, 256)).astype(np.uint64)
    d[:, :, :30] = 0
    for g in (1, 5, 2):
        cases.append((f"group{g}", s, d, g, None))
    return cases


def _lut_wrapped64(hs, hd):
    """one table over all frames with the two products taken modulo 2^64: what a 64-bit compare would build"""
    out = np.zeros((3, 256), np.uint8)
    for c in range(3):
        Cs = np.cumsum(hs[:, c].astype(object).sum(axis=0))
        Cf = np.cumsum(hd[:, c].astype(object).sum(axis=0))
        for v in range(256):
            u = 0
            while u < 255 and (Cf[u] * Cs[255]) % (1 << 64) < (Cs[v] * Cf[255]) % (1 << 64):
                u += 1
            out[c, v] = u
    return out


@pytest.mark.parametrize("case", lut_cases(), ids=lambda c: c[0])
def test_tables(case):
    name, s, d, group, want = case
    got = CR.lut(s, d, group)
    assert got.shape == (-(-s.shape[0] // group), 3, 256) and got.dtype == np.uint8
    assert np.array_equal(got, CR.lut_loop(s, d, group)), name
    if want is not None:
        assert np.array_equal(got, want), name
    assert (np.diff(got.astype(int), axis=2) >= 0).all(), f"{name}: not monotone"


def test_wide_counts_need_the_128_bit_compare():
    _, s, d, group, _ = next(c for c in lut_cases() if c[0] == "wide")
    exact = CR.lut(s, d, group)[0]
    assert int(s[:, 0].astype(object).sum()) * int(d[:, 0].astype(object).sum()) > 1 << 64
    assert not np.array_equal(exact, _lut_wrapped64(s, d)), "a wrapped 64-bit product builds the same table: the case shows nothing"
    # by hand: Cs = 3M, 5M + 5, 6M + 13 of Ns = 6M + 13; Cf = 2M + 3 at 40, 5M + 3 at 50, Nf = 7M + 14 at 60
    Ns, Nf = 6 * M + 13, 7 * M + 14
    for v, Cs in ((10, 3 * M), (20, 5 * M + 5), (30, Ns)):
        u = next(u for u, Cf in ((40, 2 * M + 3), (50, 5 * M + 3), (60, Nf)) if Cf * Ns >= Cs * Nf)
        assert (exact[:, v] == u).all()


def test_groups_are_the_tables_of_their_frames():
    _, s, d, _, _ = next(c for c in lut_cases() if c[0] == "group2")
    got = CR.lut(s, d, 2)
    for j, (a, b) in enumerate(((0, 2), (2, 4), (4, 5))):
        assert np.array_equal(got[j], CR.lut(s[a:b], d[a:b], b - a)[0])
    for bad in (0, 6):
        with pytest.raises(ValueError):
            CR.lut(s, d, bad)


def test_monotone_on_random_histograms():
    rng = np.random.default_rng(0)
    for k in range(20):
        s = rng.integers(0, [3, 1000, M][k % 3], (2, 3, 256)).astype(np.uint64)
        d = rng.integers(0, [1000, 2, M][k % 3], (2, 3, 256)).astype(np.uint64)
        s[:, :, rng.integers(0, 256, 100)] = 0
        t = CR.lut(s, d, 2)
        assert (np.diff(t.astype(int), axis=2) >= 0).all()


@pytest.mark.parametrize("rect", [None, (0, 0, 1, 1), (2, 1, 9, 4), (10, 4, 11, 5)])
def test_histogram_and_apply_against_their_loops(rect):
    rng = np.random.default_rng(3)
    F = rng.integers(0, 256, (2, 5, 11, 3), dtype=np.uint8)
    h = CR.hist(F, rect)
    assert h.dtype == np.uint32 and np.array_equal(h, CR.hist_loop(F, rect))
    x0, y0, x1, y1 = rect or (0, 0, 11, 5)
    assert (h.sum(axis=2) == (x1 - x0) * (y1 - y0)).all()
    for t in (rng.integers(0, 256, (3, 256), dtype=np.uint8), rng.integers(0, 256, (2, 3, 256), dtype=np.uint8)):
        got = CR.apply(F, t, rect)
        assert np.array_equal(got, CR.apply_loop(F, t, rect))
        outside = np.ones(F.shape, bool)
        outside[:, y0:y1, x0:x1] = False
        assert np.array_equal(got[outside], F[outside])
    for bad in ((0, 0, 12, 5), (3, 0, 3, 5), (-1, 0, 4, 4), (0, 2, 4, 2)):
        with pytest.raises(ValueError):
            CR.hist(F, bad)


def test_matching_undoes_a_monotone_grading():
    """a frame, its graded copy: the table graded -> original puts every pixel back to within the levels the grading merged"""
    from video_3d_pipeline import synthetic as syn
    L, _ = syn.stereo_pair(96, 54, 0)
    G = CR.grade(L)
    t = CR.lut(CR.hist(G[None]), CR.hist(L[None]), 1)
    back = CR.apply(G[None], t)[0]
    assert np.abs(back.astype(int) - L.astype(int)).mean() < 0.25 * np.abs(G.astype(int) - L.astype(int)).mean()
