"""The NumPy restatement of the motion-compensated temporal contract (tests/temporal_mc_ref.py) against itself: the vectorised
forms equal the literal loops, zero fields give tests/temporal_ref.py's filter, a translated texture gives the true vector, the
key has its headroom and the chaining follows a field built by hand."""
import numpy as np
import pytest

import temporal_mc_ref as MR
import temporal_ref as TR


def _clip(rng, T, H, W, shift=(2, -1), noise=4):
    """a textured clip that moves by `shift` per frame plus noise, and a depth with holes"""
    big = rng.integers(0, 256, (H + 8 * T, W + 8 * T)).astype(np.int64)
    big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) // 4
    g = np.stack([big[4 * T + shift[1] * t:4 * T + shift[1] * t + H, 4 * T + shift[0] * t:4 * T + shift[0] * t + W] for t in range(T)])
    g = np.clip(g + rng.integers(-noise, noise + 1, g.shape), 0, 255).astype(np.uint8)
    d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
    d[rng.random((T, H, W)) < 0.2] = 0.0
    return d, g


@pytest.mark.parametrize("T,H,W,S", [(2, 1, 1, 1), (3, 17, 19, 2), (3, 16, 33, 3), (4, 24, 40, 2)])
def test_vectorised_search_equals_the_loops(T, H, W, S):
    rng = np.random.default_rng(W * 31 + H)
    _, g = _clip(rng, T, H, W)
    F, Bk, resid = MR.fields(g, S)
    assert F.shape == Bk.shape == (T,) + MR.blocks(W, H)[::-1] + (2,) and F.dtype == np.int16
    assert not F[T - 1].any() and not Bk[0].any() and resid[0] == 0
    for u in range(T - 1):
        mv, _ = MR.search_loops(g[u], g[u + 1], S)
        assert np.array_equal(F[u], mv), u
        mv, sad = MR.search_loops(g[u + 1], g[u], S)
        assert np.array_equal(Bk[u + 1], mv) and resid[u + 1] == sad.sum(), u
    assert np.abs(F).max() <= S and np.abs(Bk).max() <= S


@pytest.mark.parametrize("T,H,W,S,R,fill", [(3, 17, 19, 2, 1, 1), (4, 24, 40, 2, 2, 0), (4, 9, 37, 3, 8, 1)])
def test_vectorised_filter_equals_the_loops(T, H, W, S, R, fill):
    rng = np.random.default_rng(W + H + R)
    d, g = _clip(rng, T, H, W)
    F, Bk, resid = MR.fields(g, S)
    cut = np.zeros(T, np.uint8)
    cut[T - 1] = T > 3
    got = MR.filter_clip(d, g, R, 12, cut, F, Bk, fill)
    assert np.array_equal(got, MR.filter_loops(d, g, R, 12, cut, F, Bk, fill))
    # and on random fields, which send taps outside the frame
    F2 = rng.integers(-S, S + 1, F.shape).astype(np.int16)
    B2 = rng.integers(-S, S + 1, F.shape).astype(np.int16)
    assert np.array_equal(MR.filter_clip(d, g, R, 12, cut, F2, B2, fill), MR.filter_loops(d, g, R, 12, cut, F2, B2, fill))


def test_zero_fields_give_the_uncompensated_filter():
    rng = np.random.default_rng(3)
    d, g = _clip(rng, 6, 21, 37)
    z = np.zeros((6,) + MR.blocks(37, 21)[::-1] + (2,), np.int16)
    for R, fill, cut_at in ((1, 1, None), (2, 0, 3), (8, 1, 2)):
        cut = np.zeros(6, np.uint8)
        if cut_at:
            cut[cut_at] = 1
        assert np.array_equal(MR.filter_clip(d, g, R, 12, cut, z, z, fill, 1, 4), TR.filter_clip(d, g, R, 12, cut, fill, 1, 4))


@pytest.mark.parametrize("shift", [(3, 0), (-5, 2), (0, -7), (8, 8)])
def test_translated_texture_yields_the_true_vector(shift):
    """frame 1 is frame 0 moved by `shift` without noise: every block whose search window stays inside the frame finds it exactly"""
    rng = np.random.default_rng(11)
    _, g = _clip(rng, 2, 64, 96, shift=shift, noise=0)
    F, Bk, resid = MR.fields(g, 8)
    # content at x in frame 1 was at x + shift in frame 0 (the crop moves by +shift): frame 0 -> 1 is -shift, 1 -> 0 is +shift
    assert (F[0, 1:-1, 1:-1] == (-shift[0], -shift[1])).all()
    assert (Bk[1, 1:-1, 1:-1] == shift).all()
    _, sad = MR.search(g[1], g[0], 8)
    assert not sad[1:-1, 1:-1].any()
    assert list(MR.cuts(resid, 0, 96, 64)) == [0, 1] and list(MR.cuts(resid, 20, 96, 64)) == [0, 0]


def test_key_headroom():
    """the worst cost (a black block against a white frame at the far corner of the largest search) keeps the key below 2^30,
    and the largest rank stays below the key's 8192"""
    assert MR.MAX_COST == 65280 + 64 * 64 and MR.MAX_COST * MR.KEY_SHIFT + MR.KEY_SHIFT - 1 < 1 << 30
    assert (2 * MR.MAX_SEARCH + 1) ** 2 - 1 == 4224 < MR.KEY_SHIFT
    a, b = np.zeros((16, 16), np.uint8), np.full((16, 16), 255, np.uint8)
    mv, sad = MR.search(a, b, 32)
    assert sad[0, 0] == 65280 and tuple(mv[0, 0]) == (0, 0)              # all candidates tie on the SAD: the penalty picks (0,0)
    assert int(MR.penalty(16, 16)[0, 0]) == 64 and int(MR.penalty(1, 1)[0, 0]) == 1 and int(MR.penalty(17, 3)[0, 1]) == 1
    # equal costs: the smallest rank wins, i.e. the smallest dy, then the smallest dx
    flat = np.full((16, 16), 7, np.uint8)
    assert tuple(MR.search(flat, flat, 2)[0][0, 0]) == (0, 0)


def test_chaining_on_a_field_built_by_hand():
    W, H, T = 48, 32, 4                                      # 3 x 2 blocks, centres (8,8) (24,8) (40,8) / (8,24) ...
    F, Bk = np.zeros((T, 2, 3, 2), np.int16), np.zeros((T, 2, 3, 2), np.int16)
    F[0, 0, 0] = (16, 0)                                     # block (0,0): one block to the right ...
    F[1, 0, 1] = (10, 16)                                    # ... then from block (1,0): right and one block down ...
    F[2, 1, 2] = (30, 30)                                    # ... then from block (2,1) (centre 8+26 = 34 -> block 2; 8+16 = 24 -> row 1)
    F[1, 0, 0] = (-3, -3)                                    # what a chain that did not follow the motion would read
    m = [MR.chain(F, Bk, 0, u, W, H)[0, 0] for u in range(T)]
    assert [tuple(v) for v in m] == [(0, 0), (16, 0), (26, 16), (56, 46)]
    # the position is clamped to the frame before the block is looked up: (8+56, 8+46) -> (47, 31) -> block (2,1)
    F2 = np.concatenate([F, np.zeros((1, 2, 3, 2), np.int16)])
    F2[3, 1, 2] = (1, 2)
    assert tuple(MR.chain(F2, np.zeros_like(F2), 0, 4, W, H)[0, 0]) == (57, 48)
    # backward: Bk_t, then Bk_{t-1} where the block went
    Bk[3, 1, 2] = (-20, -16)                                 # block (2,1), centre (40,24) -> (20, 8): block (1,0)
    Bk[2, 0, 1] = (-1, 5)
    Bk[2, 1, 2] = (9, 9)
    m = [tuple(MR.chain(F, Bk, 3, u, W, H)[1, 2]) for u in (3, 2, 1)]
    assert m == [(0, 0), (-20, -16), (-21, -11)]
    # clipped blocks take the clamped centre: W = 20 -> block 1 is 4 px wide, centre min(24, 19) = 19
    Fc = np.zeros((2, 1, 2, 2), np.int16)
    Fc[0, 0, 1] = (-4, 0)
    assert tuple(MR.chain(Fc, Fc, 0, 1, 20, 10)[0, 1]) == (-4, 0)


def test_vectorised_filter_equals_the_loops_on_specials():
    """NaN, infinities and depths above the fixed point's range, at the centre and carried in by displaced loads; no astype of a
    non-finite value anywhere (the NumPy warning is an error here)"""
    import nonfinite as NF
    rng = np.random.default_rng(50)
    T, H, W, S = 4, 18, 21, 2
    d, g = _clip(rng, T, H, W)
    F = rng.integers(-S, S + 1, (T,) + MR.blocks(W, H)[::-1] + (2,)).astype(np.int16)
    Bk = rng.integers(-S, S + 1, F.shape).astype(np.int16)
    z = np.zeros_like(F)
    cut = np.zeros(T, np.uint8)
    vals = list(NF.SPECIALS.values())
    with NF.cast_warnings_are_errors():
        for k, (label, where) in enumerate([(n, {int(rng.integers(H * W)): v, 0: v, H * W - 1: v}) for n, v in NF.SPECIALS.items()]
                                           + [("all", {int(i): vals[j % len(vals)] for j, i in enumerate(rng.choice(H * W, 60, replace=False))})]):
            dd = d.copy()
            dd[1 + k % 2] = NF.put(dd[1 + k % 2], where)
            R, fill = (1, 2, 8)[k % 3], k % 2
            got = MR.filter_clip(dd, g, R, 12, cut, F, Bk, fill)
            assert np.isfinite(got).all()
            assert np.array_equal(got, MR.filter_loops(dd, g, R, 12, cut, F, Bk, fill)), label
            assert np.array_equal(MR.filter_clip(dd, g, R, 12, cut, z, z, fill), TR.filter_clip(dd, g, R, 12, cut, fill)), label
