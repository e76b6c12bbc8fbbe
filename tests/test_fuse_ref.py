"""tests/fuse_ref.py against itself: the vectorised form against the literal loop, and the properties the contract promises (a
constant eye takes P, the identity returns E, both clamps saturate, every sample of the populated range owns a target).  No GPU."""
import numpy as np
import pytest

import fuse_ref as F
import stereo_source_ref as X

# (ax, bx, ay, by): a general map with both lower clamps, one sample per target, the smallest scales with an upper clamp in x and
# a lower one in y, and scales just under one sample per target
MAPS = [(14500, -70000, 25000, 3000), (65536, 0, 65536, 0), (4096, 1 << 20, 4096, -(1 << 18)), (60000, 123456, 30000, -99999)]


def _case(seed, W, H, We, Hs):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (Hs, 2 * We, 3), dtype=np.uint8)


@pytest.mark.parametrize("m", MAPS)
@pytest.mark.parametrize("eye", [0, 1])
def test_vectorised_equals_loop(m, eye):
    for seed, (W, H, We, Hs) in enumerate([(13, 9, 5, 4), (23, 7, 16, 6), (5, 3, 2, 2), (31, 17, 3, 9)]):
        E, sbs = _case(seed, W, H, We, Hs)
        assert np.array_equal(F.fuse(E, sbs, eye, *m), F.fuse_loop(E, sbs, eye, *m)), (W, H, We, Hs)


@pytest.mark.parametrize("m", MAPS)
def test_a_constant_eye_takes_the_stored_eye(m):
    """E constant: every mean and every blend of means is that constant, so out = P exactly"""
    _, sbs = _case(3, 40, 22, 11, 7)
    for level in (0, 77, 255):
        E = np.full((22, 40, 3), level, np.uint8)
        assert np.array_equal(F.fuse(E, sbs, 1, *m), X.eye_plane(sbs, 1, 40, 22, *m))


def test_a_stored_eye_equal_to_the_means_returns_the_eye():
    """the identity map of 4 x 2 targets per sample: the stored eye M(E) gives P = LP, so out = E"""
    W, H, We, Hs = 64, 24, 16, 12
    ax, bx = X.identity_map(We, W)
    ay, by = X.identity_map(Hs, H)
    E, sbs = _case(4, W, H, We, Hs)
    M, rng = F.means(E, ax, bx, ay, by, We, Hs)
    assert rng == (0, We - 1, 0, Hs - 1) and M.shape == (Hs, We, 3)
    assert np.array_equal(M, ((E.reshape(Hs, 2, We, 4, 3).astype(np.int64).sum(axis=(1, 3)) * 2 + 8) // 16).astype(np.uint8))
    for eye in (0, 1):
        sbs[:, eye * We:(eye + 1) * We] = M
        assert np.array_equal(F.fuse(E, sbs, eye, ax, bx, ay, by), E)


@pytest.mark.parametrize("m", MAPS)
def test_both_clamps_saturate(m):
    for e, s in ((255, 0), (0, 255)):
        E, sbs = np.full((9, 14, 3), e, np.uint8), np.full((5, 12, 3), s, np.uint8)
        assert (F.fuse(E, sbs, 0, *m) == s).all()
    # 2 * 255 - 0 and 0 - 255 are reached: a bright eye over a dark low band of its own and a bright stored eye, and the reverse
    E = np.zeros((8, 16, 3), np.uint8)
    E[:, ::4] = 255
    ax, bx = X.identity_map(4, 16)
    ay, by = X.identity_map(4, 8)
    # (the means are 64 and 191 everywhere)
    keep = np.ones(16, bool)
    keep[::4] = False
    out = F.fuse(E, np.full((4, 8, 3), 255, np.uint8), 1, ax, bx, ay, by)
    assert (out[:, ::4] == 255).all() and (out[:, keep] == 191).all()              # 255 - 64 + 255 clamped; 0 - 64 + 255
    out = F.fuse(255 - E, np.zeros((4, 8, 3), np.uint8), 1, ax, bx, ay, by)
    assert (out[:, ::4] == 0).all() and (out[:, keep] == 64).all()                 # 0 - 191 + 0 clamped; 255 - 191 + 0


@pytest.mark.parametrize("m", MAPS)
def test_every_sample_of_the_populated_range_owns_a_target(m):
    """a 768 x 128 eye over a 170 x 50 stored eye: N > 0 throughout, and the counts are those of the nearest-sample rule"""
    for (a, b, Nd, Ns) in ((m[0], m[1], 768, 170), (m[2], m[3], 128, 50)):
        lo, counts = F.footprint_counts(a, b, Nd, Ns)
        n = F.near(a, b, Nd, Ns)
        assert (counts > 0).all() and counts.sum() == Nd and lo == n[0] and lo + len(counts) - 1 == n[-1]
        assert (np.diff(n) >= 0).all() and (np.diff(n) <= 1).all()
    E, sbs = _case(5, 768, 128, 170, 50)
    M, rng = F.means(E, *m, 170, 50)
    assert M.shape == (rng[3] - rng[2] + 1, rng[1] - rng[0] + 1, 3)


def test_a_finer_stored_eye_is_refused():
    E, sbs = _case(6, 8, 8, 16, 16)
    for m in ((65537, 0, 65536, 0), (65536, 0, 131072, 0), (4095, 0, 65536, 0)):
        with pytest.raises(ValueError):
            F.fuse(E, sbs, 1, *m)
    with pytest.raises(ValueError):
        F.fuse(E, sbs, 2, 65536, 0, 65536, 0)
    with pytest.raises(ValueError):
        F.fuse(E.astype(np.int16), sbs, 1, 65536, 0, 65536, 0)


def test_one_pixel():
    for m in MAPS:
        E, sbs = _case(7, 1, 1, 3, 2)
        want = np.clip(E.astype(int) - E + X.eye_plane(sbs, 1, 1, 1, *m), 0, 255).astype(np.uint8)      # its own mean: out = P
        assert np.array_equal(F.fuse(E, sbs, 1, *m), want) and np.array_equal(F.fuse_loop(E, sbs, 1, *m), want)
    E, sbs = _case(8, 1, 1, 1, 1)
    assert np.array_equal(F.fuse(E, sbs, 0, 65536, 0, 65536, 0)[0, 0], sbs[0, 0]) and np.array_equal(F.fuse(E, sbs, 1, 65536, 0, 65536, 0)[0, 0], sbs[0, 1])
    assert F.fuse_batch(E[None], sbs[None], 1, 65536, 0, 65536, 0).shape == (1, 1, 1, 3)
