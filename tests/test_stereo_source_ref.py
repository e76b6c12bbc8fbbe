"""tests/stereo_source_ref.py against its literal loop twin, against tests/stereo_pack_ref.py where no eye is filled, and against
answers worked out by hand.  No GPU."""
import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_ref as R
import stereo_source_ref as X
import stereo_sub_ref as S


def _scene(W, H, Ws, Hs, seed, kind="planar"):
    rng = np.random.default_rng(seed)
    F = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sbs = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    return F, S.scene_depth(kind, H, W, seed), sbs


MAPS = [(65536, 0, 65536, 0), (21845, -9000, 30000, 77), (200000, -3 << 16, 150000, 5 << 16), (4096, 1 << 30, 1 << 20, -(1 << 30))]


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("packing", P.PACKINGS)
def test_vectorised_equals_loop(packing, sub):
    W, H = 22, 4
    F, D, sbs = _scene(W, H, 12, 5, 7 + packing, ("planar", "noise")[packing % 2])
    gains = [R.stereo_gains(6, 0.5, 0.5), R.stereo_gains(9, 0.3, 0.0), (3000, -1500, 20000)][packing % 3]
    holes = 0
    for fill in range(4):
        m = MAPS[(fill + packing) % len(MAPS)]
        got = X.render(F, D, *gains, packing, sub, sbs, fill, *m)
        assert np.array_equal(got, X.render_loop(F, D, *gains, packing, sub, sbs, fill, *m)), (packing, sub, fill)
        holes += sum(int((~X.hit_mask(D, g, gains[2], sub)).sum()) for g in gains[:2])
    assert holes > 0                                           # the scenes do have holes to fill


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("packing", P.PACKINGS)
def test_no_eye_filled_is_the_packed_render(packing, sub):
    F, D, sbs = _scene(40, 6, 10, 3, 3)
    gains = R.stereo_gains(12, 0.4, 0.5)
    want = P.render(F, D, *gains, packing, sub)
    assert np.array_equal(X.render(F, D, *gains, packing, sub, sbs, 0, *MAPS[1]), want)
    assert np.array_equal(X.render(F, D, *gains, packing, sub, None, 0), want)


def test_hit_mask_is_the_renderers_z_buffer():
    """a filled eye differs from the background render in hole targets only, and a black background (no key at all) is all holes"""
    F, D, sbs = _scene(64, 3, 8, 2, 11, "noise")
    gl, gr, conv = R.stereo_gains(20, 0.5, 0.5)
    for sub in (False, True):
        bg = P.eyes(F, D, gl, gr, conv, sub)
        fl = X.eyes(F, D, gl, gr, conv, sub, sbs, 3, *MAPS[0])
        for e, g in enumerate((gl, gr)):
            hit = X.hit_mask(D, g, conv, sub)
            assert np.array_equal(bg[e][hit], fl[e][hit])
    far = X.hit_mask(np.full((1, 8), 65535, np.uint16), 8 * 256 * 256, 0, False)        # every source leaves the row
    assert not far.any()


def test_hand_computed_row():
    """W = 6, one row, integer render, right eye only.  Depth (0, 0, 65535, 65535, 0, 0), gain_right = -512 (2 px at full depth),
    conv = 0: sources 2 and 3 land on targets 0 and 1 and win there, sources 4 and 5 stay, targets 2 and 3 are holes.
    Eye plane: SBS 2 x 4 (We = 2), right eye columns 2, 3; map u = 16384 t (a quarter pixel per target), v = 32768 (fy = 128)."""
    F = np.arange(18, dtype=np.uint8).reshape(1, 6, 3) + 100
    D = np.array([[0, 0, 65535, 65535, 0, 0]], np.uint16)
    sbs = np.zeros((2, 4, 3), np.uint8)
    sbs[0, 2], sbs[0, 3], sbs[1, 2], sbs[1, 3] = (10, 20, 30), (50, 60, 70), (110, 120, 130), (150, 160, 170)
    full = X.render(F, D, 0, -512, 0, P.FULL_SBS, False, sbs, 2, 16384, 0, 65536, 32768)
    EL, ER = full[:, :6], full[:, 6:]
    assert np.array_equal(EL, F)
    assert np.array_equal(ER[0, [0, 1, 4, 5]], F[0, [2, 3, 4, 5]])
    # t = 2: u = 32768 -> i0 = 0, fx = 128; top = 128 * 10 + 128 * 50 = 7680, bottom = 128 * 110 + 128 * 150 = 33280;
    # P = (128 * 7680 + 128 * 33280 + 32768) >> 16 = 5275648 >> 16 = 80; the other channels are 10 and 20 higher
    assert ER[0, 2].tolist() == [80, 90, 100]
    # t = 3: u = 49152 -> fx = 192; top = 64 * 10 + 192 * 50 = 10240, bottom = 64 * 110 + 192 * 150 = 35840; P = (128 * 46080 + 32768) >> 16 = 90
    assert ER[0, 3].tolist() == [90, 100, 110]
    # the background render paints both holes with the farther neighbour instead (source 4 on the right, depth 0 < 65535)
    assert np.array_equal(P.render(F, D, 0, -512, 0, P.FULL_SBS)[0, 6 + 2], F[0, 4])


def test_identity_at_equal_size_is_a_copy():
    rng = np.random.default_rng(5)
    sbs = rng.integers(0, 256, (7, 18, 3), dtype=np.uint8)
    for e in (0, 1):
        assert np.array_equal(X.eye_plane(sbs, e, 9, 7, 65536, 0, 65536, 0), sbs[:, e * 9:(e + 1) * 9])
    assert X.identity_map(9, 9) == (65536, 0) and X.identity_map(240, 480) == (32768, -16384)


def test_clamping_on_all_four_sides():
    """coordinates beyond an edge repeat the eye's edge sample, and a tap never crosses into the other eye's half"""
    rng = np.random.default_rng(6)
    sbs = rng.integers(0, 256, (4, 10, 3), dtype=np.uint8)
    We, Hs = 5, 4
    for e in (0, 1):
        eye = sbs[:, e * We:(e + 1) * We]
        left = X.eye_plane(sbs, e, 3, Hs, 65536, -(7 << 16), 65536, 0)
        assert np.array_equal(left, np.repeat(eye[:, :1], 3, axis=1))
        right = X.eye_plane(sbs, e, 3, Hs, 65536, (We - 1 << 16) + 40000, 65536, 0)       # i0 = We - 1: i1 must not be column We
        assert np.array_equal(right, np.repeat(eye[:, -1:], 3, axis=1))
        top = X.eye_plane(sbs, e, We, 2, 65536, 0, 65536, -(1 << 40))
        assert np.array_equal(top, np.repeat(eye[:1], 2, axis=0))
        bottom = X.eye_plane(sbs, e, We, 2, 65536, 0, 1 << 20, 1 << 40)
        assert np.array_equal(bottom, np.repeat(eye[-1:], 2, axis=0))
    # the last column of the left eye with fx > 0 would blend in the right eye's first column if i1 were not clamped
    edge = X.eye_plane(sbs, 0, 1, Hs, 65536, (We - 1 << 16) + 32768, 65536, 0)
    assert np.array_equal(edge[:, 0], sbs[:, We - 1])


def test_rows_beyond_2_to_the_31_in_q16():
    """Hs has no bound: (Hs - 1) << 16 passes 2^31 from Hs = 32769 on, and the row coordinate must not be narrowed to 32 bits.
    Rows are marked by their index; by = 2^40 clamps to the last row, and a map that lands between the last two rows blends them"""
    for Hs in (32768, 32769, 40000):
        sbs = np.zeros((Hs, 2, 3), np.uint8)
        sbs[:, :, 0], sbs[:, :, 1] = (np.arange(Hs) & 255)[:, None], (np.arange(Hs) >> 8)[:, None]
        last = X.eye_plane(sbs, 1, 3, 2, 65536, 0, 65536, 1 << 40)
        assert np.array_equal(last, np.broadcast_to(sbs[Hs - 1, 1], (2, 3, 3)))
        P2 = X.eye_plane(sbs, 1, 1, 2, 65536, 0, 65536, ((Hs - 3) << 16) + 32768)        # rows Hs - 3 .. Hs - 1, fy = 128
        lo = [int(sbs[Hs - 3 + k, 1, 0]) for k in range(3)]
        assert [int(P2[k, 0, 0]) for k in range(2)] == [(128 * 256 * (lo[k] + lo[k + 1]) + 32768) >> 16 for k in range(2)]
        F = np.full((2, 3, 3), 9, np.uint8)
        D = np.full((2, 3), 65535, np.uint16)
        m = (65536, 0, 65536, 1 << 40)
        got = X.render(F, D, 0, -(3 << 8), 0, P.FULL_SBS, False, sbs, 2, *m)              # the right eye is all holes
        assert np.array_equal(got, X.render_loop(F, D, 0, -(3 << 8), 0, P.FULL_SBS, False, sbs, 2, *m))
        assert np.array_equal(got[:, 3:], last)


def test_refusals_of_the_reference():
    F, D, sbs = _scene(8, 2, 6, 2, 1)
    with pytest.raises(ValueError):
        X.render(F, D, 0, -256, 0, P.FULL_SBS, False, sbs, 4)
    with pytest.raises(ValueError):
        X.eye_plane(sbs[:, :5], 0, 4, 2, 65536, 0, 65536, 0)
