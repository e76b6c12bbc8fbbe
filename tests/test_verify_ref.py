"""tests/verify_ref.py against itself: the vectorised form equals the literal per-pixel loop on the shapes the GPU tests use, and
hand-computed cells sit on the right side of the threshold."""
import numpy as np
import pytest

import stereo_source_ref as X
import verify_ref as V

MAPS = [(16384, -24576, 32768, -16384), (65536, 0, 65536, 0), (70000, 333, 131072, -99), (4096, -5000, 4096, 77),
        (17000, 1 << 18, 70000, -(1 << 17))]


def test_cells():
    assert V.cell(16384, 32768) == (4, 2) and V.cell(65536, 65536) == (1, 1) and V.cell(1 << 20, 70000) == (1, 1)
    assert V.cell(4096, 4096) == (16, 16) and V.cell(17000, 65535) == (4, 2)
    for bad in ((4095, 65536), (65536, (1 << 20) + 1)):
        with pytest.raises(ValueError):
            V.cell(*bad)


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (67, 9), (530, 34)])
def test_vectorised_form_equals_the_loop(W, H):
    rng = np.random.default_rng(W * H)
    sbs = rng.integers(0, 256, (9, 2 * (W // 3 + 2), 3), dtype=np.uint8)
    for k, m in enumerate(MAPS if W < 100 else MAPS[:1] + MAPS[3:4]):
        eye = (k + H) & 1
        P = X.eye_plane(sbs, eye, W, H, *m).astype(np.int64)
        E = np.clip(P + rng.integers(-60, 61, P.shape), 0, 255).astype(np.uint8)
        for tau in (0, 48, 765):
            got, n = V.verify(E, sbs, eye, *m, tau)
            want, nw = V.verify_loop(E, sbs, eye, *m, tau)
            assert np.array_equal(got, want) and n == nw, (m, tau)
            if tau == 765:
                assert n == 0 and np.array_equal(got, E)
        assert V.verify(E, sbs, eye, *m, 0)[1] > 0              # the noise is seen

def _flat(value, Ws=8, Hs=4):
    return np.full((Hs, Ws, 3), value, np.uint8)


def test_threshold_edge():
    """cells of 4 x 2 over a flat stored eye of 100: P = 100 everywhere.  A cell whose sums differ by exactly tau * npix is kept,
    by one more replaced; a cell's own pixels alone decide, and a partial cell at the edge counts its own npix"""
    m, tau = (16384, 0, 32768, 0), 48
    sbs = _flat(100)
    E = np.full((4, 10, 3), 100, np.uint8)                     # cells: columns 0-3, 4-7, 8-9 (partial), rows 0-1, 2-3
    E[0, 0] = (100 + 255 - 100, 100 - 100, 100 + 129)          # cell (0, 0): |155| + |-100| + |129| = 384 = 48 * 8: kept
    E[0, 4] = (255, 0, 230)                                    # cell (1, 0): 155 + 100 + 130 = 385: replaced
    E[2, 8], E[3, 9] = (196, 100, 100), (100, 4, 100)          # cell (2, 1), npix 4: 96 + 96 = 192 = 48 * 4: kept
    E[2, 0], E[2, 1] = (200, 100, 100), (0, 100, 100)          # cell (0, 1): channel sums cancel (+100 - 100): m = 0, kept
    got, n = V.verify(E, sbs, 1, *m, tau)
    want = E.copy()
    want[0, 4] = 100
    assert n == 1 and np.array_equal(got, want)
    assert V.verify_loop(E, sbs, 1, *m, tau)[1] == 1
    E[3, 8] = (100, 100, 101)                                  # the partial cell one over: replaced, all four of its pixels
    got, n = V.verify(E, sbs, 1, *m, tau)
    want[2:4, 8:10] = 100
    assert n == 2 and np.array_equal(got, want)


def test_tau_extremes():
    rng = np.random.default_rng(5)
    sbs = rng.integers(0, 256, (6, 12, 3), dtype=np.uint8)
    m = (32768, 0, 32768, 0)
    E = rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)
    got, n = V.verify(E, sbs, 0, *m, 765)                       # 765 = 3 * 255 per pixel cannot be passed
    assert n == 0 and np.array_equal(got, E)
    black, white = np.zeros_like(E), _flat(255, 12, 6)
    assert V.verify(black, white, 0, *m, 765)[1] == 0 and V.verify(black, white, 0, *m, 764)[1] == 36
    P = X.eye_plane(sbs, 0, 12, 12, *m)
    E = P.copy()
    E[0, 0, 0] ^= 1                                            # tau 0: every cell that differs in a sum, and no other
    E[5, 5, 1] ^= 1
    E[8, 8, 0], E[8, 9, 0] = np.clip([int(P[8, 8, 0]) + 3, int(P[8, 9, 0]) - 3], 0, 255)    # differs, sums equal: kept
    if int(E[8, 8, 0]) - int(P[8, 8, 0]) + int(E[8, 9, 0]) - int(P[8, 9, 0]) == 0:
        got, n = V.verify(E, sbs, 0, *m, 0)
        want = E.copy()
        want[0, 0], want[5, 5] = P[0, 0], P[5, 5]
        assert n == 2 and np.array_equal(got, want)
    got, n = V.verify(P, sbs, 0, *m, 0)
    assert n == 0 and np.array_equal(got, P)


def test_arguments():
    sbs, E = _flat(1), np.zeros((2, 2, 3), np.uint8)
    for tau in (-1, 766, 1.5, True):
        with pytest.raises(ValueError):
            V.verify(E, sbs, 1, 65536, 0, 65536, 0, tau)
    with pytest.raises(ValueError):
        V.verify(E, sbs, 2, 65536, 0, 65536, 0, 48)
    with pytest.raises(ValueError):
        V.verify(E.astype(np.int16), sbs, 1, 65536, 0, 65536, 0, 48)
    out, counts = V.verify_batch(np.stack([E, E]), np.stack([sbs, _flat(200)]), 1, 65536, 0, 65536, 0, 48)
    assert counts.dtype == np.uint32 and counts.tolist() == [0, 4] and (out[1] == 200).all() and (out[0] == 0).all()
