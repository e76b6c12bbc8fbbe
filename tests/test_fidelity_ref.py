"""tests/fidelity_ref.py against itself and against hand-computed records: the vectorised int64 form against the literal loop, the
identity, constant planes, an inverted plane, the window counts at the edges of a window's fit, and every window's fixed-point Q
against an independent float64 SSIM of the same windows."""
import numpy as np
import pytest

import fidelity_ref as F
import stereo_source_ref as X

IDENT = (65536, 0, 65536, 0)


def _sbs(right, left=None):
    """an SBS frame whose right eye is `right` u8 [H,W,3]"""
    return np.concatenate([right if left is None else left, right], axis=1)


def _texture(H, W, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    base = 128 + 60 * np.sin(xx / 3.0) + 50 * np.cos(yy / 2.0)
    return np.clip(base[..., None] + rng.integers(-25, 26, (H, W, 3)), 0, 255).astype(np.uint8)


def test_identity_scores_one_in_every_window():
    P = _texture(21, 34)
    rec = F.fidelity(P, _sbs(P), 1, *IDENT, 0)
    nwx, nwy = F.windows(34, 21)
    assert (nwx, nwy) == (7, 4)
    assert rec.tolist() == [34 * 21, 0, 0, 0, 28, 28 * F.ONE]


@pytest.mark.parametrize("k", [1, 7, 200])
def test_constant_planes_differing_by_k(k):
    """cells 2 x 2 over 20 x 18 targets: 10 x 9 cells, 1 x 1 window; every mean differs by k in each channel"""
    m = (32768, 0, 32768, 0)
    E, P = np.full((18, 20, 3), 20 + k, np.uint8), np.full((9, 10, 3), 20, np.uint8)
    rec = F.fidelity(E, _sbs(P), 1, *m, 3 * k - 1)
    ya, yb = 20 + k, 20                                       # the luma weights add up to 2^15
    s1, s2 = 64 * ya, 64 * yb
    A, B = 2 * s1 * s2 + F.C1, s1 * s1 + s2 * s2 + F.C1       # vars = covar = 0: C = D = C2, q2 = 2^20
    assert rec.tolist() == [90, 90 * 3 * k, 90 * 3 * k * k, 90, 1, (A << 20) // B]
    assert F.fidelity(E, _sbs(P), 1, *m, 3 * k)[3] == 0       # the threshold is strict


def test_inverted_texture_scores_negative():
    P = _texture(16, 24, 1)
    rec = F.fidelity(255 - P, _sbs(P), 1, *IDENT, 765)
    assert rec[4] == 15 and rec[5] < 0 and rec[3] == 0


@pytest.mark.parametrize("nc,want", [(7, 0), (8, 1), (11, 1), (12, 2)])
def test_window_columns_and_rows(nc, want):
    P = _texture(9, nc, nc)
    assert F.fidelity(P, _sbs(P), 1, *IDENT, 0)[4] == want * 1
    assert F.fidelity(np.ascontiguousarray(P.transpose(1, 0, 2)), _sbs(np.ascontiguousarray(P.transpose(1, 0, 2))), 1, *IDENT, 0)[4] == want
    assert F.windows(nc, 7) == (0, 0) and F.windows(nc, 12) == ((want, 2) if want else (0, 0))


@pytest.mark.parametrize("m", [(16384, -24576, 32768, -16384), IDENT, (21846, 0, 13108, 0), (4096, -5000, 4096, 77), (200000, -3 << 16, 150000, 5 << 16)])
def test_vectorised_form_equals_the_loop(m):
    rng = np.random.default_rng(5)
    cx, cy = F.V.cell(m[0], m[2])
    W, H = 9 * cx + 3, 10 * cy + 1
    sbs = rng.integers(0, 256, (7, 16, 3), dtype=np.uint8)
    for eye in (0, 1):
        E = F.V.disturbed(X.eye_plane(sbs, eye, W, H, *m)[None], 3)[0]
        a, b = F.fidelity(E, sbs, eye, *m, 48), F.fidelity_loop(E, sbs, eye, *m, 48)
        assert a.tolist() == b.tolist() and a[4] > 0 and 0 < a[3] < a[0]


def test_every_window_within_three_steps_of_float64():
    """two floors and one shift, each below 2^-20: |Q / 2^20 - ssim| < 3 * 2^-20; A <= B and |C| <= D hold"""
    rng = np.random.default_rng(2)
    planes = [(_texture(40, 60, 3), _texture(40, 60, 4)), (_texture(40, 60, 3), 255 - _texture(40, 60, 3)),
              (rng.integers(0, 256, (40, 60, 3), dtype=np.uint8), rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)),
              (np.zeros((40, 60, 3), np.uint8), np.full((40, 60, 3), 255, np.uint8)),
              (_texture(40, 60, 5), np.clip(_texture(40, 60, 5).astype(int) + rng.integers(-6, 7, (40, 60, 3)), 0, 255).astype(np.uint8))]
    for E, P in planes:
        sums = F.window_sums(F.luma(F.cell_means(E, 1, 1)), F.luma(F.cell_means(P, 1, 1)))
        A, B, C, D = F.abcd(*sums)
        assert (A > 0).all() and (A <= B).all() and (np.abs(C) <= D).all() and (B < 1 << 31).all() and (D < 1 << 31).all()
        q = F.window_q(*sums)
        assert q.shape == (9, 14) and (np.abs(q) <= F.ONE).all()
        assert np.abs(q / F.ONE - F.window_ssim_f64(*sums)).max() < 3 / F.ONE


def test_bad_arguments():
    P = _texture(8, 8)
    for kw in (dict(bad_thr=-1), dict(bad_thr=766), dict(bad_thr=True), dict(eye=2)):
        a = dict(eye=1, bad_thr=48)
        a.update(kw)
        with pytest.raises(ValueError):
            F.fidelity(P, _sbs(P), a["eye"], *IDENT, a["bad_thr"])
    with pytest.raises(ValueError):
        F.fidelity(P, _sbs(P), 1, 4095, 0, 65536, 0, 48)
