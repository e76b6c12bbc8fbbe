"""v3d_eye_fidelity_batch of csrc/v3d_fidelity.hip, without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/fidelity_ref.py bit for
bit.  The eye image is the right half of a full-SBS buffer, the lower half of a full top-bottom one or a buffer of its own, and
that buffer starts on its first payload byte and ends on its last; so do the SBS frames, with pitched rows and padded frames whose
slack is poisoned, and the workspace, which is exactly v3d_eye_fidelity_ws_bytes long.  Both images must stay as they are; the
records and the workspace hold garbage before the call."""
import numpy as np
import pytest

import emu_case as E
import fidelity_ref as F
import launch_plan as LP
import stereo_source_ref as X

ENTRY, WS = "v3d_eye_fidelity_batch", "v3d_eye_fidelity_ws_bytes"
driver = E.driver_fixture("fidelity", ["v3d_fidelity.hip"], [ENTRY, WS])
MAPS = [(16384, -24576, 32768, -16384), (65536, 0, 65536, 0), (4096, -5000, 4096, 77), (17000, 1 << 18, 70000, -(1 << 17)),
        (200000, -3 << 16, 150000, 5 << 16), (5958, 0, 13108, 0)]


def _noisy(rng, sbs, eye, W, H, m):
    return F.V.disturbed(np.stack([X.eye_plane(s, eye, W, H, *m) for s in sbs]), int(rng.integers(1 << 30)))


def _call(driver, tmp, eyes, sbs, eye, m, thr, layout="alone", rowpad=0, framepad=0, skew=5, rc=0, ws_skew=16, out_skew=8):
    """eyes u8 [n,H,W,3], sbs u8 [n,Hs,Ws,3]; layout: where the eye lies in its buffer (alone | sbs | tb) -> the records"""
    n, H, W = eyes.shape[:3]
    Hs, Ws = sbs.shape[1:3]
    want = None if rc else F.fidelity_batch(eyes, sbs, eye, *m, thr)
    pitch = 3 * Ws + rowpad
    ss = Hs * pitch + framepad
    other = np.random.default_rng(n + W).integers(0, 256, eyes.shape, dtype=np.uint8)
    pack = {"alone": lambda e: e, "sbs": lambda e: np.concatenate([other, e], axis=2), "tb": lambda e: np.concatenate([other, e], axis=1)}[layout]
    off, epitch = {"alone": (0, 3 * W), "sbs": (3 * W, 6 * W), "tb": (3 * W * H, 3 * W)}[layout]
    full = pack(eyes)
    need = E.query(driver, WS, n, W, H, m[0], m[2])

    def make(gp):
        sb = np.full((n - 1) * ss + (Hs - 1) * pitch + 3 * Ws, gp, np.uint8)     # ends on the last payload byte
        for i in range(n):
            for j in range(Hs):
                sb[i * ss + j * pitch:i * ss + j * pitch + 3 * Ws] = sbs[i, j].reshape(-1)
        out = np.full(8 * F.FIELDS * n, gp, np.uint8)
        return [(E.exact("eye", full.reshape(-1), skew), off), full[0].size, epitch, n, W, H, E.exact("sbs", sb, 3), ss, Ws, Hs, pitch, eye,
                *m, thr, E.exact("out", out, out_skew, expect=out.copy() if rc else want.astype("<i8").view(np.uint8).reshape(-1)),
                E.exact("ws", np.full(max(need, 64), gp, np.uint8), ws_skew, expect=np.full(max(need, 64), gp, np.uint8) if rc else None), 0]
    E.run_configs(driver, tmp, ENTRY, make, rc=rc)
    return want


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (67, 41), (200, 120)])
def test_sizes_cells_and_eyes(driver, tmp_path, W, H):
    rng = np.random.default_rng(W)
    sbs = rng.integers(0, 256, (1, 7, 12, 3), dtype=np.uint8) if W < 100 else rng.integers(0, 256, (1, 61, 202, 3), dtype=np.uint8)
    for k, m in enumerate(MAPS):
        eye = (k + W) & 1
        rec = _call(driver, tmp_path, _noisy(rng, sbs, eye, W, H, m), sbs, eye, m, (0, 48, 765)[k % 3],
                    layout=("alone", "sbs", "tb")[k % 3], skew=(1, 15, 5)[k % 3])
        if W == 200 and k == 1:
            assert rec[0, 4] > 33 * 9 and rec[0, 1] > 0         # more windows than one stage-2 tile holds


def test_window_fits(driver, tmp_path):
    """ncx and ncy at 7, 8, 11 and 12 under 1 x 1 and 2 x 2 cells"""
    rng = np.random.default_rng(8)
    for m, c in ((MAPS[1], 1), ((32768, 0, 32768, 0), 2)):
        for nc, nw in ((7, 0), (8, 1), (11, 1), (12, 2)):
            W, H = nc * c - (c - 1), 12 * c
            sbs = rng.integers(0, 256, (1, 12, 2 * 12, 3), dtype=np.uint8)
            assert _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, m), sbs, 1, m, 30)[0, 4] == 2 * nw
            assert _call(driver, tmp_path, _noisy(rng, sbs, 1, H, W, m), sbs, 1, m, 30)[0, 4] == 2 * nw


def test_content(driver, tmp_path):
    rng = np.random.default_rng(4)
    m = (32768, 0, 32768, 0)
    sbs = rng.integers(0, 256, (1, 20, 60, 3), dtype=np.uint8)
    P = X.eye_plane(sbs[0], 1, 60, 40, *m)[None]
    assert _call(driver, tmp_path, P, sbs, 1, m, 0)[0].tolist() == [600, 0, 0, 0, 6 * 4, 24 << 20]
    assert _call(driver, tmp_path, 255 - P, sbs, 1, m, 100)[0, 5] < 0
    white = np.full((1, 20, 60, 3), 255, np.uint8)
    rec = _call(driver, tmp_path, np.zeros((1, 40, 60, 3), np.uint8), white, 1, m, 764)
    assert rec[0].tolist()[:5] == [600, 600 * 765, 600 * 3 * 255 * 255, 600, 24]
    _call(driver, tmp_path, np.full((1, 40, 60, 3), 77, np.uint8), np.full((1, 20, 60, 3), 70, np.uint8), 0, m, 20)


def test_wide_rows(driver, tmp_path):
    rng = np.random.default_rng(3840)
    sbs = rng.integers(0, 256, (1, 5, 1920, 3), dtype=np.uint8)
    _call(driver, tmp_path, _noisy(rng, sbs, 1, 3840, 9, MAPS[0]), sbs, 1, MAPS[0], 48, layout="sbs")
    sbs = rng.integers(0, 256, (1, 2, 2 * 8192, 3), dtype=np.uint8)
    _call(driver, tmp_path, _noisy(rng, sbs, 1, 8192, 1, MAPS[1]), sbs, 1, MAPS[1], 48, skew=15)


def test_item_and_tile_stride(driver, tmp_path):
    """the grid's stride in both stages (tests/launch_plan.py; tests/test_launch_plan_host.py holds the regimes): 1025 items for 1024
    wave slots; 1026 items three waves across under a one-row SBS frame (a wave's second item in another column of waves, the
    same SBS rows); 257 tiles for 256 workgroups, with noise, the identical eye (a wrong multiple of 2^20 if a tile is dropped or
    doubled) and the inverted one (negative Q carried)"""
    rng = np.random.default_rng(8200)
    _, W, H = LP.EMU_STRIDE
    sbs = rng.integers(0, 256, (1, H // 2, 12, 3), dtype=np.uint8)           # the lower half clamps to the last row
    rec = _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, LP.EMU_MAP), sbs, 1, LP.EMU_MAP, 48, skew=1)
    assert rec[0, 0] == W * H and 0 < rec[0, 3] < W * H and rec[0, 4] == 0
    _, W, H = LP.EMU_TAPS
    sbs = rng.integers(0, 256, (1, 1, 2 * W, 3), dtype=np.uint8)
    rec = _call(driver, tmp_path, _noisy(rng, sbs, 0, W, H, LP.EMU_MAP), sbs, 0, LP.EMU_MAP, 48, layout="sbs")
    assert 0 < rec[0, 3] < W * H and rec[0, 4] > 0
    _, W, H = LP.EMU_TILES
    sbs = rng.integers(0, 256, (1, H, 2 * W, 3), dtype=np.uint8)
    n_win = LP.fidelity_plan(1, W, H, LP.EMU_MAP[0], LP.EMU_MAP[2]).nwy
    rec = _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, LP.EMU_MAP), sbs, 1, LP.EMU_MAP, 48, skew=15)
    assert rec[0, 4] == n_win and 0 < abs(rec[0, 5]) < n_win << 20
    P = X.eye_plane(sbs[0], 1, W, H, *LP.EMU_MAP)[None]
    assert _call(driver, tmp_path, P, sbs, 1, LP.EMU_MAP, 0)[0].tolist() == [W * H, 0, 0, 0, n_win, n_win << 20]
    assert _call(driver, tmp_path, 255 - P, sbs, 1, LP.EMU_MAP, 100)[0, 5] < -(n_win << 16)


def test_the_floor_of_eight_workgroups_a_frame(driver, tmp_path):
    """260 frames of 33 items and 9 tiles: 8 workgroups launched in either stage, workgroup 0 walks on; 5 distinct frames repeated"""
    rng = np.random.default_rng(260)
    n, W, H = LP.EMU_FLOOR_FIDELITY
    sbs = rng.integers(0, 256, (5, H, 2 * W, 3), dtype=np.uint8)
    idx = np.arange(n) % 5
    rec = _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, LP.EMU_MAP)[idx], sbs[idx], 1, LP.EMU_MAP, 48, rowpad=1, framepad=3)
    assert len({tuple(r) for r in rec[:5].tolist()}) == 5 and np.array_equal(rec, rec[:5][idx])


def test_three_frames_pitched_rows_and_padded_frames(driver, tmp_path):
    rng = np.random.default_rng(7)
    sbs = rng.integers(0, 256, (3, 12, 40, 3), dtype=np.uint8)
    eyes = _noisy(rng, sbs, 1, 77, 23, MAPS[0])
    for layout in ("sbs", "tb"):
        rec = _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], 48, layout=layout, rowpad=5, framepad=9)
        for i in range(3):                                      # a frame's record is the same alone
            assert np.array_equal(_call(driver, tmp_path, eyes[i:i + 1], sbs[i:i + 1], 1, MAPS[0], 48, layout=layout)[0], rec[i])


def test_rows_beyond_2_to_the_31_in_q16(driver, tmp_path):
    rng = np.random.default_rng(9)
    sbs = rng.integers(0, 256, (1, 32769, 2, 3), dtype=np.uint8)
    for m in ((65536, 0, 65536, 1 << 40), (65536, 0, 1 << 20, ((32769 - 34) << 16) + 32768)):
        _call(driver, tmp_path, _noisy(rng, sbs, 1, 9, 11, m), sbs, 1, m, 20)


def test_refusals(driver, tmp_path):
    rng = np.random.default_rng(1)
    sbs = rng.integers(0, 256, (2, 3, 8, 3), dtype=np.uint8)
    eyes = rng.integers(0, 256, (2, 4, 9, 3), dtype=np.uint8)
    for bad in ((4095, 0, 65536, 0), (65536, 0, (1 << 20) + 1, 0), (65536, (1 << 40) + 1, 65536, 0), (65536, 0, 65536, -(1 << 40) - 1)):
        _call(driver, tmp_path, eyes, sbs, 1, bad, 48, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 2, MAPS[0], 48, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], -1, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], 766, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], 48, rowpad=-1, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], 48, ws_skew=8, rc=-1)
    _call(driver, tmp_path, eyes, sbs, 1, MAPS[0], 48, out_skew=4, rc=-1)
    wide = np.zeros((2, 1, 2 * 8193, 3), np.uint8)              # an eye wider than 8192 is unsupported, unless an argument is bad too
    _call(driver, tmp_path, eyes, wide, 1, MAPS[0], 48, rc=-3)
    _call(driver, tmp_path, eyes, wide, 1, MAPS[0], 766, rc=-1)
    assert E.query(driver, WS, 0, 9, 4, 65536, 65536) == 0 and E.query(driver, WS, 1, 8193, 4, 65536, 65536) == 0
    assert E.query(driver, WS, 1, 9, 4, 4095, 65536) == 0 and E.query(driver, WS, 1, 9, 4, 65536, 65536) > 0
