"""v3d_verify_eye_source_batch of csrc/v3d_verify.hip, without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/verify_ref.py byte for
byte.  The eye image is the right half of a full-SBS buffer, the lower half of a full top-bottom one or a buffer of its own, and
that buffer starts on its first payload byte and ends on its last; so do the SBS frames, with pitched rows and padded frames whose
slack is poisoned and must stay as it is.  The counters hold garbage before the call."""
import numpy as np
import pytest

import emu_case as E
import launch_plan as LP
import verify_ref as V

ENTRY = "v3d_verify_eye_source_batch"
driver = E.driver_fixture("verify", ["v3d_verify.hip"], [ENTRY])
MAPS = [(16384, -24576, 32768, -16384), (65536, 0, 65536, 0), (4096, -5000, 4096, 77), (17000, 1 << 18, 70000, -(1 << 17)),
        (200000, -3 << 16, 150000, 5 << 16)]


def _noisy(rng, sbs, eye, W, H, m, share=0.4, amp=40):
    """an eye image that agrees with the stored eye up to small noise, but for `share` of its pixels, which are anything"""
    import stereo_source_ref as X
    P = np.stack([X.eye_plane(s, eye, W, H, *m) for s in sbs]).astype(np.int64)
    out = np.clip(P + rng.integers(-amp, amp + 1, P.shape), 0, 255)
    wrong = rng.random(P.shape[:3]) < share
    out[wrong] = rng.integers(0, 256, (int(wrong.sum()), 3))
    return out.astype(np.uint8)


def _call(driver, tmp, eyes, sbs, eye, m, tau, layout="alone", rowpad=0, framepad=0, skew=5, rc=0):
    """eyes u8 [n,H,W,3], sbs u8 [n,Hs,Ws,3]; layout: where the eye lies in its buffer (alone | sbs | tb)"""
    n, H, W = eyes.shape[:3]
    Hs, Ws = sbs.shape[1:3]
    want, counts = (eyes, np.zeros(n, np.uint32)) if rc else V.verify_batch(eyes, sbs, eye, *m, tau)
    pitch = 3 * Ws + rowpad
    ss = Hs * pitch + framepad
    rng = np.random.default_rng(n + W)
    other = rng.integers(0, 256, eyes.shape, dtype=np.uint8)   # the left eye of the packed frame: not to be touched
    pack = {"alone": lambda e: e, "sbs": lambda e: np.concatenate([other, e], axis=2), "tb": lambda e: np.concatenate([other, e], axis=1)}[layout]
    off, epitch = {"alone": (0, 3 * W), "sbs": (3 * W, 6 * W), "tb": (3 * W * H, 3 * W)}[layout]
    full = pack(eyes)
    stride = full[0].size

    def make(gp):
        sb = np.full((n - 1) * ss + (Hs - 1) * pitch + 3 * Ws, gp, np.uint8)     # ends on the last payload byte
        for i in range(n):
            for j in range(Hs):
                sb[i * ss + j * pitch:i * ss + j * pitch + 3 * Ws] = sbs[i, j].reshape(-1)
        ebuf = E.exact("eye", full.reshape(-1), skew, expect=pack(want).reshape(-1))
        cnt = E.exact("replaced", np.full(4 * n, 0xEE, np.uint8), 4,
                      expect=np.full(4 * n, 0xEE, np.uint8) if rc else counts.astype("<u4").view(np.uint8))
        return [(ebuf, off), stride, epitch, n, W, H, E.exact("sbs", sb, 3), ss, Ws, Hs, pitch, eye, *m, tau, cnt, 0]
    E.run_configs(driver, tmp, ENTRY, make, rc=rc)
    return counts


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (67, 9), (530, 34)])
def test_sizes_cells_and_eyes(driver, tmp_path, W, H):
    rng = np.random.default_rng(W)
    sbs = rng.integers(0, 256, (1, 7, 12, 3), dtype=np.uint8) if W < 100 else rng.integers(0, 256, (1, 19, 270, 3), dtype=np.uint8)
    for k, m in enumerate(MAPS):
        eye = (k + W) & 1
        counts = _call(driver, tmp_path, _noisy(rng, sbs, eye, W, H, m), sbs, eye, m, (0, 48, 765)[k % 3],
                       layout=("alone", "sbs", "tb")[k % 3], skew=(1, 15, 5)[k % 3])
        if W > 60 and k % 3 == 1:
            cx, cy = V.cell(m[0], m[2])
            assert 0 < counts[0] < -(-W // cx) * -(-H // cy)   # the case decides both ways


def test_wide_rows(driver, tmp_path):
    rng = np.random.default_rng(3840)
    sbs = rng.integers(0, 256, (1, 3, 1920, 3), dtype=np.uint8)
    _call(driver, tmp_path, _noisy(rng, sbs, 1, 3840, 4, MAPS[0]), sbs, 1, MAPS[0], 48, layout="sbs")
    sbs = rng.integers(0, 256, (1, 2, 2 * 8192, 3), dtype=np.uint8)
    _call(driver, tmp_path, _noisy(rng, sbs, 1, 8192, 1, MAPS[1]), sbs, 1, MAPS[1], 48, skew=15)


def test_item_stride(driver, tmp_path):
    """the grid's stride over the items (tests/launch_plan.py; tests/test_launch_plan_host.py holds the regimes): 1025 items for
    1024 wave slots, and 1026 items three waves across under a one-row SBS frame, where a wave's second item lies in another
    column of waves and blends the same SBS rows as its first"""
    rng = np.random.default_rng(8200)
    _, W, H = LP.EMU_STRIDE
    sbs = rng.integers(0, 256, (1, H // 2, 12, 3), dtype=np.uint8)           # the lower half clamps to the last row
    counts = _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, LP.EMU_MAP), sbs, 1, LP.EMU_MAP, 48, skew=1)
    assert 0 < counts[0] < W * H
    _, W, H = LP.EMU_TAPS
    sbs = rng.integers(0, 256, (1, 1, 2 * W, 3), dtype=np.uint8)
    counts = _call(driver, tmp_path, _noisy(rng, sbs, 0, W, H, LP.EMU_MAP), sbs, 0, LP.EMU_MAP, 48, layout="sbs")
    assert 0 < counts[0] < W * H


def test_the_floor_of_eight_workgroups_a_frame(driver, tmp_path):
    """260 frames of 33 items: 9 workgroups wanted, 8 launched, workgroup 0's first wave walks on; 5 distinct frames repeated"""
    rng = np.random.default_rng(260)
    n, W, H = LP.EMU_FLOOR_VERIFY
    sbs = rng.integers(0, 256, (5, H, 2 * W, 3), dtype=np.uint8)
    idx = np.arange(n) % 5
    counts = _call(driver, tmp_path, _noisy(rng, sbs, 1, W, H, LP.EMU_MAP)[idx], sbs[idx], 1, LP.EMU_MAP, 48, rowpad=1, framepad=3)
    assert len(set(counts[:5].tolist())) > 1 and np.array_equal(counts, counts[:5][idx])


def test_three_frames_pitched_rows_and_padded_frames(driver, tmp_path):
    rng = np.random.default_rng(7)
    sbs = rng.integers(0, 256, (3, 6, 40, 3), dtype=np.uint8)
    for layout in ("sbs", "tb"):
        _call(driver, tmp_path, _noisy(rng, sbs, 1, 77, 11, MAPS[0]), sbs, 1, MAPS[0], 48, layout=layout, rowpad=5, framepad=9)


def test_rows_beyond_2_to_the_31_in_q16(driver, tmp_path):
    """(Hs - 1) << 16 passes 2^31: the bottom clamp and a blend of the last rows, the SBS buffer ending on its last payload byte"""
    rng = np.random.default_rng(9)
    sbs = rng.integers(0, 256, (1, 32769, 2, 3), dtype=np.uint8)
    for m in ((65536, 0, 65536, 1 << 40), (65536, 0, 1 << 20, ((32769 - 34) << 16) + 32768)):
        _call(driver, tmp_path, _noisy(rng, sbs, 1, 7, 3, m), sbs, 1, m, 20)


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
    wide = np.zeros((2, 1, 2 * 8193, 3), np.uint8)              # an eye wider than 8192 is unsupported, unless an argument is bad too
    _call(driver, tmp_path, eyes, wide, 1, MAPS[0], 48, rc=-3)
    _call(driver, tmp_path, eyes, wide, 1, MAPS[0], 766, rc=-1)
