"""k_split_tb of csrc/v3d_pre.hip (gray and BGR, single and batch), without a GPU: the kernel source runs in the stand-alone
emulator driver (tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/tb_ref.py
byte for byte.  The frame starts 0 .. 3 bytes into its 4-byte word and ends on its heap block's last byte: the last row has no
pitch padding behind it and the first none in front, so neither load plan may leave the payload.  Pitches dense, + 4, + 5 and, where
3 W is no multiple of 4, the next multiple of 4: an aligned base with a pitch of a multiple of 4 takes the dword plan for whole pixel
groups, everything else the byte plan.  Widths 5 and 7 are less than two pixel groups with a partial last one, 1028 is one pixel group
beyond a workgroup's 1024 columns.  Heights: eyes of 1, 2 and 3 rows have both borders inside one tap window; 118, 120 and 122 are
one row short of, exactly and one row over two bands of TB_BAND = 60 rows (at fewer placements: the bands do not depend on
the load plan)."""
import numpy as np
import pytest

import emu_case as E
import tb_ref

ENTRIES = ["v3d_tb_to_gray", "v3d_split_tb", "v3d_tb_to_gray_batch"]
driver = E.driver_fixture("pre_tb", ["v3d_pre.hip"], ENTRIES)
TB_BAND = 60
WIDTHS = [5, 7, 64, 322, 1076, 1028]
SMALL_HEIGHTS = [2, 4, 6, 18]
BAND_HEIGHTS = [2 * TB_BAND - 2, 2 * TB_BAND, 2 * TB_BAND + 2]


def every_placement(W):
    """(base offset, pitch padding)"""
    return [(o, p) for o in range(4) for p in sorted({0, 4, 5, -3 * W % 4})]


SOME_PLACEMENTS = [(0, 0), (3, 4), (2, 5)]


def _frame_bytes(frames, pitch, stride, gp):
    """[n,H,W,3] -> the bytes from the first frame's first to the last frame's last payload byte"""
    n, H, W, _ = frames.shape
    img = np.full((n - 1) * stride + (H - 1) * pitch + W * 3, gp, np.uint8)
    for f in range(n):
        for y in range(H):
            img[f * stride + y * pitch:f * stride + y * pitch + W * 3] = frames[f, y].reshape(-1)
    return img


def _out(name, want, skew, gp):
    return E.exact(name, np.full(want.size, gp, np.uint8), skew, expect=want.reshape(-1))


def _run_single(driver, tmp_path, W, H, unsqueeze, placements):
    tb = tb_ref.content(1, H, W, W * 3 + H)
    want = {True: tb_ref.to_gray(tb[0], bool(unsqueeze)), False: tb_ref.split(tb[0], bool(unsqueeze))}
    for i, (off, pad) in enumerate(placements):
        gray = (i + H // 2) % 2 == 0                                # both entries meet every offset and both load plans
        wl, wr = want[gray]
        pitch = W * 3 + pad

        def make(gp):
            return [E.exact("tb", _frame_bytes(tb, pitch, 0, gp), off), W, H, pitch, unsqueeze, _out("left", wl, 1, gp), _out("right", wr, 3, gp), 0]
        E.run_configs(driver, tmp_path, ENTRIES[0] if gray else ENTRIES[1], make)


@pytest.mark.parametrize("unsqueeze", [1, 0])
@pytest.mark.parametrize("H", SMALL_HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_split_at_every_base_offset_and_pitch(driver, tmp_path, W, H, unsqueeze):
    _run_single(driver, tmp_path, W, H, unsqueeze, every_placement(W))


@pytest.mark.parametrize("unsqueeze", [1, 0])
@pytest.mark.parametrize("H", BAND_HEIGHTS)
@pytest.mark.parametrize("W", [7, 322, 1028])
def test_split_around_the_band_height(driver, tmp_path, W, H, unsqueeze):
    _run_single(driver, tmp_path, W, H, unsqueeze, SOME_PLACEMENTS)


@pytest.mark.parametrize("unsqueeze", [1, 0])
@pytest.mark.parametrize("W,H,off,pad,spad", [(66, 18, 0, 0, 0), (1076, 6, 3, 4, 8), (7, 122, 2, 5, 7), (1028, 4, 0, 4, 12)])
def test_gray_batch(driver, tmp_path, W, H, off, pad, spad, unsqueeze):
    n = 3
    tb = tb_ref.content(n, H, W, W + 1)
    wl, wr = tb_ref.to_gray_batch(tb, bool(unsqueeze))
    pitch = W * 3 + pad
    stride = H * pitch + spad

    def make(gp):
        return [E.exact("tb", _frame_bytes(tb, pitch, stride, gp), off), n, W, H, pitch, stride, unsqueeze, _out("left", wl, 2, gp), _out("right", wr, 5, gp), 0]
    E.run_configs(driver, tmp_path, ENTRIES[2], make)


@pytest.mark.parametrize("args", [
    dict(H=7), dict(H=0), dict(W=0), dict(pitch=3 * 8 - 1), dict(n=0), dict(n=2, stride=6 * 24 - 1)])
def test_refused_calls_write_nothing(driver, tmp_path, args):
    a = dict(n=1, W=8, H=6, pitch=24, stride=0)
    a.update(args)
    tb = tb_ref.content(2, 6, 8, 1)

    def make(gp):
        out = lambda name: E.exact(name, np.full(2 * 8 * 8, gp, np.uint8), 1)       # expected unchanged
        return [E.exact("tb", _frame_bytes(tb, 24, 6 * 24, gp), 0), a["n"], a["W"], a["H"], a["pitch"], a["stride"], 1, out("left"), out("right"), 0]
    E.run_configs(driver, tmp_path, ENTRIES[2], make, rc=-1)
