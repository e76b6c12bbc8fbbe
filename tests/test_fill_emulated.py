"""csrc/v3d_fill.hip itself, without a GPU: the kernel source runs in the stand-alone emulator driver (tests/emu_case.py), plain and
under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/fill_ref.py byte for byte.  Widths on both sides of
every change of pixels per thread (W + 7 <= 2048 / 4096 / 8192), each of the eight 2-byte phases of a row inside a 16-byte block,
the hole patterns of tests/test_fill_gpu.py, one band and two bands of the empty-row pass, a source row more than 256 rows away,
in place and out of place.  k_fill_rows reads the aligned 16-byte blocks that cover a row: the input lies in exactly the blocks
that hold its payload, with the slack poisoned."""
import numpy as np
import pytest

import emu_case as E
import fill_ref as FR
from test_fill_gpu import patterns

ENTRY = "v3d_fill_holes_disp16_batch"
driver = E.driver_fixture("fill", ["v3d_fill.hip"], [ENTRY, "v3d_fill_holes_ws_bytes"])
WIDTHS = [1, 7, 2041, 2042, 4089, 4090, 8185, 8186, 8192]
ROW_PATTERNS = ("empty-rows", "one-row", "frame-invalid", "runs")          # what a tall frame adds


def _call(driver, tmp, d, phase, inplace, pad=0):
    """d int16 [n,H,W] at 2-byte phase `phase` (0 .. 7) of a 16-byte block, frames pad elements apart beyond their size"""
    n, H, W = d.shape
    want = FR.fill(d)
    stride = H * W + pad
    nws = E.query(driver, "v3d_fill_holes_ws_bytes", n, H)
    assert nws == (n * H + 15) // 16 * 16

    def make(gp):
        src = np.full((n - 1) * stride + H * W, gp * 257, np.uint16).view(np.int16)
        for f in range(n):
            src[f * stride:f * stride + H * W] = d[f].reshape(-1)
        buf, off = E.chunked("disp", src, 2 * phase, gp)
        ws = E.exact("ws", np.full(nws, gp, np.uint8), 32, expect=None)
        if inplace:
            assert pad == 0
            buf.expect = buf.image.copy()
            buf.expect[off:off + 2 * want.size] = want.reshape(-1).view(np.uint8)
            return [(buf, off), stride, n, W, H, (buf, off), ws, 0]
        out = E.exact("out", np.full(2 * want.size, gp, np.uint8), 2 * ((phase * 3 + 1) % 8), expect=want.reshape(-1).view(np.uint8))
        return [(buf, off), stride, n, W, H, out, ws, 0]
    E.run_configs(driver, tmp, ENTRY, make)


@pytest.mark.parametrize("H", [1, 5, 33])
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_phases_patterns(driver, tmp_path, W, H):
    n = 2 if H == 5 else 1
    for i, (name, d) in enumerate(patterns(n, H, W, W * 131 + H).items()):
        if H == 33 and name not in ROW_PATTERNS:
            continue
        inplace = i % 2 == 1
        _call(driver, tmp_path, d, (i + W) % 8, inplace, pad=0 if inplace else 3 * (n - 1))


@pytest.mark.parametrize("inplace", [False, True])
def test_a_source_row_more_than_256_rows_away(driver, tmp_path, inplace):
    rng = np.random.default_rng(300)
    d = np.full((1, 300, 3), -16, np.int16)
    d[0, 0] = rng.integers(0, 1024, 3)
    d[0, 0, 1] = -1
    _call(driver, tmp_path, d, 5, inplace)


@pytest.mark.parametrize("W,H", [(7, 5), (2042, 2), (3, 70)])
def test_a_frame_with_no_valid_pixel_is_copied(driver, tmp_path, W, H):
    d = np.random.default_rng(W).integers(-32768, 0, (1, H, W)).astype(np.int16)
    _call(driver, tmp_path, d, 3, False)
    _call(driver, tmp_path, d, 6, True)
