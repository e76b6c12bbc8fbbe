"""csrc/v3d_stereo.hip itself (both entries), without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/stereo_ref.py and
tests/stereo_sub_ref.py byte for byte.  Widths on both sides of every change of pixels per thread (8 up to 2048, 16 up to 4096,
32 above) and widths that end inside a thread's run; one band of 4 rows plus one of 1.  k_render_stereo reads the aligned 16-byte
blocks that cover a row, so the frame and the depth lie in exactly the blocks that hold their payload, at several phases, with
the slack poisoned: a block without payload must not be loaded, and the slack must not reach the output."""
import numpy as np
import pytest

import emu_case as E
import stereo_ref as R
import stereo_sub_ref as S

ENTRIES = ["v3d_render_stereo_batch", "v3d_render_stereo_subpixel_batch"]
driver = E.driver_fixture("stereo", ["v3d_stereo.hip"], ENTRIES)
REF = {ENTRIES[0]: R.render, ENTRIES[1]: S.render}
GMAX = (1 << 24) - 1
WIDTHS = [1, 7, 255, 2047, 2048, 2049, 4090, 4096, 4097, 8190, 8192]


def _gains(W):
    """zero, the defaults, +-(2^24 - 1) at both ends of the convergence, a shift of at least W"""
    return [(0, 0, 32768), R.stereo_gains(), (GMAX, -GMAX, 0), (-GMAX, GMAX, 65535), (W * 256 + 77, -(W * 256 + 77), 0)]


def _call(driver, tmp, entry, F, D, gl, gr, conv, layout, fphase, dphase, fpad=0, dpad=0):
    """F u8 [n,H,W,3], D u16 [n,H,W]; frames fpad bytes / dpad elements apart beyond their size"""
    n, H, W = D.shape
    want = np.stack([REF[entry](F[i], D[i], gl, gr, conv, layout) for i in range(n)])
    fs, ds = H * W * 3 + fpad, H * W + dpad

    def make(gp):
        fb = np.full((n - 1) * fs + H * W * 3, gp, np.uint8)
        db = np.full((n - 1) * ds + H * W, gp * 257, np.uint16)
        for i in range(n):
            fb[i * fs:i * fs + H * W * 3] = F[i].reshape(-1)
            db[i * ds:i * ds + H * W] = D[i].reshape(-1)
        (fbuf, foff), (dbuf, doff) = E.chunked("frame", fb, fphase, gp), E.chunked("depth", db, dphase, gp)
        out = E.exact("out", np.full(want.size, gp, np.uint8), (fphase * 5 + 1) % 16, expect=want.reshape(-1))
        return [(fbuf, foff), fs, (dbuf, doff), ds, n, W, H, gl, gr, conv, layout, out, 0]
    E.run_configs(driver, tmp, entry, make)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_gains_and_layouts(driver, tmp_path, W, H, entry):
    F = np.random.default_rng(W).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    for i, (gl, gr, conv) in enumerate(_gains(W)):
        kind = ("noise", "planar")[(i + H) % 2]
        D = S.scene_depth(kind, H, W, W + H + i)[None]
        layout = (i + H // 2) % 2 if W % 2 == 0 else R.FULL_SBS             # both layouts at every even width
        _call(driver, tmp_path, entry, F, D, gl, gr, conv, layout, (3 * i + W) % 16, 2 * ((i + W + H) % 8))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("layout", [R.FULL_SBS, R.HALF_SBS])
def test_nearest_key_beyond_a_wave_or_absent(driver, tmp_path, entry, layout):
    F, D, (gl, gr, conv) = R.far_key_scene()
    _call(driver, tmp_path, entry, F[None], D[None], gl, gr, conv, layout, 9, 6)


@pytest.mark.parametrize("entry", ENTRIES)
def test_two_frames_at_an_odd_offset_and_a_padded_stride(driver, tmp_path, entry):
    n, H, W = 2, 5, 333
    F = np.random.default_rng(8).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([S.scene_depth(("planar", "steep")[i], H, W, 100 + i) for i in range(n)])
    gl, gr, conv = R.stereo_gains(80, 0.4, 0.3)
    _call(driver, tmp_path, entry, F, D, gl, gr, conv, R.FULL_SBS, 5, 2, fpad=45, dpad=7)
