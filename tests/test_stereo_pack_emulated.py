"""v3d_render_stereo_packed_batch of csrc/v3d_stereo.hip, without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/stereo_pack_ref.py byte
for byte.  Widths on both sides of every change of pixels per thread (8 up to 2048, 16 up to 4096, 32 above) and widths that end
inside a thread's run; H = 2 (one row pair, one left-eye and one right-eye row) and H = 6 (a band of 4 rows plus a ragged band
that holds one pair); every new packing, both renderers.  As in tests/test_stereo_emulated.py the frame and the depth lie in
exactly the 16-byte blocks that hold their payload, at several phases, with the slack poisoned, and the output ends on its last
byte: the words a thread parks in LDS (the even row of half top-bottom, the left eye of an anaglyph) must come back as they were
under both thread orders and both LDS poisons."""
import numpy as np
import pytest

import emu_case as E
import stereo_pack_ref as P
import stereo_ref as R
import stereo_sub_ref as S

ENTRY = "v3d_render_stereo_packed_batch"
driver = E.driver_fixture("stereo_pack", ["v3d_stereo.hip"], [ENTRY])
GMAX = (1 << 24) - 1
WIDTHS = [1, 7, 255, 2047, 2048, 2049, 4097, 8192]
NEW = (P.FULL_TB, P.HALF_TB, P.ROWS, P.ANAGLYPH_COLOUR, P.ANAGLYPH_DUBOIS)


def _gains(W):
    """zero, the defaults, +-(2^24 - 1) at both ends of the convergence, a shift of at least W"""
    return [(0, 0, 32768), R.stereo_gains(), (GMAX, -GMAX, 0), (-GMAX, GMAX, 65535), (W * 256 + 77, -(W * 256 + 77), 0)]


def _call(driver, tmp, F, D, gl, gr, conv, sub, packing, fphase, dphase, fpad=0, dpad=0):
    """F u8 [n,H,W,3], D u16 [n,H,W]; frames fpad bytes / dpad elements apart beyond their size"""
    n, H, W = D.shape
    want = np.stack([P.render(F[i], D[i], gl, gr, conv, packing, bool(sub)) for i in range(n)])
    fs, ds = H * W * 3 + fpad, H * W + dpad

    def make(gp):
        fb = np.full((n - 1) * fs + H * W * 3, gp, np.uint8)
        db = np.full((n - 1) * ds + H * W, gp * 257, np.uint16)
        for i in range(n):
            fb[i * fs:i * fs + H * W * 3] = F[i].reshape(-1)
            db[i * ds:i * ds + H * W] = D[i].reshape(-1)
        (fbuf, foff), (dbuf, doff) = E.chunked("frame", fb, fphase, gp), E.chunked("depth", db, dphase, gp)
        out = E.exact("out", np.full(want.size, gp, np.uint8), (fphase * 5 + 1) % 16, expect=want.reshape(-1))
        return [(fbuf, foff), fs, (dbuf, doff), ds, n, W, H, gl, gr, conv, sub, packing, out, 0]
    E.run_configs(driver, tmp, ENTRY, make)


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("W", WIDTHS)
def test_widths_gains_and_packings(driver, tmp_path, W, H, sub):
    F = np.random.default_rng(W).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    gains = _gains(W)
    for i, packing in enumerate(NEW):                          # five packings, five gain sets: rotated by width, height and renderer
        gl, gr, conv = gains[(i + W + H // 2 + sub) % len(gains)]
        kind = ("noise", "planar")[(i + H // 2) % 2]
        D = S.scene_depth(kind, H, W, W + H + i)[None]
        _call(driver, tmp_path, F, D, gl, gr, conv, sub, packing, (3 * i + W) % 16, 2 * ((i + W + H) % 8))


# the row staging is sized to the byte for 8192 pixels whose BGR row starts at byte 15 of a 16-byte block (1537 chunks) and whose
# depth row starts at byte 14 (1025 chunks), the parked words right behind: the dynamic LDS of the side-by-side march is a heap block
# of the launch's size, the static LDS of the anaglyph march an array of st_lds_bytes, and AddressSanitizer has a red zone behind each
@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("packing", [P.FULL_SBS, P.ANAGLYPH_DUBOIS])
def test_widest_row_at_the_worst_alignment(driver, tmp_path, packing, sub):
    W, H = 8192, 2
    F = np.random.default_rng(15).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    D = S.scene_depth("planar", H, W, 14 + sub)[None]
    _call(driver, tmp_path, F, D, *R.stereo_gains(60, 0.5, 0.5), sub, packing, 15, 14)


@pytest.mark.parametrize("sub", [0, 1])
def test_nearest_key_beyond_a_wave_or_absent(driver, tmp_path, sub):
    F, D, (gl, gr, conv) = R.far_key_scene()
    for packing in NEW:
        _call(driver, tmp_path, F[None], D[None], gl, gr, conv, sub, packing, 9, 6)


@pytest.mark.parametrize("sub", [0, 1])
def test_two_frames_at_an_odd_offset_and_a_padded_stride(driver, tmp_path, sub):
    n, H, W = 2, 6, 333
    F = np.random.default_rng(8).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([S.scene_depth(("planar", "steep")[i], H, W, 100 + i) for i in range(n)])
    gl, gr, conv = R.stereo_gains(80, 0.4, 0.3)
    for packing in NEW:
        _call(driver, tmp_path, F, D, gl, gr, conv, sub, packing, 5, 2, fpad=45, dpad=7)


def test_codes_0_and_1_and_a_refusal(driver, tmp_path):
    """the two side-by-side layouts through the packed entry, and a refused call that writes nothing"""
    H, W = 5, 38
    F = np.random.default_rng(2).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    D = S.scene_depth("planar", H, W, 3)[None]
    gl, gr, conv = R.stereo_gains()
    for sub in (0, 1):
        for packing in (P.FULL_SBS, P.HALF_SBS):
            _call(driver, tmp_path, F, D, gl, gr, conv, sub, packing, 3, 4)

    def make(gp):
        (fbuf, foff), (dbuf, doff) = E.chunked("frame", F.reshape(-1), 0, gp), E.chunked("depth", D.reshape(-1), 0, gp)
        out = E.exact("out", np.full(H * W * 3, gp, np.uint8), 0)                 # expected unchanged
        return [(fbuf, foff), H * W * 3, (dbuf, doff), H * W, 1, W, H, gl, gr, conv, 0, P.HALF_TB, out, 0]
    E.run_configs(driver, tmp_path, ENTRY, make, rc=-1)                           # odd H
