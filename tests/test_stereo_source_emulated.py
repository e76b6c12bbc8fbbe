"""v3d_render_stereo_source_batch of csrc/v3d_stereo.hip, without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/stereo_source_ref.py byte
for byte.  The frame and the depth lie in exactly the 16-byte blocks that hold their payload, as in
tests/test_stereo_pack_emulated.py; the SBS frames end on their last payload byte and start on their first (the entry reads them
byte by byte: "payload only"), with pitched rows and padded frames whose slack is poisoned."""
import numpy as np
import pytest

import emu_case as E
import stereo_pack_ref as P
import stereo_ref as R
import stereo_source_ref as X
import stereo_sub_ref as S

ENTRY = "v3d_render_stereo_source_batch"
driver = E.driver_fixture("stereo_source", ["v3d_stereo.hip"], [ENTRY])
MAPS = [(65536, 0, 65536, 0), (21845, -9000, 30000, 77), (200000, -3 << 16, 150000, 5 << 16), (4096, 1 << 30, 1 << 20, -(1 << 30))]


def _call(driver, tmp, F, D, gains, sub, packing, sbs, fill, m, rowpad=0, framepad=0, rc=0, fphase=5, dphase=6, want=None):
    """F u8 [n,H,W,3], D u16 [n,H,W], sbs u8 [n,Hs,Ws,3]; SBS rows rowpad bytes, frames framepad bytes apart beyond their size; the
    frame and the depth at bytes fphase and dphase of a 16-byte block; want: the expected frames where the caller has them"""
    n, H, W = D.shape
    Hs, Ws = sbs.shape[1:3]
    if rc:                                                     # a refused call: the poisoned output stays as it is
        ow, oh = P.output_size(packing, W, H)
        want = np.zeros((n, oh, ow, 3), np.uint8)
    elif want is None:
        want = np.stack([X.render(F[i], D[i], *gains, packing, bool(sub), sbs[i], fill, *m) for i in range(n)])
    pitch = 3 * Ws + rowpad
    ss = Hs * pitch + framepad

    def make(gp):
        (fbuf, foff), (dbuf, doff) = E.chunked("frame", F.reshape(-1), fphase, gp), E.chunked("depth", D.reshape(-1), dphase, gp)
        sb = np.full((n - 1) * ss + (Hs - 1) * pitch + 3 * Ws, gp, np.uint8)     # ends on the last payload byte
        for i in range(n):
            for j in range(Hs):
                sb[i * ss + j * pitch:i * ss + j * pitch + 3 * Ws] = sbs[i, j].reshape(-1)
        out = E.exact("out", np.full(want.size, gp, np.uint8), 7, **({} if rc else {"expect": want.reshape(-1)}))
        return [(fbuf, foff), H * W * 3, (dbuf, doff), H * W, n, W, H, *gains, sub, packing, E.exact("sbs", sb, 3), ss, Ws, Hs, pitch,
                fill, *m, out, 0]
    E.run_configs(driver, tmp, ENTRY, make, rc=rc)


def _scene(n, W, H, Ws, Hs, seed, kinds=("planar", "noise", "steep")):
    rng = np.random.default_rng(seed)
    F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    sbs = rng.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
    return F, np.stack([S.scene_depth(kinds[i % len(kinds)], H, W, seed + i) for i in range(n)]), sbs


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (255, 5), (254, 6), (2050, 3), (4100, 2)])
def test_sizes_packings_and_fills(driver, tmp_path, W, H, sub):
    F, D, sbs = _scene(1, W, H, 6 if W < 100 else 322, 2 if W < 100 else 45, W + sub)
    packs = [p for p in P.PACKINGS if not (p == P.HALF_SBS and W % 2) and not (p == P.HALF_TB and H % 2)]
    for fill in (1, 2, 3):
        packing = packs[(fill + W + sub) % len(packs)]
        gains = [R.stereo_gains(24, 0.5, 0.5), R.stereo_gains(40, 0.5, 0.0), (W * 256 + 77, -(W * 256 + 77), 0)][(fill + H) % 3]
        _call(driver, tmp_path, F, D, gains, sub, packing, sbs, fill, MAPS[(fill + W) % len(MAPS)])


# every instantiation with a source that is wider than 8 pixels per thread (16 up to 4096, 32 above), both renderers, all seven
# packings, both eyes filled; H = 2: one row pair.  The 8-pixel ones run above
WIDE_SIZES = [(2050, 2), (4100, 2)]


def test_every_source_instantiation_is_launched():
    """the 3 x 2 x 5 instantiations k_render_stereo<PPT, SUB, K, StSource> against the cases of test_every_packing"""
    k_of = {P.FULL_SBS: "sbs", P.HALF_SBS: "sbs", P.FULL_TB: "tb", P.HALF_TB: "htb", P.ROWS: "rows", P.ANAGLYPH_COLOUR: "ana",
            P.ANAGLYPH_DUBOIS: "ana"}
    ppt = lambda W: 8 if W <= 2048 else 16 if W <= 4096 else 32
    cases = {(ppt(W), sub, k_of[p]) for W, H in WIDE_SIZES + [(254, 6)] for sub in (0, 1) for p in P.PACKINGS if P.output_size(p, W, H)}
    assert cases == {(n, sub, k) for n in (8, 16, 32) for sub in (0, 1) for k in ("sbs", "tb", "htb", "rows", "ana")} and len(cases) == 30


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("W,H", WIDE_SIZES + [(254, 6)])
def test_every_packing(driver, tmp_path, W, H, sub):
    F, D, sbs = _scene(1, W, H, 322, 45, W + 7 + sub, kinds=("planar",))
    gains = R.stereo_gains(60, 0.5, 0.5)
    EL, ER = X.eyes(F[0], D[0], *gains, bool(sub), sbs[0], 3, *MAPS[1])
    plain = P.eyes(F[0], D[0], *gains, bool(sub))
    assert (EL != plain[0]).any() and (ER != plain[1]).any()    # the fill does change both eyes
    for packing in P.PACKINGS:
        _call(driver, tmp_path, F, D, gains, sub, packing, sbs, 3, MAPS[1], want=P.pack(EL, ER, packing)[None])


# the row staging is sized to the byte for 8192 pixels whose BGR row starts at byte 15 of a 16-byte block (1537 chunks) and whose
# depth row starts at byte 14 (1025 chunks), the parked words right behind: under AddressSanitizer the dynamic LDS of the side-by-side
# march is a heap block of the launch's size and the static LDS of the anaglyph march an array of st_lds_bytes, each with a red zone
# right behind.  3 * 8192 and 2 * 8192 are multiples of 16: both rows have these offsets
@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("packing", [P.FULL_SBS, P.ANAGLYPH_DUBOIS])
def test_widest_row_at_the_worst_alignment(driver, tmp_path, packing, sub):
    F, D, sbs = _scene(1, 8192, 2, 322, 45, 15 + sub, kinds=("planar",))
    _call(driver, tmp_path, F, D, R.stereo_gains(60, 0.5, 0.5), sub, packing, sbs, 3, MAPS[1], fphase=15, dphase=14)


@pytest.mark.parametrize("sub", [0, 1])
def test_holes_longer_than_a_waves_run(driver, tmp_path, sub):
    F, D, gains = R.far_key_scene()
    sbs = np.random.default_rng(4).integers(0, 256, (1, 3, 64, 3), dtype=np.uint8)
    _call(driver, tmp_path, F[None], D[None], gains, sub, P.FULL_SBS, sbs, 3, (4096, -5000, 98304, 0))


@pytest.mark.parametrize("sub", [0, 1])
def test_three_frames_pitched_rows_and_padded_frames(driver, tmp_path, sub):
    F, D, sbs = _scene(3, 333, 6, 10, 4, 21)
    for packing in (P.FULL_TB, P.ANAGLYPH_DUBOIS):
        _call(driver, tmp_path, F, D, R.stereo_gains(80, 0.4, 0.3), sub, packing, sbs, 2, MAPS[1], rowpad=5, framepad=9)


@pytest.mark.parametrize("sub", [0, 1])
@pytest.mark.parametrize("Hs", [32768, 32769, 40000])
def test_rows_beyond_2_to_the_31_in_q16(driver, tmp_path, Hs, sub):
    """(Hs - 1) << 16 passes 2^31 from Hs = 32769 on: the bottom clamp and a blend of the last rows, with the SBS buffer ending on
    its last payload byte (a row coordinate narrowed to 32 bits reads far in front of it)"""
    rng = np.random.default_rng(Hs)
    F = rng.integers(0, 256, (1, 3, 7, 3), dtype=np.uint8)
    D = S.scene_depth("noise", 3, 7, Hs)[None]
    sbs = rng.integers(0, 256, (1, Hs, 2, 3), dtype=np.uint8)
    for m in ((65536, 0, 65536, 1 << 40), (65536, 0, 1 << 20, ((Hs - 34) << 16) + 32768)):
        _call(driver, tmp_path, F, D, R.stereo_gains(510, 0.5, 0.5), sub, P.FULL_SBS, sbs, 3, m)


def test_no_eye_filled_and_refusals(driver, tmp_path):
    F, D, sbs = _scene(2, 38, 5, 6, 2, 2)
    g = R.stereo_gains()
    _call(driver, tmp_path, F, D, g, 0, P.ROWS, sbs, 0, MAPS[0])
    for bad in ((4095, 0, 65536, 0), (65536, 0, (1 << 20) + 1, 0), (65536, (1 << 40) + 1, 65536, 0), (65536, 0, 65536, -(1 << 40) - 1)):
        _call(driver, tmp_path, F, D, g, 0, P.FULL_SBS, sbs, 2, bad, rc=-1)
    _call(driver, tmp_path, F, D, g, 0, P.FULL_SBS, sbs, 4, MAPS[0], rc=-1)
    _call(driver, tmp_path, F, D, g, 0, P.FULL_SBS, sbs, 2, MAPS[0], rowpad=-1, rc=-1)
    _call(driver, tmp_path, F, D, g, 2, P.FULL_SBS, sbs, 2, MAPS[0], rc=-1)
    wide = np.zeros((2, 1, 2 * 8193, 3), np.uint8)              # an eye wider than 8192 is unsupported, unless an argument is bad too
    _call(driver, tmp_path, F, D, g, 0, P.FULL_SBS, wide, 2, MAPS[0], rc=-3)
    _call(driver, tmp_path, F, D, (1 << 24, 0, 0), 0, P.FULL_SBS, wide, 2, MAPS[0], rc=-1)
