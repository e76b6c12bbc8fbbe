"""csrc/v3d_colour.hip without a GPU: the kernel source runs in the stand-alone emulator driver (tests/emu_case.py), plain and under
AddressSanitizer / UndefinedBehaviorSanitizer, in both configurations, and must equal tests/colour_ref.py bit for bit.
The histogram's image lies in exactly the aligned 16-byte blocks that hold its payload (what the header lets the entry read), so the
rectangle's last row ends in the allocation's last block; the images of the apply entry start on their first payload byte and end on
their last: it may touch nothing but the rectangle.  Padding between rows and frames is poisoned."""
import numpy as np
import pytest

import colour_ref as CR
import emu_case as E
from test_colour_ref import lut_cases

HIST, LUT, APPLY = "v3d_bgr_hist_batch", "v3d_colour_lut_batch", "v3d_bgr_lut_batch"
driver = E.driver_fixture("colour", ["v3d_colour.hip"], [HIST, LUT, APPLY])


def _frames(n, H, W, seed, smooth=False):
    rng = np.random.default_rng(seed)
    if smooth:                                                 # few levels, long runs: the contended bins
        return np.broadcast_to((np.arange(W) // 7 + seed)[None, None, :, None] % 5 * 50, (n, H, W, 3)).astype(np.uint8) + rng.integers(0, 2, (n, H, W, 3), dtype=np.uint8)
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _layout(F, pitch, stride, poison):
    """frames [n,H,W,3] -> the bytes from the first payload byte to the last, rows `pitch` and frames `stride` bytes apart"""
    n, H, W, _ = F.shape
    img = np.full((n - 1) * stride + (H - 1) * pitch + 3 * W, poison, np.uint8)
    for f in range(n):
        for y in range(H):
            o = f * stride + y * pitch
            img[o:o + 3 * W] = F[f, y].reshape(-1)
    return img


def _hist(driver, tmp, F, rect, phase=0, rowpad=0, framepad=0, rc=0, pitch=None, stride=None):
    n, H, W, _ = F.shape
    pitch = 3 * W + rowpad if pitch is None else pitch
    stride = H * max(pitch, 3 * W) + framepad if stride is None else stride
    want = CR.hist(F, rect) if rc == 0 else None
    x0, y0, x1, y1 = rect

    def make(gp):
        img, off = E.chunked("bgr", _layout(F, max(pitch, 3 * W), max(stride, 1), gp), phase, gp)
        out = E.exact("hist", np.full(n * 768 * 4, gp, np.uint8), 4, **({} if rc else {"expect": want.reshape(-1).view(np.uint8)}))
        return [(img, off), stride, n, W, H, pitch, x0, y0, x1, y1, out, 0]
    E.run_configs(driver, tmp, HIST, make, rc=rc)


@pytest.mark.parametrize("w", [1, 5, 16, 17, 341])
def test_histogram_widths_at_every_phase(driver, tmp_path, w):
    """the image base at an odd byte and an odd pitch: the rows' segments start at every byte of a 16-byte block"""
    W, H = w + 19, 5
    F = _frames(1, H, W, w)
    for x0 in range(0, 16, 3 if w > 100 else 1):
        _hist(driver, tmp_path, F, (x0, 1, x0 + w, H), phase=(2 * x0 + 1) % 16, rowpad=1 + x0 % 3)


def test_histogram_wide_rows_bands_and_frames(driver, tmp_path):
    """2731 pixels = 8193 bytes = 171 chunks a row, two rows to a band: a lane takes a second item and the items wrap over a row end;
    4200 pixels = 263 chunks: more than the workgroup's lanes in one row; three padded frames, several bands each, whose workgroups
    flush into one histogram; the whole image and its last pixel (the allocation's last block)"""
    F = _frames(1, 5, 2731, 1)
    _hist(driver, tmp_path, F, (0, 0, 2731, 5), phase=5)
    F = _frames(1, 3, 4200, 2)
    _hist(driver, tmp_path, F, (0, 0, 4200, 3), phase=15, rowpad=3)
    _hist(driver, tmp_path, F, (1, 0, 4200, 1), phase=0)
    F = _frames(3, 37, 90, 3, smooth=True)
    _hist(driver, tmp_path, F, (0, 0, 90, 37), phase=9, rowpad=5, framepad=7)
    _hist(driver, tmp_path, F, (3, 2, 88, 36), phase=3, rowpad=16, framepad=32)
    _hist(driver, tmp_path, F, (89, 36, 90, 37), phase=11, rowpad=5, framepad=7)
    _hist(driver, tmp_path, F, (0, 0, 1, 1), phase=11)
    F = np.full((1, 40, 60, 3), 77, np.uint8)                  # one bin per channel
    _hist(driver, tmp_path, F, (0, 0, 60, 40), phase=1)


def test_histogram_refusals(driver, tmp_path):
    F = _frames(2, 4, 6, 0)
    for rect in ((0, 0, 7, 4), (0, 0, 6, 5), (2, 0, 2, 4), (0, 3, 6, 3), (-1, 0, 6, 4), (0, -1, 6, 4), (4, 0, 3, 4)):
        _hist(driver, tmp_path, F, rect, rc=-1)
    _hist(driver, tmp_path, F, (0, 0, 6, 4), pitch=17, rc=-1)
    _hist(driver, tmp_path, F, (0, 0, 6, 4), stride=4 * 18 - 1, rc=-1)


@pytest.mark.parametrize("case", lut_cases(), ids=lambda c: c[0])
def test_tables(driver, tmp_path, case):
    name, s, d, group, _ = case
    want = CR.lut(s, d, group)

    def make(gp):
        hs = E.exact("hist_src", s.astype(np.uint32).reshape(-1).view(np.uint8), 4)
        hd = E.exact("hist_dst", d.astype(np.uint32).reshape(-1).view(np.uint8), 8)
        out = E.exact("lut", np.full(want.size, gp, np.uint8), 1, expect=want.reshape(-1))
        return [hs, hd, s.shape[0], group, out, 0]
    E.run_configs(driver, tmp_path, LUT, make)


def test_table_refusals(driver, tmp_path):
    s = np.zeros((2, 3, 256), np.uint32)
    for n, group in ((2, 0), (2, 3), (0, 1)):
        def make(gp):
            hs, hd = E.exact("hist_src", s.reshape(-1).view(np.uint8), 4), E.exact("hist_dst", s.reshape(-1).view(np.uint8), 4)
            return [hs, hd, n, group, E.exact("lut", np.full(2 * 768, gp, np.uint8), 0), 0]
        E.run_configs(driver, tmp_path, LUT, make, rc=-1)


def _apply(driver, tmp, F, T, rect, in_place, sphase=0, dphase=0, srowpad=0, drowpad=0, sframepad=0, dframepad=0, rc=0, lut_stride=None):
    n, H, W, _ = F.shape
    sp, dp = 3 * W + srowpad, 3 * W + (srowpad if in_place else drowpad)
    ss, ds = H * sp + sframepad, H * dp + (sframepad if in_place else dframepad)
    x0, y0, x1, y1 = rect
    per_frame = T.ndim == 3 and T.shape[0] == n and n > 1
    ls = (768 + 5 if per_frame else 0) if lut_stride is None else lut_stride
    want = CR.apply(F, T, rect) if rc == 0 else F

    def make(gp):
        tab = np.full(((n - 1) * ls if per_frame else 0) + 768, gp, np.uint8)
        for f in range(n if per_frame else 1):
            tab[f * ls:f * ls + 768] = (T[f] if T.ndim == 3 else T).reshape(-1)
        lut = E.exact("lut", tab, 3)
        if in_place:
            io = E.exact("img", _layout(F, sp, ss, gp), sphase, expect=_layout(want, sp, ss, gp))
            return [io, ss, n, W, H, sp, x0, y0, x1, y1, lut, ls, io, ds, dp, 0]
        src = E.exact("src", _layout(F, sp, ss, gp), sphase)
        blank = np.full(F.shape, gp, np.uint8)
        if rc == 0:
            blank[:, y0:y1, x0:x1] = want[:, y0:y1, x0:x1]
        dst = E.exact("dst", _layout(blank, dp, ds, gp), dphase, expect=_layout(blank, dp, ds, gp))
        return [src, ss, n, W, H, sp, x0, y0, x1, y1, lut, ls, dst, ds, dp, 0]
    E.run_configs(driver, tmp, APPLY, make, rc=rc)


def test_apply_in_place_at_every_phase(driver, tmp_path):
    """the right half of a frame, as the pipeline calls it: edges at every byte of a block, one table and one per frame"""
    F = _frames(2, 4, 46, 4)
    rng = np.random.default_rng(1)
    shared, per = rng.integers(0, 256, (3, 256), dtype=np.uint8), rng.integers(0, 256, (2, 3, 256), dtype=np.uint8)
    for ph in range(16):
        _apply(driver, tmp_path, F, per if ph % 2 else shared, (23 - ph % 5, ph % 2, 46 - ph % 3, 4), True, sphase=ph, srowpad=ph % 4,
               sframepad=ph % 7)


def test_apply_out_of_place_both_routes(driver, tmp_path):
    """source and destination at the same byte of a block with pitches 16 apart (aligned 16-byte loads), and at different ones
    (byte loads); a row longer than the workgroup's 256 blocks; a single pixel; every byte outside the rectangle keeps its poison"""
    rng = np.random.default_rng(2)
    T = rng.integers(0, 256, (3, 3, 256), dtype=np.uint8)
    F = _frames(3, 5, 50, 5)
    _apply(driver, tmp_path, F, T, (0, 0, 50, 5), False, sphase=6, dphase=6, srowpad=2, drowpad=18, sframepad=3, dframepad=35)
    _apply(driver, tmp_path, F, T, (7, 1, 41, 4), False, sphase=6, dphase=6, srowpad=2, drowpad=18, sframepad=3, dframepad=35)
    for dphase in (0, 7, 15):
        _apply(driver, tmp_path, F, T[0], (7, 1, 41, 4), False, sphase=3, dphase=dphase, srowpad=1, drowpad=4, dframepad=9)
    F = _frames(1, 2, 1500, 6)
    _apply(driver, tmp_path, F, T[1], (1, 0, 1500, 2), False, sphase=1, dphase=1)
    _apply(driver, tmp_path, F, T[1], (1499, 1, 1500, 2), False, sphase=1, dphase=2)
    _apply(driver, tmp_path, F, T[1], (0, 0, 1500, 2), True, sphase=13)


def test_apply_refusals(driver, tmp_path):
    F = _frames(2, 4, 6, 0)
    T = np.zeros((3, 256), np.uint8)
    _apply(driver, tmp_path, F, T, (0, 0, 7, 4), False, rc=-1)
    _apply(driver, tmp_path, F, T, (3, 0, 3, 4), True, rc=-1)
    _apply(driver, tmp_path, F, T, (0, 0, 6, 4), False, lut_stride=767, rc=-1)
    _apply(driver, tmp_path, F, T, (0, 0, 6, 4), False, drowpad=-1, rc=-1)
    _apply(driver, tmp_path, F, T, (0, 0, 6, 4), False, dframepad=-1, rc=-1)

    def overlapping(gp):                                       # the destination one row below the source, inside its extent
        img = E.exact("img", np.full(2 * 4 * 18 + 18, gp, np.uint8), 0)
        return [img, 72, 2, 6, 4, 18, 0, 0, 6, 4, E.exact("lut", T.reshape(-1), 0), 0, (img, 18), 72, 18, 0]
    E.run_configs(driver, tmp_path, APPLY, overlapping, rc=-1)
