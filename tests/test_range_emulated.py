"""csrc/v3d_range.hip itself, without a GPU: the kernel source runs in the stand-alone emulator driver (tests/emu_case.py), plain
and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/range_ref.py and tests/temporal_ref.py bit for bit:
the robust range at q = 50 % and 100 %, the plain min / max, and both normalisations.  Frames of 1, 35 and 8481 elements (one
lane, less than a wave, two 4096-pixel steps and a ragged third with one element past the last group of 4), aligned with strides of whole 16-byte groups (the
vector route) and 4 bytes off with an odd stride (the element route); the clip ends on its heap block's last byte."""
import numpy as np
import pytest

import emu_case as E
import range_ref as RR
import temporal_ref as TR

ENTRIES = ["v3d_depth_robust_minmax_batch", "v3d_depth_robust_minmax_ws_bytes", "v3d_depth_minmax_batch", "v3d_depth_to_u16_batch",
           "v3d_depth_to_u16_range_batch"]
driver = E.driver_fixture("range", ["v3d_range.hip"], ENTRIES)
SHAPES = [(1, 1), (5, 7), (257, 33)]
T = 4


def _clip(W, H):
    """frames of a matcher's kind (multiples of 1/16, a fifth invalid), off the grid, with samples at and above the last bin,
    and one whose valid values all share one histogram bin"""
    rng = np.random.default_rng(W * 31 + H)
    d = (rng.integers(1, 1024, (T, H, W)) / 16).astype(np.float32)
    d[rng.random((T, H, W)) < 0.2] = 0.0
    d[1] += (rng.random((H, W)) < 0.5) * np.float32(1 / 64)
    d[1][rng.random((H, W)) < 0.1] = -3.5
    d[2][rng.random((H, W)) < 0.3] = 2047 / 16
    d[2].reshape(-1)[0] = 3000.0
    d[3] = np.where(rng.random((H, W)) < 0.3, 0.0, 12.5).astype(np.float32)
    d[3].reshape(-1)[-1] = 12.5
    return d


def _bytes(d, stride, gp):
    n, per = d.shape[0], d[0].size
    img = np.full(((n - 1) * stride + per) * 4, gp, np.uint8)
    for f in range(n):
        img[f * stride * 4:(f * stride + per) * 4] = d[f].reshape(-1).view(np.uint8)
    return img


def _f32(v):
    return np.ascontiguousarray(v, np.float32).reshape(-1).view(np.uint8)


LAYOUTS = {"vector": (0, 4), "element": (4, 3)}                     # base skew in bytes, stride padding in elements


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("q", [5000, 10000])
@pytest.mark.parametrize("W,H", SHAPES)
def test_robust_range(driver, tmp_path, W, H, q, layout):
    d = _clip(W, H)
    skew, pad = LAYOUTS[layout]
    stride = W * H + pad + (-(W * H) % 4 if layout == "vector" else 0)
    want = RR.robust_minmax(d, q)
    assert want[3, 1] == np.float32(12.5)                             # one bin holds every valid pixel: it is the white point
    nws = E.query(driver, ENTRIES[1], T)

    def make(gp):
        return [E.exact("depth", _bytes(d, stride, gp), skew), T, W * H, stride, q, E.exact("ws", np.full(nws, gp, np.uint8), 16, expect=None),
                E.exact("out", np.full(8 * T, gp, np.uint8), 4, expect=_f32(want)), 0]
    E.run_configs(driver, tmp_path, ENTRIES[0], make)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_minmax_and_both_normalisations(driver, tmp_path, W, H, layout):
    d = _clip(W, H)
    skew, pad = LAYOUTS[layout]
    stride = W * H + pad
    mm = TR.minmax(d)
    own = TR.to_u16_range(d, mm)
    lohi = RR.robust_minmax(d, 9000)
    ranged = TR.to_u16_range(d, lohi)
    u16 = lambda name, w, gp: E.exact(name, np.full(2 * w.size, gp, np.uint8), 2, expect=w.reshape(-1).view(np.uint8))
    E.run_configs(driver, tmp_path, ENTRIES[2], lambda gp: [E.exact("depth", _bytes(d, stride, gp), skew), T, W * H, stride,
                                                           E.exact("out", np.full(8 * T, gp, np.uint8), 4, expect=_f32(mm)), 0])
    E.run_configs(driver, tmp_path, ENTRIES[3], lambda gp: [E.exact("depth", _bytes(d, stride, gp), skew), T, W * H, stride, u16("out", own, gp),
                                                           E.exact("ws", np.full(8 * T, gp, np.uint8), 4, expect=None), 0])
    E.run_configs(driver, tmp_path, ENTRIES[4], lambda gp: [E.exact("depth", _bytes(d, stride, gp), skew), T, W * H, stride,
                                                           E.exact("lohi", _f32(lohi), 4), u16("out", ranged, gp), 0])
