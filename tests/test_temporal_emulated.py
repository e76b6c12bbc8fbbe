"""csrc/v3d_temporal.hip itself (cuts, window range, the plain filter), without a GPU: the kernel sources run in the stand-alone
emulator driver (tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal
tests/temporal_ref.py bit for bit.  Sizes of one lane, less than a row of lanes, one 256 x 4 tile exactly and one column / row
more; radius 0, 1 and the largest, with a scene cut inside the window; fill 0 and 1; aligned clips with strides of whole 16-byte
groups (the vector route where W is a multiple of 4) and clips at odd bases with odd strides (the element route).  Every clip ends
on its heap block's last byte."""
import numpy as np
import pytest

import emu_case as E
import temporal_ref as TR

KERNELS = ["v3d_temporal.hip", "v3d_temporal_mc.hip"]
ENTRIES = ["v3d_temporal_cuts", "v3d_temporal_range", "v3d_temporal_filter_batch", "v3d_temporal_motion", "v3d_temporal_filter_mc_batch"]
driver = E.driver_fixture("temporal", KERNELS, ENTRIES)
SHAPES = [(1, 1), (3, 2), (63, 5), (256, 8), (257, 9)]
LAYOUTS = {"aligned": (0, 0, 16), "odd": (4, 3, 5)}                # skew of depth (bytes) and of gray, stride padding (elements)


def clip(T, H, W, seed, cut_at=None):
    """depth with invalid, negative, NaN and off-grid samples inside the filters' domain; luma that drifts a little, and steps at
    frame cut_at"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 1024, (1, H, W))
    d = (np.clip(base + rng.integers(-40, 41, (T, H, W)), -30, 32767) / 16).astype(np.float32)
    d += (rng.random((T, H, W)) < 0.3) * np.float32(1 / 64)
    d[rng.random((T, H, W)) < 0.05] = np.nan
    d[rng.random((T, H, W)) < 0.1] = -3.5
    d[rng.random((T, H, W)) < 0.1] = 0.0
    g = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-5, 6, (T, H, W)), 0, 255).astype(np.uint8)
    if cut_at is not None:
        g[cut_at:] = 255 - g[cut_at:]
    return d, g


def planes(a, stride, gp):
    """[T,H,W] -> bytes, frames `stride` elements apart, ending on the last payload byte"""
    T, per, item = a.shape[0], a[0].size, a.itemsize
    img = np.full(((T - 1) * stride + per) * item, gp, np.uint8)
    for f in range(T):
        img[f * stride * item:(f * stride + per) * item] = np.ascontiguousarray(a[f]).reshape(-1).view(np.uint8)
    return img


def raw(v, dtype):
    return np.ascontiguousarray(v, dtype).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_cuts_and_window_range(driver, tmp_path, W, H, layout):
    T = 6
    d, g = clip(T, H, W, W + H, cut_at=3)
    _, gskew, pad = LAYOUTS[layout]
    gstride = W * H + pad + (-(W * H) % 16 if layout == "aligned" else 0)
    for c in (0, 20, 256):
        cut = TR.cuts(g, c)
        E.run_configs(driver, tmp_path, ENTRIES[0], lambda gp: [
            E.exact("gray", planes(g, gstride, gp), gskew), gstride, T, W, H, c, E.exact("ws", np.full(8 * T, gp, np.uint8), 8, expect=None),
            E.exact("cut", np.full(T, gp, np.uint8), 3, expect=cut), 0])
    assert TR.cuts(g, 20).tolist() == [0, 0, 0, 1, 0, 0]
    finite = np.nan_to_num(d, nan=0.0)
    mm = TR.minmax(finite)
    for R, t0, n in ((0, 0, T), (1, 1, 4), (8, 0, T)):
        want = TR.ranges(mm, cut := TR.cuts(g, 20), R, t0, n)
        E.run_configs(driver, tmp_path, ENTRIES[1], lambda gp: [
            E.exact("mm", raw(mm, np.float32), 4), E.exact("cut", cut, 1), T, t0, n, R,
            E.exact("lohi", np.full(8 * n, gp, np.uint8), 4, expect=raw(want, np.float32)), 0])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", [0, 1, 8])
@pytest.mark.parametrize("W,H", SHAPES)
def test_filter(driver, tmp_path, W, H, R, layout):
    T = 2 * R + 3 if R < 8 else 11
    d, g = clip(T, H, W, 7 * W + H + R, cut_at=T // 2 + 1)            # inside the window of the targets around it
    cut = TR.cuts(g, 20)
    assert cut.sum() == 1
    dskew, gskew, pad = LAYOUTS[layout]
    dstride = gstride = W * H + pad + (-(W * H) % 4 if layout == "aligned" else 0)
    for fill, (t0, n) in ((1, (0, T)), (0, (1, T - 2))):
        want = TR.filter_clip(d, g, R, 12, cut, fill, t0, n)
        E.run_configs(driver, tmp_path, ENTRIES[2], lambda gp: [
            E.exact("depth", planes(d, dstride, gp), dskew), dstride, E.exact("gray", planes(g, gstride, gp), gskew), gstride, T, W, H, t0, n,
            R, 12, fill, E.exact("cut", cut, 1), E.exact("out", np.full(4 * want.size, gp, np.uint8), dskew, expect=raw(want, np.float32)), 0])
