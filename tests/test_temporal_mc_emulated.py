"""csrc/v3d_temporal_mc.hip and the compensated filter of csrc/v3d_temporal.hip, without a GPU: the kernel sources run in the
stand-alone emulator driver (tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal
tests/temporal_mc_ref.py bit for bit.  Frames of one block, of blocks clipped to one column and row, of more than one block row
and of more than the four blocks of a workgroup; search radius 1 and the largest; fields that lead outside the frame.  Every clip
ends on its heap block's last byte."""
import numpy as np
import pytest

import emu_case as E
import temporal_mc_ref as MC
from test_temporal_emulated import ENTRIES, KERNELS, LAYOUTS, clip, planes, raw

driver = E.driver_fixture("temporal", KERNELS, ENTRIES)
SHAPES = [(16, 16), (17, 17), (33, 19), (70, 17)]


def _pan(T, H, W, seed, step):
    """a textured plane that moves `step` px per frame to the left and one row down, over a static noise floor"""
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + T + 2, W + step * T + 2)).astype(np.uint8)
    g = np.stack([big[T - t:T - t + H, step * t:step * t + W] for t in range(T)])
    return np.ascontiguousarray(g)


@pytest.mark.parametrize("S", [1, 32])
@pytest.mark.parametrize("W,H", SHAPES)
def test_motion_fields_residual_and_cuts(driver, tmp_path, W, H, S):
    T = 3
    g = _pan(T, H, W, W * 3 + H + S, min(S, 3))
    F, Bk, resid = MC.fields(g, S)
    BW, BH = MC.blocks(W, H)
    stride = W * H + 5
    for c in (0, 40):
        cut = MC.cuts(resid, c, W, H)
        E.run_configs(driver, tmp_path, ENTRIES[3], lambda gp: [
            E.exact("gray", planes(g, stride, gp), 3), stride, T, W, H, S, c,
            E.exact("fwd", np.full(F.size * 2, gp, np.uint8), 2, expect=raw(F, np.int16)),
            E.exact("bwd", np.full(Bk.size * 2, gp, np.uint8), 6, expect=raw(Bk, np.int16)),
            E.exact("resid", np.full(8 * T, gp, np.uint8), 8, expect=raw(resid, np.uint64)),
            E.exact("cut", np.full(T, gp, np.uint8), 1, expect=cut), 0])
    assert F.shape == (T, BH, BW, 2) and resid[0] == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S", [1, 32])
@pytest.mark.parametrize("W,H", SHAPES)
def test_compensated_filter(driver, tmp_path, W, H, S, layout):
    T, R = 5, 2
    d, g = clip(T, H, W, W + 11 * H + S, cut_at=None)
    rng = np.random.default_rng(W + S)
    BW, BH = MC.blocks(W, H)
    # any vector within the search radius is a legal field: at S = 32 most chains leave these frames
    F = rng.integers(-S, S + 1, (T, BH, BW, 2)).astype(np.int16)
    Bk = rng.integers(-S, S + 1, (T, BH, BW, 2)).astype(np.int16)
    F[T - 1] = 0
    Bk[0] = 0
    cut = np.zeros(T, np.uint8)
    cut[4] = 1
    dskew, gskew, pad = LAYOUTS[layout]
    stride = W * H + pad + (-(W * H) % 4 if layout == "aligned" else 0)
    for fill in (1, 0):
        want = MC.filter_clip(d, g, R, 12, cut, F, Bk, fill)
        E.run_configs(driver, tmp_path, ENTRIES[4], lambda gp: [
            E.exact("depth", planes(d, stride, gp), dskew), stride, E.exact("gray", planes(g, stride, gp), gskew), stride, T, W, H, 0, T,
            R, 12, fill, E.exact("cut", cut, 1), E.exact("fwd", raw(F, np.int16), 2), E.exact("bwd", raw(Bk, np.int16), 6),
            E.exact("out", np.full(4 * want.size, gp, np.uint8), dskew, expect=raw(want, np.float32)), 0])
    if S == 32:
        m = MC.chain(F, Bk, 2, 4, W, H)
        assert (np.abs(m[..., 0]) >= W).any() or (np.abs(m[..., 1]) >= H).any(), "no chain leaves the frame"
