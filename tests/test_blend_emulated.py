"""csrc/v3d_blend.hip itself, without a GPU: v3d_mono_blend and v3d_mono_blend_batch run in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal oracle.mono_blend bit for bit:
enlarging, shrinking, the identity, ratios that are no whole numbers, one-row and one-pixel maps, and a batch with a padded
mono_stride, per-frame ranges and one flat frame (no mono term).  Every buffer ends on its heap block's last byte, so a bilinear tap
one column or one row past the map is a sanitizer report; the workspace is exactly v3d_mono_blend_ws_bytes(n)."""
import numpy as np
import pytest

import emu_case as E

ENTRIES = ["v3d_mono_blend", "v3d_mono_blend_batch", "v3d_mono_blend_ws_bytes"]
driver = E.driver_fixture("blend", ["v3d_blend.hip"], ENTRIES)
CASES = [(192, 108, 384, 384), (192, 108, 48, 48), (64, 64, 64, 64), (203, 77, 97, 333), (70, 1, 5, 3), (257, 33, 1, 1), (64, 64, 128, 128), (300, 9, 7, 2)]


def _bits(w):
    return int(np.float32(w).view(np.uint32))


def _raw(a, dtype):
    return np.ascontiguousarray(a, dtype).reshape(-1).view(np.uint8)


def _inputs(W, H, mw, mh, seed, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    d16 = rng.integers(0, 1009, (H, W)).astype(np.int16)
    d16[rng.random((H, W)) < 0.2] = -16
    return d16, (rng.random((mh, mw)) * (hi - lo) + lo).astype(np.float32)


@pytest.mark.parametrize("W,H,mw,mh", CASES)
def test_mono_blend(driver, tmp_path, oracle, W, H, mw, mh):
    d16, mono = _inputs(W, H, mw, mh, W + mw)
    weights = (0.25, 0.75) if (W, H, mw, mh) == CASES[3] else (0.7, 0.3)
    want = oracle.mono_blend(d16, mono, *weights)
    assert mw * mh == 1 or (want > 0).mean() > 0.5
    nws = E.query(driver, ENTRIES[2], 1)
    assert nws == 8
    E.run_configs(driver, tmp_path, ENTRIES[0], lambda gp: [
        E.exact("disp", _raw(d16, np.int16), 2), W, H, E.exact("mono", _raw(mono, np.float32), 4), mw, mh, _bits(weights[0]), _bits(weights[1]),
        E.exact("out", np.full(4 * W * H, gp, np.uint8), 4, expect=_raw(want, np.float32)), E.exact("ws", np.full(nws, gp, np.uint8), 16, expect=None), 0])


@pytest.mark.parametrize("W,H,mw,mh,pad", [(70, 5, 7, 3, 5), (64, 8, 64, 8, 3), (203, 9, 97, 33, 0)])
def test_a_batch_with_a_padded_stride_per_frame_ranges_and_a_flat_frame(driver, tmp_path, oracle, W, H, mw, mh, pad):
    n, stride = 3, mw * mh + pad
    ins = [_inputs(W, H, mw, mh, 1, 0.0, 1.0), _inputs(W, H, mw, mh, 2, -50.0, 300.0), _inputs(W, H, mw, mh, 3)]
    ins[2] = (ins[2][0], np.zeros((mh, mw), np.float32))             # flat after the resize too: 0 a + 0 b is exact, 3 a + 3 b is not
    want = np.stack([oracle.mono_blend(d, m) for d, m in ins])
    assert np.array_equal(want[2], oracle.disp_to_depth(ins[2][0])) and not np.array_equal(want[0], oracle.mono_blend(ins[0][0], ins[1][1]))
    nws = E.query(driver, ENTRIES[2], n)
    assert nws == 8 * n

    def make(gp):
        mono = np.full(((n - 1) * stride + mw * mh) * 4, gp, np.uint8)
        for f in range(n):
            mono[4 * f * stride:4 * (f * stride + mw * mh)] = _raw(ins[f][1], np.float32)
        return [E.exact("disp", _raw(np.stack([d for d, _ in ins]), np.int16), 2), n, W, H, E.exact("mono", mono, 4), mw, mh, stride, _bits(0.7), _bits(0.3),
                E.exact("out", np.full(4 * n * W * H, gp, np.uint8), 4, expect=_raw(want, np.float32)), E.exact("ws", np.full(nws, gp, np.uint8), 0, expect=None), 0]
    E.run_configs(driver, tmp_path, ENTRIES[1], make)
