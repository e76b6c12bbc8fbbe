"""csrc/v3d_quality.hip itself (both entries), without a GPU: the kernel source runs in the stand-alone emulator driver
(tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/quality_ref.py bit for
bit.  The sizes, disparities and depths of tests/test_quality_gpu.py up to 1037 x 9 and 4112 x 4; every plane ends on its heap
block's last byte (only the payload of a row may be read), once aligned with 16-byte pitches and strides (the vector route where
W is a multiple of 8) and once at odd bases with padded pitches and strides (the byte route)."""
import numpy as np
import pytest

import emu_case as E
import quality_ref as QR
from test_quality_gpu import SIZES, _depths, _disparities, _grays

ENTRIES = ["v3d_quality_reproj_batch", "v3d_quality_flicker_batch", "v3d_quality_reproj_ws_bytes", "v3d_quality_flicker_ws_bytes"]
driver = E.driver_fixture("quality", ["v3d_quality.hip"], ENTRIES)
SIZES = [s for s in SIZES if s[0] <= 4112]
IDS = [f"{w}x{h}x{n}" for w, h, n in SIZES]


def _planes(a, pitch, stride, item, gp):
    """a [n,H,W] of `item`-byte elements -> bytes with rows `pitch` and frames `stride` ELEMENTS apart, ending on the last payload byte"""
    n, H, W = a.shape
    img = np.full(((n - 1) * stride + (H - 1) * pitch + W) * item, gp, np.uint8)
    rows = np.ascontiguousarray(a).view(np.uint8).reshape(n, H, W * item)
    for f in range(n):
        for y in range(H):
            o = (f * stride + y * pitch) * item
            img[o:o + W * item] = rows[f, y]
    return img


def _u64(v):
    return np.ascontiguousarray(v, np.int64).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("W,H,n", SIZES, ids=IDS)
def test_reproj(driver, tmp_path, W, H, n, layout):
    L, R = _grays(n, H, W, 3 * W + H)
    if layout == "aligned":
        pitch, sk = (W + 15) // 16 * 16, (0, 0, 0)
        fstride, dstride = H * pitch + 16, H * W + 8
    else:
        pitch, sk = W + 5, (1, 3, 2)
        fstride, dstride = H * pitch + 11, H * W + 7
    nws = E.query(driver, "v3d_quality_reproj_ws_bytes", n, W, H)
    big = n * H * W > 20000
    for name, d in _disparities(n, H, W, W + 5 * H).items():
        if big and name in ("invalid", "d16"):
            continue
        for thr in ((16,) if name != "random" or big else (0, 16, 255)):
            want = QR.reproj(L, R, d, thr)

            def make(gp):
                return [E.exact("left", _planes(L, pitch, fstride, 1, gp), sk[0]), E.exact("right", _planes(R, pitch, fstride, 1, gp), sk[1]),
                        n, W, H, pitch, fstride, E.exact("disp", _planes(d, W, dstride, 2, gp), sk[2]), dstride, thr,
                        E.exact("out", np.full(want.size * 8, gp, np.uint8), 8, expect=_u64(want)),
                        E.exact("ws", np.full(nws, gp, np.uint8), 16, expect=None), 0]
            E.run_configs(driver, tmp_path, ENTRIES[0], make)


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("W,H,k", [(w, h, k) for k, (w, h, _) in enumerate(SIZES)], ids=IDS)
def test_flicker(driver, tmp_path, W, H, k, layout):
    T = 2 + k % 4
    depth, gray = _depths(T, H, W, 11 * W + H)
    dstride, gstride, sk = (H * W + 4, H * W + 8, (0, 0)) if layout == "aligned" else (H * W + 3, H * W + 5, (4, 3))
    nws = E.query(driver, "v3d_quality_flicker_ws_bytes", T, W, H)
    for still, jump in ((4, 16), (0, 0), (255, 32767)) if T * H * W <= 20000 else ((4, 16),):
        want = QR.flicker(depth, gray, still, jump)

        def make(gp):
            return [E.exact("depth", _planes(depth, W, dstride, 4, gp), sk[0]), dstride, E.exact("gray", _planes(gray, W, gstride, 1, gp), sk[1]),
                    gstride, T, W, H, still, jump, E.exact("out", np.full(want.size * 8, gp, np.uint8), 24, expect=_u64(want)),
                    E.exact("ws", np.full(nws, gp, np.uint8), 16, expect=None), 0]
        E.run_configs(driver, tmp_path, ENTRIES[1], make)
