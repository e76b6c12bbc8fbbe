"""csrc/v3d_framematch.hip itself, without a GPU: the kernel source runs in the stand-alone emulator driver (tests/emu_case.py),
plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/framematch_ref.py bit for bit.  The signature
entry promises that only the W payload bytes of a row are read (v3d_wave.h's row_load16), so the plane ends on its heap block's
last byte: the last row has no pitch padding behind it.  Dense, 16-byte and odd pitches, an aligned and an odd base."""
import numpy as np
import pytest

import emu_case as E
import framematch_ref as FR

driver = E.driver_fixture("framematch", ["v3d_framematch.hip"], ["v3d_frame_signature_batch", "v3d_signature_scores"])


def _frames(n, H, W, seed):
    """random frames, then one all-255 and one all-0 frame"""
    g = np.random.default_rng(seed).integers(0, 256, (n + 2, H, W), dtype=np.uint8)
    g[n], g[n + 1] = 255, 0
    return g


# 64x36: one pixel per cell; 65x37: cells of 1 and 2; 322x182: partial last group; 8190x36: the widest cells.  Layouts: dense
# (the vector route where W is a multiple of 16), a pitch of whole 16-byte groups (the vector route with a partial last group),
# pitch + 7 from base + 1 (the byte route)
@pytest.mark.parametrize("layout", ["dense", "pitch16", "pitch7-base1"])
@pytest.mark.parametrize("W,H", [(64, 36), (65, 37), (322, 182), (8190, 36)])
def test_signature(driver, tmp_path, W, H, layout):
    g = _frames(1, H, W, W * 7 + H)
    n = g.shape[0]
    want = FR.signature(g).astype(np.uint16)
    pitch, base = {"dense": (W, 0), "pitch16": ((W + 15) // 16 * 16 + 16, 0), "pitch7-base1": (W + 7, 1)}[layout]
    stride = H * pitch + (32 if layout == "pitch16" else 11 if layout == "pitch7-base1" else 0)

    def make(gp):
        img = np.full((n - 1) * stride + (H - 1) * pitch + W, gp, np.uint8)
        for f in range(n):
            for y in range(H):
                img[f * stride + y * pitch:f * stride + y * pitch + W] = g[f, y]
        out = E.exact("sig", np.full(2 * want.size, gp, np.uint8), 2, expect=want.reshape(-1).view(np.uint8))
        return [E.exact("gray", img, base), n, W, H, pitch, stride, out, 0]
    E.run_configs(driver, tmp_path, "v3d_frame_signature_batch", make)
    assert (want[n - 2] == 65280).all() and (want[n - 1] == 0).all()


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 9)])
def test_scores(driver, tmp_path, na, nb):
    rng = np.random.default_rng(na * 16 + nb)
    a = rng.integers(0, 65281, (na, FR.G)).astype(np.uint16)
    b = rng.integers(0, 65281, (nb, FR.G)).astype(np.uint16)
    a[0] = 65280                                                     # zero variance, the largest sums
    b[-1] = np.where(np.arange(FR.G) % 2 == 0, 0, 65280)             # the largest terms
    num, va, vb = FR.scores(a, b)
    i64 = lambda v: np.ascontiguousarray(v, np.int64).reshape(-1).view(np.uint8)

    def make(gp):
        out = lambda name, v, skew: E.exact(name, np.full(8 * np.size(v), gp, np.uint8), skew, expect=i64(v))
        return [E.exact("a", a.view(np.uint8), 2), na, E.exact("b", b.view(np.uint8), 6), nb,
                out("num", num, 8), out("va", va, 24), out("vb", vb, 0), 0]
    E.run_configs(driver, tmp_path, "v3d_signature_scores", make)
