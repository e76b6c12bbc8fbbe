"""csrc/v3d_png.hip itself (with csrc/v3d_wave.h), without a GPU: the kernel source is compiled as plain C++ against
tests/emu/v3d_common.h, where the 256 threads of a workgroup are fibers and barriers / wave shuffles are rendezvous, and
v3d_png_deflate_batch is called on poisoned host buffers at the alignments the header grants.  `out` and `offsets` must equal tests/png_ref.py byte for byte --
streams, zero gaps, zero tail --, nothing outside `out`, `offsets` and `ws` may change, and every 16-byte load must be aligned.
This checks the kernels' arithmetic and indexing; what only the device can show (LDS atomics, real wave scheduling, speed) is
left to tests/test_png_gpu.py and tests/test_png_guard_gpu.py.
The same cases then run through the stand-alone driver (tests/emu_case.py), plain and under AddressSanitizer and
UndefinedBehaviorSanitizer: heap buffers that end on their payload's last byte, dynamic LDS of exactly the launch's size, both
workgroup and thread orders, two LDS and two global poisons."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import emu_case as E
import png_ref as P
from emu_case import CSRC, EMU
from conftest import ROOT


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one as well)"
    d = tmp_path_factory.mktemp("png_emu")
    assert open(os.path.join(CSRC, "v3d_png.hip")).read().count("extern __shared__") == 1
    src, = E.stage(str(d), ["v3d_png.hip"])
    lib = d / "libpngemu.so"
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-fPIC", "-shared", "-w", "-I", str(d), "-I", EMU, "-I", os.path.join(ROOT, "include"),
                           "-o", str(lib), src, os.path.join(EMU, "harness.cpp")])
    L = C.CDLL(str(lib))
    L.v3d_png_out_bytes.restype = L.v3d_png_ws_bytes.restype = C.c_size_t
    L.v3d_png_deflate_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_int] * 4 + [C.c_void_p] * 4
    return L


def _buf(nbytes, skew, poison):
    """nbytes at 256 k + skew inside a poisoned block -> (block, view)"""
    block = np.full(nbytes + 1024, poison, np.uint8)
    off = (-block.ctypes.data) % 256 + 256 + skew
    return block, block[off:off + nbytes]


# fmt, W, H, n, frame padding (elements), skew of img / out (bytes), poison
CASES = [(P.GRAY16, 1, 1, 3, 7, 2, 1, 0xA5), (P.GRAY16, 127, 5, 3, 7, 2, 1, 0xFF), (P.GRAY16, 129, 2, 2, 0, 0, 0, 0xA5),
         (P.BGR8, 1, 2, 1, 0, 1, 3, 0xFF), (P.BGR8, 85, 4, 3, 7, 1, 1, 0xA5), (P.BGR8, 86, 4, 2, 16, 5, 7, 0xFF),
         (P.GRAY16, 1001, 5, 2, 7, 6, 9, 0xA5), (P.BGR8, 2731, 2, 1, 0, 3, 1, 0xA5), (P.GRAY16, 8192, 2, 1, 0, 2, 1, 0xFF),
         (P.GRAY16, 64, 300, 2, 3, 2, 5, 0xA5)]


@pytest.mark.parametrize("fmt,W,H,n,pad,skew_img,skew_out,poison", CASES,
                         ids=[f"{'g16' if c[0] == 0 else 'bgr'}-{c[1]}x{c[2]}x{c[3]}" for c in CASES])
def test_kernel_source_equals_the_reference(emu, fmt, W, H, n, pad, skew_img, skew_out, poison):
    frames = [P.content_image(fmt, W, H, 3 * W + f) for f in range(n)]
    want, want_off, _ = P.batch(frames, fmt)
    item = 2 if fmt == P.GRAY16 else 1
    per = frames[0].size * item
    stride = per + pad * item
    bi, img = _buf(n * stride, skew_img, poison)
    for f in range(n):
        img[f * stride:f * stride + per] = frames[f].reshape(-1).view(np.uint8)
    nout = emu.v3d_png_out_bytes(fmt, n, W, H)
    assert nout == want.size
    bo, out = _buf(nout, skew_out, poison)
    bw, ws = _buf(emu.v3d_png_ws_bytes(fmt, n, W, H), 16, poison)
    bf, off = _buf(8 * (n + 1), 8, poison)
    before = [b.copy() for b in (bi, bo, bw, bf)]
    loads = emu.emu_misaligned_loads()
    assert emu.v3d_png_deflate_batch(img.ctypes.data, stride, fmt, n, W, H, out.ctypes.data, off.ctypes.data, ws.ctypes.data, None) == 0
    assert emu.emu_misaligned_loads() == loads, "a 16-byte load off its alignment"
    assert np.array_equal(off.view(np.uint64), want_off)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0])}"
    assert np.array_equal(bi, before[0]), "the input was written"
    for block, snap, view in ((bo, before[1], out), (bw, before[2], ws), (bf, before[3], off)):
        lo = view.ctypes.data - block.ctypes.data
        assert np.array_equal(block[:lo], snap[:lo]) and np.array_equal(block[lo + view.size:], snap[lo + view.size:]), "a store outside its buffer"


# ---- the same source in the stand-alone driver, plain and sanitized ----
driver = E.driver_fixture("png", ["v3d_png.hip"], ["v3d_png_deflate_batch", "v3d_png_out_bytes", "v3d_png_ws_bytes"])
# + the second round of k_png_offsets and its carry (more than 256 frames)
DRIVER_CASES = [c[:7] for c in CASES] + [(P.GRAY16, 3, 2, 300, 0, 0, 0)]


@pytest.mark.parametrize("fmt,W,H,n,pad,skew_img,skew_out", DRIVER_CASES,
                         ids=[f"{'g16' if c[0] == 0 else 'bgr'}-{c[1]}x{c[2]}x{c[3]}" for c in DRIVER_CASES])
def test_driver_equals_the_reference(driver, tmp_path, fmt, W, H, n, pad, skew_img, skew_out):
    frames = [P.content_image(fmt, W, H, 3 * W + f) for f in range(n)]
    want, want_off, _ = P.batch(frames, fmt)
    item = 2 if fmt == P.GRAY16 else 1
    per = frames[0].size * item
    stride = per + pad * item
    nout = E.query(driver, "v3d_png_out_bytes", fmt, n, W, H)
    assert nout == want.size
    nws = E.query(driver, "v3d_png_ws_bytes", fmt, n, W, H)

    def make(gp):
        # the last frame's payload ends on the allocation's last byte: the padding belongs to the stride, not to the buffer
        img = np.full((n - 1) * stride + per, gp, np.uint8)
        for f in range(n):
            img[f * stride:f * stride + per] = frames[f].reshape(-1).view(np.uint8)
        return [E.exact("img", img, skew_img), stride, fmt, n, W, H,
                E.exact("out", np.full(nout, gp, np.uint8), skew_out, expect=want),
                E.exact("offsets", np.full(8 * (n + 1), gp, np.uint8), 8, expect=want_off.astype(np.uint64).view(np.uint8)),
                E.exact("ws", np.full(nws, gp, np.uint8), 16, expect=None), 0]
    E.run_configs(driver, tmp_path, "v3d_png_deflate_batch", make)
