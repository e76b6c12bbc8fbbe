"""Memory behaviour of v3d_png_deflate_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py holds every
other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four placements
(aligned, minimum alignment -- gray16 frames 2 bytes, BGR frames and `out` 1 byte, `offsets` 8 and `ws` 16 bytes off a 256-byte
boundary --, frame strides padded by 16 bytes and by 7 elements) and over two poison bytes.  The case is entered into that file's
CASES table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py cover this entry too; this
file runs it.

Expected outputs come from tests/png_ref.py: the whole of `out` up to v3d_png_out_bytes (streams, zero gaps, zero tail) and
`offsets`.  Variants: format @ W x H x n."""
import numpy as np
import pytest

import png_ref as PR
import test_abi_guard_gpu as G

ENTRY = "v3d_png_deflate_batch"
# odd widths and a one-pixel image; rows of 1 .. 97 positions per thread; n = 3 so that padodd has frames to pad
VARIANTS = ("g16@253x5x3", "bgr@85x4x3", "g16@1x1x3", "bgr@1x2x1", "g16@8192x2x2", "bgr@2731x3x3")


def case_png_deflate(k, variant):
    kind, dims = variant.split("@")
    W, H, n = (int(v) for v in dims.split("x"))
    fmt = PR.GRAY16 if kind == "g16" else PR.BGR8
    frames = [PR.content_image(fmt, W, H, 10 * W + f) for f in range(n)]
    data = np.stack(frames).reshape(n, H, -1)
    L = k.native.lib()
    img = k.inp("img", data, stride=True)
    out = k.out("out", np.uint8, (L.v3d_png_out_bytes(fmt, n, W, H),))
    off = k.out("offsets", np.uint64, (n + 1,))
    ws = k.ws("ws", L.v3d_png_ws_bytes(fmt, n, W, H), align=G.WS_ALIGN)
    call = lambda lib: lib.v3d_png_deflate_batch(G._p(img), img.frame_stride_bytes, fmt, n, W, H, G._p(out), G._p(off), G._p(ws), G._stream())

    def expect():
        want, offsets, _ = PR.batch(frames, fmt)
        return {"out": want, "offsets": offsets}
    return call, expect, None


G.CASES[ENTRY] = (case_png_deflate, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] == ENTRY]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding, `out`, `offsets` and the workspace: the same bits, i.e. no unwritten byte of
    `out` and no dependence on what the workspace held"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
