"""Memory behaviour of v3d_fill_holes_disp16_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py holds
every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four placements
(aligned, minimum alignment, strides padded by 16 bytes and by 7 elements) and over two poison bytes.  The case is entered into
that file's CASES table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py (every entry with
a `void* stream` has a guard case) cover this entry too; this file runs it.

Variants: W x H @ n, out of place (the input under guard as well) and in place (one inout buffer, dense as the entry demands)."""
import numpy as np
import pytest

import fill_ref as FR
import test_abi_guard_gpu as G

ENTRY = "v3d_fill_holes_disp16_batch"
# 8 / 16 / 40 pixels per thread; odd widths; more rows than one band of either pass; n = 3 so that padodd has frames to pad
VARIANTS = ("out@253x37x3", "inplace@253x37x3", "out@2050x5x3", "inplace@64x3x1", "out@8190x2x2", "out@1x9x3")


def _frames(n, H, W, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 1024, (n, H, W)).astype(np.int16)
    d[rng.random((n, H, W)) < 0.4] = -16
    d[:, :, :min(64, W - 1)] = -16
    d[:, H // 3] = -1                                         # an empty row in every frame
    d[:, -1] = -32768                                         # and the last one
    if n > 1:
        d[1] = -16                                            # one frame entirely invalid: copied through
    return d


def case_fill_holes(k, variant):
    mode, dims = variant.split("@")
    W, H, n = (int(v) for v in dims.split("x"))
    data = _frames(n, H, W, W + H)
    ws = k.ws("ws", k.native.lib().v3d_fill_holes_ws_bytes(n, H), align=G.WS_ALIGN)
    if mode == "inplace":
        d = k.inout("disp", data)
        call = lambda lib: lib.v3d_fill_holes_disp16_batch(G._p(d), H * W, n, W, H, G._p(d), G._p(ws), G._stream())
        return call, lambda: {"disp": FR.fill(data)}, None
    d = k.inp("disp", data, stride=True)
    o = k.out("filled", np.int16, (n, H, W))
    call = lambda lib: lib.v3d_fill_holes_disp16_batch(G._p(d), d.frame_stride, n, W, H, G._p(o), G._p(ws), G._stream())
    return call, lambda: {"filled": FR.fill(data)}, None


G.CASES[ENTRY] = (case_fill_holes, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] == ENTRY]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding, the output and the row flags: the same bits, i.e. no unwritten sample and no
    dependence on what the workspace or the output held"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
