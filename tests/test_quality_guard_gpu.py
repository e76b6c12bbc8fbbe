"""Memory behaviour of v3d_quality_reproj_batch and v3d_quality_flicker_batch, held to the header's memory contract the way
tests/test_abi_guard_gpu.py holds every other entry: the raw ctypes functions on the buffers of a guard arena
(tests/guard_arena.py), in that file's four placements and over two poison bytes.  Both cases are entered into that file's CASES
table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py cover them; this file runs them.

Variants W x H @ n (frames of the batch / of the clip): an odd width whose last group is partial, 320 x 180, whose dense rows take
the vector loads in the aligned placements and the byte loads in the skewed and odd ones, one column, and a wide plane with more
than one row band.  The workspaces are poisoned, the padding between rows and frames too: nothing of either may reach a record."""
import numpy as np
import pytest

import quality_ref as QR
import test_abi_guard_gpu as G

REPROJ, FLICKER = "v3d_quality_reproj_batch", "v3d_quality_flicker_batch"
VARIANTS = ("253x77x3", "320x180x3", "1x5x2", "4112x9x2")


def _dims(variant):
    return (int(v) for v in variant.split("x"))


def case_reproj(k, variant):
    W, H, n = _dims(variant)
    rng = np.random.default_rng(W + H)
    L, R = rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    d = rng.integers(-20, min(16 * W + 20, 32768), (n, H, W)).astype(np.int16)
    d[0, 0, 0] = 32767
    l, r = k.inp("left", L, pitch=True, stride=True), k.inp("right", R, pitch=True, stride=True)
    dd = k.inp("disp16", d, stride=True)
    ws = k.ws("ws", k.native.lib().v3d_quality_reproj_ws_bytes(n, W, H), align=16)
    o = k.out("records", np.uint64, (n, 8), align=8)
    call = lambda lib: lib.v3d_quality_reproj_batch(G._p(l), G._p(r), n, W, H, l.pitch_bytes, l.frame_stride_bytes, G._p(dd), dd.frame_stride,
                                                    16, G._p(o), G._p(ws), G._stream())
    return call, lambda: {"records": QR.reproj(L, R, d, 16).astype(np.uint64)}, None


def case_flicker(k, variant):
    W, H, T = _dims(variant)
    rng = np.random.default_rng(W + H + 1)
    depth = (np.clip(rng.integers(1, 1024, (1, H, W)) + rng.integers(-30, 31, (T, H, W)), -16, 32767) / 16).astype(np.float32)
    depth[rng.random((T, H, W)) < 0.1] = np.nan
    gray = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-5, 6, (T, H, W)), 0, 255).astype(np.uint8)
    dd, g = k.inp("depth", depth, stride=True), k.inp("gray", gray, stride=True)
    ws = k.ws("ws", k.native.lib().v3d_quality_flicker_ws_bytes(T, W, H), align=16)
    o = k.out("records", np.uint64, (T - 1, 4), align=8)
    call = lambda lib: lib.v3d_quality_flicker_batch(G._p(dd), dd.frame_stride, G._p(g), g.frame_stride_bytes, T, W, H, 4, 16, G._p(o), G._p(ws),
                                                     G._stream())
    return call, lambda: {"records": QR.flicker(depth, gray, 4, 16).astype(np.uint64)}, None


G.CASES[REPROJ] = (case_reproj, VARIANTS, True)
G.CASES[FLICKER] = (case_flicker, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in (REPROJ, FLICKER)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding, the workspaces and the outputs: the same bits, i.e. no unwritten field, no
    dependence on what the workspace held and no byte past a row's payload that reaches a sum"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
