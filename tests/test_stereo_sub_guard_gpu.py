"""Memory behaviour of v3d_render_stereo_subpixel_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py
holds every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four
placements (aligned, minimum alignment, strides padded by 16 bytes and by 7 elements) and over two poison bytes.  The case is entered
into that file's CASES table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py (every entry
with a `void* stream` has a guard case) cover this entry too; this file runs it.

Variants: layout @ W x H, n = 3: the integer entry's sizes (a run that ends inside a thread, a half-SBS pair at the row's end, more
than one thread run, a row shorter than one run)."""
import numpy as np
import pytest

import stereo_sub_ref as S
import test_abi_guard_gpu as G

ENTRY = "v3d_render_stereo_subpixel_batch"
VARIANTS = ("full@255x5", "half@254x5", "full@1000x4", "full@7x3")


def case_render_stereo_subpixel(k, variant):
    mode, dims = variant.split("@")
    layout = S.FULL_SBS if mode == "full" else S.HALF_SBS
    W, H = (int(v) for v in dims.split("x"))
    n = 3
    rng = np.random.default_rng(W + layout)
    frames = rng.integers(0, 256, (n, H, W * 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(kind, H, W, W + i) for i, kind in enumerate(("planar", "steep", "noise"))])
    gl, gr, conv = S.stereo_gains(24.0, 0.5, 0.5)
    f, d = k.inp("frame_bgr", frames, stride=True), k.inp("depth", depth, stride=True)
    ow = 2 * W if layout == S.FULL_SBS else W
    o = k.out("out_bgr", np.uint8, (n, H, ow * 3))
    call = lambda lib: lib.v3d_render_stereo_subpixel_batch(G._p(f), f.frame_stride_bytes, G._p(d), d.frame_stride, n, W, H, gl, gr,
                                                            conv, layout, G._p(o), G._stream())
    return call, lambda: {"out_bgr": np.stack([S.render(frames[i].reshape(H, W, 3), depth[i], gl, gr, conv, layout).reshape(H, -1)
                                               for i in range(n)])}, None


G.CASES[ENTRY] = (case_render_stereo_subpixel, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] == ENTRY]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding and the output: the same bits, i.e. no unwritten byte and no read past an input
    that reaches the result"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
