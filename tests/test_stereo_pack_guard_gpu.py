"""Memory behaviour of v3d_render_stereo_packed_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py
holds every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four
placements (aligned, minimum alignment, strides padded by 16 bytes and by 7 elements) and over two poison bytes.  The case is entered
into that file's CASES table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py (every entry
with a `void* stream` has a guard case) cover this entry too; this file runs it.

Variants: packing[-sub] @ W x H, n = 3: every new packing at one small size, both renderers (a run that ends inside a thread,
a half top-bottom pair in a ragged band, more than one thread run, a row shorter than one run, a band of one left-eye row)."""
import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_sub_ref as S
import test_abi_guard_gpu as G

ENTRY = "v3d_render_stereo_packed_batch"
CODES = {"tb": P.FULL_TB, "htb": P.HALF_TB, "rows": P.ROWS, "ana": P.ANAGLYPH_COLOUR, "dub": P.ANAGLYPH_DUBOIS}
VARIANTS = ("tb@255x5", "htb@254x6", "rows@1000x5", "ana@7x3", "dub@255x5", "tb-sub@7x3", "htb-sub@1000x6", "rows-sub@255x5",
            "ana-sub@254x6", "dub-sub@1000x4")


def case_render_stereo_packed(k, variant):
    mode, dims = variant.split("@")
    packing, sub = CODES[mode.split("-")[0]], int(mode.endswith("-sub"))
    W, H = (int(v) for v in dims.split("x"))
    n = 3
    rng = np.random.default_rng(W + packing)
    frames = rng.integers(0, 256, (n, H, W * 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(kind, H, W, W + i) for i, kind in enumerate(("planar", "steep", "noise"))])
    gl, gr, conv = S.stereo_gains(24.0, 0.5, 0.5)
    f, d = k.inp("frame_bgr", frames, stride=True), k.inp("depth", depth, stride=True)
    ow, oh = P.output_size(packing, W, H)
    o = k.out("out_bgr", np.uint8, (n, oh, ow * 3))
    call = lambda lib: lib.v3d_render_stereo_packed_batch(G._p(f), f.frame_stride_bytes, G._p(d), d.frame_stride, n, W, H, gl, gr,
                                                          conv, sub, packing, G._p(o), G._stream())
    return call, lambda: {"out_bgr": np.stack([P.render(frames[i].reshape(H, W, 3), depth[i], gl, gr, conv, packing,
                                                        bool(sub)).reshape(oh, -1) for i in range(n)])}, None


G.CASES[ENTRY] = (case_render_stereo_packed, VARIANTS, True)


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
