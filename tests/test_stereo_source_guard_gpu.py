"""Memory behaviour of v3d_render_stereo_source_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py
holds every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four
placements and over two poison bytes.  The case is entered into that file's CASES table, so its run_case, its placements and the
header gate of tests/test_guard_arena_host.py (every entry with a `void* stream` has a guard case) cover this entry too; this file
runs it.  The SBS frames have pitched rows and padded frames in the padded placements: only their payload may reach the result.

Variants: renderer @ W x H [packing], n = 3, fill_eyes = 3: the integer and the sub-pixel render at a run that ends inside a thread
and at more than one thread run, and one packed layout."""
import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_source_ref as X
import stereo_sub_ref as S
import test_abi_guard_gpu as G

ENTRY = "v3d_render_stereo_source_batch"
VARIANTS = ("int@255x5", "sub@255x5", "int@1000x4", "sub@1000x4", "int@254x6-htb")
MAP = (21845, -9000, 30000, 77)


def case_render_stereo_source(k, variant):
    mode, dims = variant.split("@")
    dims, _, pack = dims.partition("-")
    packing, sub = (P.HALF_TB if pack == "htb" else P.FULL_SBS), int(mode == "sub")
    W, H = (int(v) for v in dims.split("x"))
    n, Ws, Hs, fill = 3, 10, 4, 3
    rng = np.random.default_rng(W + sub)
    frames = rng.integers(0, 256, (n, H, W * 3), dtype=np.uint8)
    sbs = rng.integers(0, 256, (n, Hs, Ws * 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(kind, H, W, W + i) for i, kind in enumerate(("planar", "steep", "noise"))])
    gl, gr, conv = S.stereo_gains(24.0, 0.5, 0.5)
    f, d = k.inp("frame_bgr", frames, stride=True), k.inp("depth", depth, stride=True)
    s = k.inp("sbs_bgr", sbs, pitch=True, stride=True, odd=5)
    ow, oh = P.output_size(packing, W, H)
    o = k.out("out_bgr", np.uint8, (n, oh, ow * 3))
    call = lambda lib: lib.v3d_render_stereo_source_batch(G._p(f), f.frame_stride_bytes, G._p(d), d.frame_stride, n, W, H, gl, gr,
                                                          conv, sub, packing, G._p(s), s.frame_stride_bytes, Ws, Hs, s.pitch_bytes,
                                                          fill, *MAP, G._p(o), G._stream())
    return call, lambda: {"out_bgr": np.stack([X.render(frames[i].reshape(H, W, 3), depth[i], gl, gr, conv, packing, bool(sub),
                                                        sbs[i].reshape(Hs, Ws, 3), fill, *MAP).reshape(oh, -1) for i in range(n)])}, None


G.CASES[ENTRY] = (case_render_stereo_source, VARIANTS, True)


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
