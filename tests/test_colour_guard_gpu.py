"""Memory behaviour of the three colour-matching entries (csrc/v3d_colour.hip), held to the header's memory contract the way
tests/test_abi_guard_gpu.py holds every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py),
in that file's four placements and over two poison bytes.  The cases are entered into that file's CASES table, so its run_case, its
placements and the header gate of tests/test_guard_arena_host.py (every entry with a `void* stream` has a guard case) cover these
entries too; this file runs them.

Variants: histogram and apply as WxH-rectangle at n = 3: the whole image, an inner rectangle whose rows start and end inside a
16-byte block, one pixel column.  The apply entry runs in place (`ip`: the image is an inout buffer whose expected content is the
whole image, so the bytes outside the rectangle are compared too) and out of place (`op`: the destination starts as a copy of the
source for the same reason; `aligned`, `minalign` and `pad16` put both images at the same byte of a 16-byte block, the aligned-load
route, `padodd` pads their rows by 5 and by 3 bytes, the byte-load route), with one table (`one`) and one per frame (`per`).  The
table entry has no pitch or stride."""
import numpy as np
import pytest

import colour_ref as CR
import test_abi_guard_gpu as G

HIST, LUT, APPLY = "v3d_bgr_hist_batch", "v3d_colour_lut_batch", "v3d_bgr_lut_batch"
RECTS = {"whole": None, "inner": (3, 1, 95, 8), "column": (50, 0, 51, 9)}
W, H, N = 101, 9, 3


def _frames(seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


def case_bgr_hist(k, variant):
    F, rect = _frames(1), RECTS[variant]
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    b = k.inp("bgr", F.reshape(N, H, W * 3), pitch=True, stride=True, odd=5)
    o = k.out("hist", np.uint32, (N, 3 * 256))
    call = lambda lib: lib.v3d_bgr_hist_batch(G._p(b), b.frame_stride_bytes, N, W, H, b.pitch_bytes, x0, y0, x1, y1, G._p(o), G._stream())
    return call, lambda: {"hist": CR.hist(F, rect).reshape(N, -1)}, None


def case_colour_lut(k, variant):
    group = int(variant[1:])
    rng = np.random.default_rng(2)
    s, d = rng.integers(0, 5000, (5, 3, 256)).astype(np.uint32), rng.integers(0, 70, (5, 3, 256)).astype(np.uint32)
    a, b = k.inp("hist_src", s.reshape(5, -1)), k.inp("hist_dst", d.reshape(5, -1))
    tables = -(-5 // group)
    o = k.out("lut", np.uint8, (tables, 3 * 256))
    call = lambda lib: lib.v3d_colour_lut_batch(G._p(a), G._p(b), 5, group, G._p(o), G._stream())
    return call, lambda: {"lut": CR.lut(s, d, group).reshape(tables, -1)}, None


def case_bgr_lut(k, variant):
    mode, tables, name = variant.split("-")
    F, rect = _frames(3), RECTS[name]
    x0, y0, x1, y1 = rect or (0, 0, W, H)
    T = np.random.default_rng(4).integers(0, 256, (N if tables == "per" else 1, 3, 256), dtype=np.uint8)
    t = k.inp("lut", T.reshape(T.shape[0], -1), stride=False)
    ls = 768 if tables == "per" else 0
    want = CR.apply(F, T, rect).reshape(N, H, W * 3)
    if mode == "ip":
        io = k.inp("img", F.reshape(N, H, W * 3), pitch=True, stride=True, odd=5, role="inout")
        k.outs["img"] = io
        call = lambda lib: lib.v3d_bgr_lut_batch(G._p(io), io.frame_stride_bytes, N, W, H, io.pitch_bytes, x0, y0, x1, y1, G._p(t), ls,
                                                 G._p(io), io.frame_stride_bytes, io.pitch_bytes, G._stream())
        return call, lambda: {"img": want}, None
    s = k.inp("src", F.reshape(N, H, W * 3), pitch=True, stride=True, odd=5)
    # the destination: the source's bytes already in place, so that the bytes outside the rectangle, which the entry must not
    # write, are part of the expected image
    d = k.inp("dst", F.reshape(N, H, W * 3), pitch=True, stride=True, odd=3, role="inout")
    k.outs["dst"] = d
    call = lambda lib: lib.v3d_bgr_lut_batch(G._p(s), s.frame_stride_bytes, N, W, H, s.pitch_bytes, x0, y0, x1, y1, G._p(t), ls,
                                             G._p(d), d.frame_stride_bytes, d.pitch_bytes, G._stream())
    return call, lambda: {"dst": want}, None


G.CASES[HIST] = (case_bgr_hist, tuple(RECTS), True)
G.CASES[LUT] = (case_colour_lut, ("g1", "g2", "g5"), False)
G.CASES[APPLY] = (case_bgr_lut, ("ip-one-whole", "ip-per-inner", "ip-one-column", "op-per-whole", "op-one-inner", "op-per-column"), True)
ENTRIES = (HIST, LUT, APPLY)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in ENTRIES]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding and the outputs: the same bits, i.e. no unwritten byte and no read past an input
    that reaches the result"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
