"""Memory behaviour of the top-bottom split (v3d_tb_to_gray, v3d_tb_to_gray_batch, v3d_split_tb), held to the header's memory
contract the way tests/test_abi_guard_gpu.py holds the SBS entries: the raw ctypes functions on the buffers of a guard arena
(tests/guard_arena.py), in that file's four placements (aligned, minimum alignment, pitches and strides padded by 16 bytes and by
5 bytes / 7 bytes) and over two poison bytes.  The cases are entered into that file's CASES table, so its run_case, its placements
and the header gate of tests/test_guard_arena_host.py (every entry with a `void* stream` has a guard case) cover these entries too;
this file runs them.  Expected outputs: tests/tb_ref.py.

Variants: 322 x 46 (rows of no multiple of 4 bytes: the byte plan unless the pitch is padded to one, a partial last pixel group),
1076 x 10 (rows of a multiple of 4 bytes, two workgroups across: the dword plan when the base is aligned) and 64 x 8."""
import numpy as np
import pytest

import tb_ref
import test_abi_guard_gpu as G

TO_GRAY, TO_GRAY_BATCH, SPLIT = "v3d_tb_to_gray", "v3d_tb_to_gray_batch", "v3d_split_tb"
VARIANTS = ("unsqueeze@322x46", "plain@322x46", "unsqueeze@1076x10", "plain@1076x10", "unsqueeze@64x8")


def _dims(variant):
    mode, dims = variant.split("@")
    unsq = mode == "unsqueeze"
    W, H = (int(v) for v in dims.split("x"))
    return unsq, W, H, (H if unsq else H // 2)


def case_tb_to_gray(k, variant):
    unsq, W, H, oh = _dims(variant)
    tb = tb_ref.content(1, H, W, W + H)[0]
    s = k.inp("tb", tb.reshape(H, W * 3), pitch=True, odd=5)
    L, R = k.out("left", np.uint8, (oh, W)), k.out("right", np.uint8, (oh, W))
    call = lambda lib: lib.v3d_tb_to_gray(G._p(s), W, H, s.pitch_bytes, int(unsq), G._p(L), G._p(R), G._stream())
    return call, lambda: dict(zip(("left", "right"), tb_ref.to_gray(tb, unsq))), None


def case_split_tb(k, variant):
    unsq, W, H, oh = _dims(variant)
    tb = tb_ref.content(1, H, W, W + H + 1)[0]
    s = k.inp("tb", tb.reshape(H, W * 3), pitch=True, odd=5)
    L, R = k.out("left", np.uint8, (oh, W * 3)), k.out("right", np.uint8, (oh, W * 3))
    call = lambda lib: lib.v3d_split_tb(G._p(s), W, H, s.pitch_bytes, int(unsq), G._p(L), G._p(R), G._stream())
    return call, lambda: {n: a.reshape(oh, -1) for n, a in zip(("left", "right"), tb_ref.split(tb, unsq))}, None


def case_tb_to_gray_batch(k, variant):
    unsq, W, H, oh = _dims(variant)
    n = 3
    tb = tb_ref.content(n, H, W, W + H + 2)
    s = k.inp("tb", tb.reshape(n, H, W * 3), pitch=True, stride=True, odd=5)
    L, R = k.out("left", np.uint8, (n, oh, W)), k.out("right", np.uint8, (n, oh, W))
    call = lambda lib: lib.v3d_tb_to_gray_batch(G._p(s), n, W, H, s.pitch_bytes, s.frame_stride_bytes, int(unsq), G._p(L), G._p(R), G._stream())
    return call, lambda: dict(zip(("left", "right"), tb_ref.to_gray_batch(tb, unsq))), None


G.CASES[TO_GRAY] = (case_tb_to_gray, VARIANTS, True)
G.CASES[TO_GRAY_BATCH] = (case_tb_to_gray_batch, VARIANTS[:3] + VARIANTS[4:], True)
G.CASES[SPLIT] = (case_split_tb, VARIANTS, True)
MINE = (TO_GRAY, TO_GRAY_BATCH, SPLIT)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in MINE]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the pitch and stride padding and the outputs: the same bits, i.e. no unwritten sample and no
    byte outside the payload that reaches the result"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{entry}[{variant}] {place}: {name!r} depends on the poison"
