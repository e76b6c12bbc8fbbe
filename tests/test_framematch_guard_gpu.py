"""Memory behaviour of v3d_frame_signature_batch and v3d_signature_scores, held to the header's memory contract the way
tests/test_abi_guard_gpu.py holds every other entry: the raw ctypes functions on the buffers of a guard arena
(tests/guard_arena.py), in that file's four placements and over two poison bytes.  Both cases are entered into that file's CASES
table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py cover them; this file runs them.

Signature variants W x H @ n: 16-byte groups that end inside the row (253, 322), the smallest plane, a wide one with two groups
per lane row, and 320 x 180, whose dense rows take the vector loads in the aligned placements and the byte loads in the skewed
and odd ones."""
import numpy as np
import pytest

import framematch_ref as FR
import test_abi_guard_gpu as G

SIG, SCORES = "v3d_frame_signature_batch", "v3d_signature_scores"
SIG_VARIANTS = ("253x77x3", "320x180x3", "64x36x3", "4112x40x2", "322x182x1")
SCORE_VARIANTS = ("5x9", "1x1")


def _planes(n, H, W, seed):
    g = np.random.default_rng(seed).integers(0, 256, (n, H, W), dtype=np.uint8)
    g[-1, :, W // 2:] = 255                                   # saturated cells
    return g


def case_signature(k, variant):
    W, H, n = (int(v) for v in variant.split("x"))
    data = _planes(n, H, W, W + H)
    g = k.inp("gray", data, pitch=True, stride=True)
    o = k.out("sig", np.uint16, (n, FR.G))
    call = lambda lib: lib.v3d_frame_signature_batch(G._p(g), n, W, H, g.pitch_bytes, g.frame_stride_bytes, G._p(o), G._stream())
    return call, lambda: {"sig": FR.signature(data)}, None


def _signatures(n, seed):
    s = np.random.default_rng(seed).integers(0, 65281, (n, FR.G)).astype(np.uint16)
    s[0] = 65280                                              # zero variance
    if n > 1:
        s[1] = np.where(np.arange(FR.G) % 2 == 0, 0, 65280)   # the largest variance
    return s


def case_scores(k, variant):
    na, nb = (int(v) for v in variant.split("x"))
    a, b = _signatures(na, 1), _signatures(nb, 2)
    A, B = k.inp("sig_a", a), k.inp("sig_b", b)
    num, va, vb = k.out("num", np.int64, (na, nb)), k.out("var_a", np.int64, (na,)), k.out("var_b", np.int64, (nb,))
    call = lambda lib: lib.v3d_signature_scores(G._p(A), na, G._p(B), nb, G._p(num), G._p(va), G._p(vb), G._stream())
    return call, lambda: dict(zip(("num", "var_a", "var_b"), FR.scores(a, b))), None


G.CASES[SIG] = (case_signature, SIG_VARIANTS, True)
G.CASES[SCORES] = (case_scores, SCORE_VARIANTS, False)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in (SIG, SCORES)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding and the outputs: the same bits, i.e. no unwritten cell and no byte read past a
    row's payload that reaches a sum"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
