"""Memory behaviour of v3d_plane_profiles_batch, v3d_profile_match_scores and v3d_warp_u16_batch, held to the header's memory
contract the way tests/test_abi_guard_gpu.py holds every other entry: the raw ctypes functions on the buffers of a guard arena
(tests/guard_arena.py), in that file's four placements and over two poison bytes.  The cases are entered into that file's CASES
table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py cover them; this file runs them.

Profile variants W x H @ n: 16-byte groups that end inside the row (253, 322), the smallest plane, one of several segments per
row, and 320 x 180, whose dense rows take the vector loads in the aligned placements and the byte loads in the skewed and odd
ones.  Match variants na x nb @ bins.  Warp variants Ws x Hs -> Wo x Ho: odd widths put every other output row off the 8-byte
boundary its stores are grouped by."""
import numpy as np
import pytest

import register_ref as RR
import test_abi_guard_gpu as G

PROFILES, MATCH, WARP = "v3d_plane_profiles_batch", "v3d_profile_match_scores", "v3d_warp_u16_batch"
PROFILE_VARIANTS = ("253x77x3", "320x180x3", "1x1x3", "2050x9x2", "322x182x1")
MATCH_VARIANTS = ("23x31@8", "256x512@512")
WARP_VARIANTS = ("17x5-9x4", "130x70-131x69", "64x36-64x36")


def case_profiles(k, variant):
    W, H, n = (int(v) for v in variant.split("x"))
    data = np.random.default_rng(W + H).integers(0, 256, (n, H, W), dtype=np.uint8)
    data[-1, :, W // 2:] = 255
    g = k.inp("gray", data, pitch=True, stride=True)
    col, row = k.out("col", np.uint32, (n, W)), k.out("row", np.uint32, (n, H))
    L = k.native.lib()
    ws = k.ws("ws", L.v3d_plane_profiles_ws_bytes(n, W, H), align=G.WS_ALIGN)
    call = lambda lib: lib.v3d_plane_profiles_batch(G._p(g), n, W, H, g.pitch_bytes, g.frame_stride_bytes, G._p(col), G._p(row), G._p(ws), G._stream())
    return call, lambda: dict(zip(("col", "row"), RR.profiles(data))), None


def case_match(k, variant):
    dims, bins = variant.split("@")
    (na, nb), bins, K = (int(v) for v in dims.split("x")), int(bins), 2
    rng = np.random.default_rng(na)
    a, b = rng.integers(0, 1 << 21, (K, na)).astype(np.uint32), rng.integers(0, 1 << 21, (K, nb)).astype(np.uint32)
    nom = na * RR.Q // nb
    cand = np.array([(nom, 0), (nom, 4321), (nom * 7 // 8, na * RR.Q // 16), (nom, -na * RR.Q), (RR.A_MAX, RR.B_MAX), (RR.A_MIN, -RR.B_MAX)], dtype=np.int64)
    A, B, Cd = k.inp("prof_a", a), k.inp("prof_b", b), k.inp("cand", cand)
    out = k.out("out", np.int64, (K, len(cand) * RR.FIELDS))
    ws = k.ws("ws", k.native.lib().v3d_profile_match_ws_bytes(K, na, nb), align=G.WS_ALIGN)
    call = lambda lib: lib.v3d_profile_match_scores(G._p(A), na, G._p(B), nb, K, G._p(Cd), len(cand), bins, G._p(out), G._p(ws), G._stream())
    return call, lambda: {"out": RR.match_scores(a, b, cand, bins)}, None


def case_warp(k, variant):
    (Ws, Hs), (Wo, Ho) = (tuple(int(v) for v in part.split("x")) for part in variant.split("-"))
    n = 3
    data = np.random.default_rng(Ws + Wo).integers(0, 65536, (n, Hs, Ws)).astype(np.uint16)
    m = (RR.rhu(RR.Fraction(Ws * RR.Q, Wo)) + 5, -RR.Q // 2, RR.rhu(RR.Fraction(Hs * RR.Q, Ho)) - 3, RR.Q // 3) if (Ws, Hs) != (Wo, Ho) else (RR.Q, 0, RR.Q, 0)
    s = k.inp("src", data.reshape(n, 1, Hs * Ws), stride=True)              # rows dense: only the frames are padded
    out = k.out("out", np.uint16, (n, Ho * Wo))
    call = lambda lib: lib.v3d_warp_u16_batch(G._p(s), n, Ws, Hs, s.frame_stride, *m, 4242, G._p(out), Wo, Ho, G._stream())
    return call, lambda: {"out": RR.warp(data, *m, 4242, Wo, Ho)}, None


G.CASES[PROFILES] = (case_profiles, PROFILE_VARIANTS, True)
G.CASES[MATCH] = (case_match, MATCH_VARIANTS, False)
G.CASES[WARP] = (case_warp, WARP_VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in (PROFILES, MATCH, WARP)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding, the outputs and the workspaces: the same bits, i.e. no unwritten cell, no
    dependence on workspace content and no byte read past a row's payload that reaches a sum"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"
