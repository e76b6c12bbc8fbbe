"""Memory behaviour of v3d_temporal_motion and v3d_temporal_filter_mc_batch, held to the header's memory contract the way
tests/test_abi_guard_gpu.py holds every other entry: the raw ctypes functions on the buffers of a guard arena
(tests/guard_arena.py), in that file's four placements and over two poison bytes.  Both cases are entered into that file's CASES
table, so its run_case, its placements and the header gate of tests/test_guard_arena_host.py cover them; this file runs them.

Variants: "vec", a 64-wide clip whose dense frames take the filter's vector route in the aligned placements and the element-wise
one in the skewed and odd ones, and "odd", 37x9: clipped blocks on both edges, rows at every alignment.  The search window reaches
S pixels past every edge of a frame and the filter's taps follow random vectors far outside it: nothing outside a frame's payload
may be read into a result, nothing outside the outputs written.  resid is an output: the entry zeroes it over the poison."""
import numpy as np
import pytest

import temporal_mc_ref as MR
import test_abi_guard_gpu as G

MOTION, FILTER = "v3d_temporal_motion", "v3d_temporal_filter_mc_batch"
VARIANTS = ("vec", "odd")
S = 3


def _moving_clip(variant, seed):
    T, H, W = G.CLIP if variant == "vec" else G.CLIP_ODD
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (H + 2 * T, W + 2 * T)).astype(np.int64)
    big = (big + np.roll(big, 1, 1)) // 2
    gray = np.stack([big[t:t + H, 2 * T - 2 * t:2 * T - 2 * t + W] for t in range(T)])
    gray = np.clip(gray + rng.integers(-4, 5, gray.shape), 0, 255).astype(np.uint8)
    gray[T // 2:] = 255 - gray[T // 2:]
    depth, _ = G._clip(T, H, W, seed + 1)
    return depth, gray


def case_motion(k, variant):
    _, gray = _moving_clip(variant, 40)
    T, H, W = gray.shape
    BW, BH = MR.blocks(W, H)
    g = k.inp("gray", gray, stride=True)
    f, b = k.out("mv_fwd", np.int16, (T, BH, BW * 2)), k.out("mv_bwd", np.int16, (T, BH, BW * 2))
    r, c = k.out("resid", np.uint64, (T,), align=8), k.out("cut", np.uint8, (T,))
    call = lambda lib: lib.v3d_temporal_motion(G._p(g), g.frame_stride_bytes, T, W, H, S, 20, G._p(f), G._p(b), G._p(r), G._p(c), G._stream())

    def expect():
        F, Bk, resid = MR.fields(gray, S)
        return {"mv_fwd": F.reshape(T, BH, BW * 2), "mv_bwd": Bk.reshape(T, BH, BW * 2), "resid": resid, "cut": MR.cuts(resid, 20, W, H)}

    return call, expect, None


def case_filter(k, variant):
    depth, gray = _moving_clip(variant, 42)
    T, H, W = gray.shape
    BW, BH = MR.blocks(W, H)
    rng = np.random.default_rng(43)
    F = rng.integers(-32, 33, (T, BH, BW, 2)).astype(np.int16)           # any field the search could write, far past the frame's edges
    Bk = rng.integers(-32, 33, (T, BH, BW, 2)).astype(np.int16)
    F[:, 0, 0], Bk[:, 0, 0] = (2, 1), (-2, -1)
    cut = np.zeros(T, np.uint8)
    cut[T - 1] = 1
    R, tau, fill, t0, n = 2, 12, 1, 1, 3
    d, g, c = k.inp("depth", depth, stride=True), k.inp("gray", gray, stride=True), k.inp("cut", cut)
    f, b = k.inp("mv_fwd", F.reshape(T, BH, BW * 2)), k.inp("mv_bwd", Bk.reshape(T, BH, BW * 2))
    o = k.out("out", np.float32, (n, H, W))
    call = lambda lib: lib.v3d_temporal_filter_mc_batch(G._p(d), d.frame_stride, G._p(g), g.frame_stride_bytes, T, W, H, t0, n, R, tau, fill,
                                                        G._p(c), G._p(f), G._p(b), G._p(o), G._stream())
    return call, lambda: {"out": MR.filter_clip(depth, gray, R, tau, cut, F, Bk, fill, t0, n)}, None


G.CASES[MOTION] = (case_motion, VARIANTS, True)
G.CASES[FILTER] = (case_filter, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] in (MOTION, FILTER)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding and the outputs: the same bits, i.e. no unwritten vector or sample and no byte
    past a frame's payload that reaches a sum"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{entry}[{variant}] {place}: {name!r} depends on the poison"
