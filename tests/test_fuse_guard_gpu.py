"""Memory behaviour of v3d_fuse_eye_source_batch, held to the header's memory contract the way tests/test_abi_guard_gpu.py holds
every other entry: the raw ctypes function on the buffers of a guard arena (tests/guard_arena.py), in that file's four placements
and over two poison bytes.  The case is entered into that file's CASES table, so its run_case, its placements and the header gate
of tests/test_guard_arena_host.py cover this entry too; this file runs it.

The eye is the right half of a full-SBS buffer (variant `sbs`) or the lower half of a full top-bottom one (`tb`): the buffer is
in/out, so the left eye's half of the same rows, the padding of pitched rows and of padded frames, the red zones and the SBS
frames must hold their bytes, and only the eye's payload and the workspace, which is exactly v3d_fuse_eye_source_ws_bytes long and
poisoned before the call, may change.  Every refusal returns its code with nothing enqueued: no byte of the arena changes."""
import ctypes as C

import numpy as np
import pytest

import fuse_ref as F
import test_abi_guard_gpu as G

ENTRY = "v3d_fuse_eye_source_batch"
VARIANTS = ("sbs@67x9", "tb@67x9", "sbs@530x34-16", "sbs@255x5-1")
# cells of 4 x 2 with the lower clamps, the smallest scales (an upper clamp in x: a sample that owns hundreds of columns), one
# sample per target
MAPS = {"": (16384, -24576, 32768, -16384), "16": (4096, 1 << 20, 4096, -(1 << 18)), "1": (65536, 0, 65536, 333)}


def _inputs(variant):
    layout, dims = variant.split("@")
    dims, _, mk = dims.partition("-")
    W, H = (int(v) for v in dims.split("x"))
    n, Ws, Hs, m = 3, 2 * (W // 3 + 1), H // 2 + 2, MAPS[mk]
    rng = np.random.default_rng(W + len(layout))
    sbs = rng.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)
    E = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    left = rng.integers(0, 256, E.shape, dtype=np.uint8)
    return layout, W, H, n, Ws, Hs, m, sbs, E, left


def case_fuse_eye_source(k, variant):
    layout, W, H, n, Ws, Hs, m, sbs, E, left = _inputs(variant)
    full = np.concatenate([left, E], axis=2 if layout == "sbs" else 1)
    oh, ow = full.shape[1:3]
    io = k.inp("eye_bgr", full.reshape(n, oh, ow * 3), pitch=True, stride=True, odd=5, role="inout")
    k.outs["eye_bgr"] = io
    s = k.inp("sbs_bgr", sbs.reshape(n, Hs, Ws * 3), pitch=True, stride=True, odd=5)
    ws = k.ws("ws", k.native.lib().v3d_fuse_eye_source_ws_bytes(n, Ws, Hs), align=G.WS_ALIGN)
    off = 3 * W if layout == "sbs" else H * io.pitch_bytes

    def call(lib):
        return lib.v3d_fuse_eye_source_batch(C.c_void_p(io.ptr + off), io.frame_stride_bytes, io.pitch_bytes, n, W, H, G._p(s),
                                             s.frame_stride_bytes, Ws, Hs, s.pitch_bytes, 1, *m, G._p(ws), G._stream())

    def expect():
        want = F.fuse_batch(E, sbs, 1, *m)
        assert (want != E).any()
        return {"eye_bgr": np.concatenate([left, want], axis=2 if layout == "sbs" else 1).reshape(n, oh, ow * 3)}
    return call, expect, None


G.CASES[ENTRY] = (case_fuse_eye_source, VARIANTS, True)


def _runs(placements):
    return [p for p in G._runs(placements) if p.values[0] == ENTRY]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(G.PLACEMENTS))
def test_guarded_call(native, oracle, entry, variant, place):
    G.run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", _runs(("aligned", "padodd")))
def test_two_poisons(native, oracle, entry, variant, place):
    """0xA5 and 0xFF in the red zones, the padding and the workspace: the same bits, i.e. no read past an input and no workspace
    content reaches the result"""
    a = G.run_case(native, oracle, entry, variant, place, 0xA5)
    b = G.run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{variant} {place}: {name!r} depends on the poison"


ERR_ARG, ERR_UNSUPPORTED = -1, -3


@pytest.mark.gpu
def test_every_refusal_returns_its_code_and_enqueues_nothing(native):
    import torch
    layout, W, H, n, Ws, Hs, m, sbs, E, left = _inputs("sbs@67x9")
    k = G.Kit("padodd", 0xA5, native)
    full = np.concatenate([left, E], axis=2)
    io = k.inp("eye_bgr", full.reshape(n, H, 6 * W), pitch=True, stride=True, odd=5, role="inout")
    s = k.inp("sbs_bgr", sbs.reshape(n, Hs, Ws * 3), pitch=True, stride=True, odd=5)
    lib = native.lib()
    ws = k.ws("ws", lib.v3d_fuse_eye_source_ws_bytes(n, Ws, Hs), align=G.WS_ALIGN)
    k.arena.fill().snapshot()
    before = k.arena.download()
    good = dict(eye=io.ptr + 3 * W, es=io.frame_stride_bytes, ep=io.pitch_bytes, n=n, W=W, H=H, sbs=s.ptr, ss=s.frame_stride_bytes, Ws=Ws,
                Hs=Hs, pitch=s.pitch_bytes, e=1, ax=m[0], bx=m[1], ay=m[2], by=m[3], ws=ws.ptr)
    wide = dict(W=8193, ep=3 * 8193, es=H * 3 * 8193)
    bad = [(dict(eye=None), ERR_ARG), (dict(sbs=None), ERR_ARG), (dict(ws=None), ERR_ARG), (dict(ws=ws.ptr + 8), ERR_ARG),
           (dict(ws=ws.ptr + 1), ERR_ARG), (dict(n=0), ERR_ARG), (dict(W=0), ERR_ARG),
           (dict(H=0), ERR_ARG), (dict(ep=3 * W - 1), ERR_ARG), (dict(es=H * io.pitch_bytes - 1), ERR_ARG), (dict(Ws=Ws + 1), ERR_ARG),
           (dict(Ws=0), ERR_ARG), (dict(Hs=0), ERR_ARG), (dict(pitch=3 * Ws - 1), ERR_ARG), (dict(ss=Hs * s.pitch_bytes - 1), ERR_ARG),
           (dict(e=2), ERR_ARG), (dict(e=-1), ERR_ARG), (dict(ax=4095), ERR_ARG), (dict(ax=(1 << 20) + 1), ERR_ARG), (dict(ay=4095), ERR_ARG),
           (dict(ay=(1 << 20) + 1), ERR_ARG), (dict(bx=(1 << 40) + 1), ERR_ARG), (dict(bx=-(1 << 40) - 1), ERR_ARG),
           (dict(by=(1 << 40) + 1), ERR_ARG), (dict(by=-(1 << 40) - 1), ERR_ARG),
           # too wide, with a pitch and strides that fit the width, or a stored eye finer than the frame: unsupported, unless an
           # argument is bad too
           (wide, ERR_UNSUPPORTED), (dict(Ws=2 * 8193, pitch=6 * 8193, ss=Hs * 6 * 8193), ERR_UNSUPPORTED),
           (dict(ax=65537), ERR_UNSUPPORTED), (dict(ay=65537), ERR_UNSUPPORTED), (dict(ax=1 << 20, ay=1 << 20), ERR_UNSUPPORTED),
           (dict(wide, e=2), ERR_ARG), (dict(wide, ws=ws.ptr + 8), ERR_ARG), (dict(ax=65537, ws=None), ERR_ARG),
           (dict(ay=65537, by=(1 << 40) + 1), ERR_ARG), (dict(Ws=2 * 8193, pitch=6 * 8193, ss=Hs * 6 * 8193, e=2), ERR_ARG)]

    def run(a):
        return lib.v3d_fuse_eye_source_batch(C.c_void_p(a["eye"]), a["es"], a["ep"], a["n"], a["W"], a["H"], C.c_void_p(a["sbs"]), a["ss"],
                                             a["Ws"], a["Hs"], a["pitch"], a["e"], a["ax"], a["bx"], a["ay"], a["by"], C.c_void_p(a["ws"]),
                                             G._stream())
    for change, code in bad:
        rc = run(dict(good, **change))
        assert rc == code, (change, rc, lib.v3d_last_error().decode())
    torch.cuda.synchronize()
    assert np.array_equal(k.arena.download(), before), "a refused call wrote"
    for a in (dict(n=0), dict(Ws=0), dict(Ws=Ws + 1), dict(Hs=0), dict(Ws=2 * 8193)):
        b = dict(good, **a)
        assert lib.v3d_fuse_eye_source_ws_bytes(b["n"], b["Ws"], b["Hs"]) == 0
    need = n * Hs * (Ws // 2) * 3
    assert lib.v3d_fuse_eye_source_ws_bytes(n, Ws, Hs) == -(-need // 16) * 16
    # a single frame may have any stride
    assert run(dict(good, n=1, es=0, ss=0)) == 0
    torch.cuda.synchronize()
    k.arena.check()
    got = io.get()[0].reshape(H, 2 * W, 3)
    assert np.array_equal(got[:, W:], F.fuse(E[0], sbs[0], 1, *m)) and np.array_equal(got[:, :W], left[0])
