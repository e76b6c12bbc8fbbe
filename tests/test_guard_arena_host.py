"""The guard arena (tests/guard_arena.py) proves itself on the CPU: a NumPy stand-in for a C-ABI entry is given planted faults,
each must be reported against the right buffer, side and offset, and a clean stand-in must pass.  Second group: the
completeness gate -- every function include/v3d_hip.h declares with a `void* stream` has a case in tests/test_abi_guard_gpu.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from guard_arena import Arena, GuardError, RED_ZONE

H, W, PITCH, N = 5, 13, 16, 3


def _arena(poison=0xA5):
    """src u8 [N][H][W] with padded rows and frames -> dst int16 [N][H][W] padded rows, ws f32 [7]"""
    a = Arena("cpu", poison)
    rng = np.random.default_rng(0)
    src = a.buf("src", "in", np.uint8, (N, H, W), pitch=PITCH, frame_stride=H * PITCH + 7).set(rng.integers(0, 256, (N, H, W), dtype=np.uint8))
    dst = a.buf("dst", "out", np.int16, (N, H, W), skew=2, pitch=W + 3)
    ws = a.buf("ws", "ws", np.float32, (7,), skew=4)
    a.fill().snapshot()
    return a, src, dst, ws


def _entry(a, src, dst, ws, fault=None):
    """the stand-in: dst = 2 * src, ws = scratch; `fault` plants one wrong store"""
    m = a.host()
    img = src.view(m)
    idx = dst._index()                                             # payload bytes [N][H][W * 2]
    m[idx.reshape(-1)] = (img.astype(np.int16) * 2).reshape(-1).view(np.uint8)
    m[ws.start:ws.start + ws.extent] = 1
    end = dst.start + dst.extent
    if fault == "element past out":
        m[end:end + 2] = 0
    elif fault == "row past out":
        m[end:end + W * 2] = 0
    elif fault == "byte before out":
        m[dst.start - 1] = 0
    elif fault == "write into in":
        m[src.start + 2 * src.frame_stride_bytes + 3 * PITCH + 4] ^= 0xFF
    elif fault == "row padding of out":
        m[dst.start + W * 2] = 0                                   # first padding byte of row 0
    elif fault == "row padding of in":
        m[src.start + W] = 0
    elif fault == "byte past ws":
        m[ws.start + ws.extent] = 0
    elif fault == "frame padding of in":
        m[src.start + H * PITCH + 2] = 0                           # between frame 0 and frame 1
    return dst.view(m)


def test_clean_entry_passes_and_views_strip_the_padding():
    a, src, dst, ws = _arena()
    got = _entry(a, src, dst, ws)
    a.check()
    assert got.shape == (N, H, W) and np.array_equal(got, src.get().astype(np.int16) * 2) and np.array_equal(dst.get(), got)
    assert src.pitch_bytes == PITCH and src.frame_stride_bytes == H * PITCH + 7 and dst.pitch_bytes == (W + 3) * 2
    assert src.ptr % 256 == 0 and dst.ptr % 256 == 2 and ws.ptr % 256 == 4
    assert src.ptr == a.base_ptr + src.start


FAULTS = {   # fault -> (buffer, side, offset relative to the payload's first byte, bytes)
    "element past out": ("dst", "after", lambda b: b.extent, 2),
    "row past out": ("dst", "after", lambda b: b.extent, W * 2),
    "byte before out": ("dst", "before", lambda b: -1, 1),
    "write into in": ("src", "inside", lambda b: 2 * b.frame_stride_bytes + 3 * PITCH + 4, 1),
    "row padding of out": ("dst", "inside", lambda b: W * 2, 1),
    "row padding of in": ("src", "inside", lambda b: W, 1),
    "byte past ws": ("ws", "after", lambda b: b.extent, 1),
    "frame padding of in": ("src", "inside", lambda b: H * PITCH + 2, 1),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_reported_against_its_buffer(fault):
    name, where, offset, count = FAULTS[fault]
    a, src, dst, ws = _arena()
    _entry(a, src, dst, ws, fault)
    with pytest.raises(GuardError) as e:
        a.check()
    b = {"src": src, "dst": dst, "ws": ws}[name]
    assert (e.value.name, e.value.where, e.value.offset, e.value.count) == (name, where, offset(b), count), str(e.value)
    assert name in str(e.value) and where in str(e.value) and str(offset(b)) in str(e.value)


def test_fill_poisons_outputs_workspaces_zones_and_padding():
    for poison in (0xA5, 0xFF):
        a, src, dst, ws = _arena(poison)
        m = a.host()
        assert (dst.get().view(np.uint8) == poison).all() and (ws.get().view(np.uint8) == poison).all()
        assert (m[src.start - RED_ZONE:src.start] == poison).all() and (m[dst.start + dst.extent:dst.start + dst.extent + RED_ZONE] == poison).all()
        assert (m[src.start + W:src.start + PITCH] == poison).all()                # row padding of an input
        assert (m[src.start + H * PITCH:src.start + H * PITCH + 7] == poison).all()  # frame padding
        assert np.isnan(ws.get()).all() == (poison == 0xFF)
    a.fill(0x00)                                                                   # refill with another poison keeps the inputs
    assert (dst.get() == 0).all() and np.array_equal(src.get(), src.data)


def test_red_zones_cover_a_row_and_alignment_is_enforced():
    a = Arena("cpu")
    wide = a.buf("wide", "out", np.float32, (2, 3000))
    assert wide.zone == 3000 * 4 >= RED_ZONE
    nxt = a.buf("next", "ws", np.uint8, (100,), align=16, skew=16)
    assert nxt.start - (wide.start + wide.extent) >= wide.zone + nxt.zone
    with pytest.raises(ValueError):
        a.buf("bad", "ws", np.uint8, (100,), align=16, skew=8)                     # less than the granted alignment
    with pytest.raises(ValueError):
        a.buf("overlap", "in", np.uint8, (2, 4, 8), pitch=8, frame_stride=16)
    a.fill()
    assert nxt.ptr % 256 == 16


# ------------------------------------------------------------------------------------------------------------------------
# completeness gate: the guard table is tied to the header the way tests/test_abi.py ties the binding list to it
# ------------------------------------------------------------------------------------------------------------------------
EXEMPT = {
    "v3d_sgbm_stream_wait_lockstep": "orders a stream behind the lock-step pass: moves no data, takes no buffer",
}


def _stream_entries():
    text = open(os.path.join(ROOT, "include", "v3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(v3d_[a-z0-9_]+)\s*\(([^)]*)\)", text) if re.search(r"void\s*\*\s*stream\b", m.group(2)))


def test_every_stream_entry_has_a_guard_case():
    import test_abi_guard_gpu as G
    entries = _stream_entries()
    assert len(entries) >= 31 and "v3d_sgbm_compute_batch" in entries and "v3d_version" not in entries
    missing = [e for e in entries if e not in G.CASES and e not in EXEMPT]
    assert not missing, f"declared with a stream in v3d_hip.h but without a case in tests/test_abi_guard_gpu.py: {missing}"
    stale = [e for e in list(G.CASES) + list(EXEMPT) if e not in entries]
    assert not stale, f"guard cases / exemptions for entries the header does not declare: {stale}"
    assert not set(G.CASES) & set(EXEMPT)
    assert all(isinstance(r, str) and r for r in EXEMPT.values())


def test_every_case_runs_in_every_placement():
    """the parametrisation itself: each entry has the aligned and the minimum-alignment run, each entry with a pitch or stride
    parameter both padded runs, and the two-poison runs cover all of them"""
    import test_abi_guard_gpu as G
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v3d_hip.h")).read(), flags=re.S)
    ids = [p.id for p in G._runs(G.PLACEMENTS)]
    two = [p.id for p in G._runs(("aligned", "padodd"))]
    for entry, (fn, variants, padded) in G.CASES.items():
        assert variants and callable(fn)
        args = re.search(r"\b" + entry + r"\s*\(([^)]*)\)", text).group(1)
        assert padded == bool(re.search(r"\bpitch\b|_stride\b", args)), f"{entry}: `padded` disagrees with its signature"
        for v in variants:
            for place in G.PLACEMENTS:
                assert (f"{entry}-{v}-{place}" in ids) == (padded or not place.startswith("pad"))
            assert f"{entry}-{v}-aligned" in two and (f"{entry}-{v}-padodd" in two) == padded
