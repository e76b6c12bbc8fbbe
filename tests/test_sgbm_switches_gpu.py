"""The state of an SGBM handle that the rest of the suite only sets: every key of v3d_sgbm_set_option computed with, a live
handle walked through its option states, profiling mode, the wrap of the lock-step launch sequence, and the two service
entries v3d_sgbm_stream_wait_lockstep / v3d_sgbm_workspace_bytes.  Bar: bit-exact int16 against the CPU oracle, and
sync_errors() == 0 at the end of every test ("results never depend on a switch", include/v3d_hip.h).

A workgroup order that skips a tile leaves that tile's bytes as the previous call left them, so no checked call here
follows a call on the same images: a handle is first run on other images with every switch at its default, and two
consecutive calls never see the same pair in the same frame slot."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import mismatch_report, textured_pair

pytestmark = pytest.mark.gpu

ERR_ARG = -1                       # V3D_ERR_ARG (include/v3d_hip.h)
PROF_MAX_CALLS = 512               # V3D_PROF_MAX_CALLS (video-3d-pipeline_amd/csrc/v3d_sgbm_internal.h)
SEQ_LAST = 0xFFFFF                 # the last value of the 20-bit launch sequence; 0 is never carried

# every settable switch that a compute call reads, at its default (v3d_sgbm_internal.h)
DEFAULTS = {"lockstep": 1, "hfused": 1, "chain_dpl": 4, "hsplit": 0, "vdd_dpl": 0, "cost_band": 90, "cost_xcd": 1,
            "vdd_xcd": 0, "hf_xcd": 0, "hf_persist": 1, "lrm_tiles": 0}


@functools.lru_cache(maxsize=None)
def _pair(W, H, seed):
    L, R = textured_pair(W, H, seed=seed)
    L.setflags(write=False); R.setflags(write=False)
    return L, R


_REF = {}


def _ref(oracle, kind, W, H, seed, mode=0):
    """the oracle's answer for _pair(W, H, seed): computed once per session, shared, read-only"""
    key = (kind, W, H, seed, mode)
    if key not in _REF:
        fn = {"disp": oracle.sgbm_compute, "raw": oracle.sgbm_raw, "cost": oracle.cost_volume}[kind]
        a = fn(*_pair(W, H, seed), oracle.default_params(mode=mode))
        a.setflags(write=False)
        _REF[key] = a
    return _REF[key]


def _up(native, W, H, seeds):
    """device tensors of the pairs with these seeds: [n, H, W] for a list, [H, W] for a single seed"""
    if isinstance(seeds, int):
        L, R = _pair(W, H, seeds)
        return native.to_device(np.array(L)), native.to_device(np.array(R))
    return (native.to_device(np.stack([_pair(W, H, s)[0] for s in seeds])),
            native.to_device(np.stack([_pair(W, H, s)[1] for s in seeds])))


def _same(got, want, name):
    r = mismatch_report(got, want, name)
    assert not r, r


def _compute_checked(native, oracle, m, W, H, seeds, mode, name):
    """one batched compute call on the pairs `seeds`, every frame against the oracle; returns the disparities"""
    got = m.compute(*_up(native, W, H, list(seeds))).cpu().numpy()
    for i, s in enumerate(seeds):
        _same(got[i], _ref(oracle, "disp", W, H, s, mode), f"{name}: frame {i} (seed {s})")
    return got


# ----------------------------------------------------------------------------------------------------------------------
# 1. switches that no other test computes with: cost_band, cost_xcd, vdd_xcd, hf_xcd
# ----------------------------------------------------------------------------------------------------------------------
# (W, H, batch): three k_cost column strips, the last ragged, bands that end mid-image / one column strip, fewer than 8
# workgroups in every grid / exact multiples of the strip widths.  Grid sizes: k_cost 54, 45, 36, 25, 20, 18, 15, 9, 5, 2, 1;
# k_hfused 9, 5, 3, 2, 1; k_vdd 9, 6, 4, 2, 1 (a multiple of 8: the 48 workgroups of k_cost in the walk of section 2)
SHAPES = [(64 + 136, 45, 3), (64 + 59, 9, 1), (64 + 256, 33, 1)]
SHAPE_IDS = [f"{w}x{h}x{n}" for w, h, n in SHAPES]
COST_BANDS = [8, 9, 13, 44, 45, 46, 65536]     # a band of 8, bands that do not divide H = 45, H - 1, H, H + 1, one band for any H


def _switch_case(native, oracle, W, H, n, options, mode=0, cost=False, raw=False, before=None):
    """a fresh handle run once on other images at the defaults, then switched to `options` and held to the oracle: a
    batched compute, the cost volume and / or the raw disparity of single frames, and a batched compute on the first
    images.  Each call's images differ, frame slot by frame slot, from those of the call before it."""
    A, B, P = [400 + i for i in range(n)], 410, [420 + i for i in range(n)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, mode=mode)
    try:
        m.compute(*_up(native, W, H, P))                                  # defaults: fills every workspace with other data
        for k, v in options.items():
            m.set_option(k, v)
        if before:
            before(m)
        _compute_checked(native, oracle, m, W, H, A, mode, f"{options}")
        if cost:
            for s in (B, A[-1]):
                got = m.debug_cost_volume(*_up(native, W, H, s)).cpu().numpy()
                _same(got, _ref(oracle, "cost", W, H, s, mode), f"{options}: C of seed {s}")
        if raw:
            for s in (B, A[0]):
                got = m.debug_raw(*_up(native, W, H, s)).cpu().numpy()
                _same(got, _ref(oracle, "raw", W, H, s, mode), f"{options}: raw disparity of seed {s}")
        _compute_checked(native, oracle, m, W, H, P, mode, f"{options}, second batch")
        assert m.sync_errors() == 0
    finally:
        m.close()


@pytest.mark.parametrize("xcd", [1, 0])
@pytest.mark.parametrize("band", COST_BANDS)
@pytest.mark.parametrize("W,H,n", SHAPES, ids=SHAPE_IDS)
def test_cost_band_and_tile_order(native, oracle, W, H, n, band, xcd):
    """k_cost at band heights other than 90 (the 5-row running sum restarts at every band), in both workgroup orders, on
    grids whose size is no multiple of the 8 XCDs"""
    _switch_case(native, oracle, W, H, n, {"cost_band": band, "cost_xcd": xcd}, cost=True)


@pytest.mark.parametrize("dpl", [4, 8])
@pytest.mark.parametrize("W,H,n", SHAPES, ids=SHAPE_IDS)
def test_hfused_xcd_order(native, oracle, W, H, n, dpl):
    """hf_xcd acts only with one wave per row group (hf_persist = 0): both lane mappings"""
    _switch_case(native, oracle, W, H, n, {"hf_persist": 0, "hf_xcd": 1, "chain_dpl": dpl}, raw=True)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dpl", [4, 8])
@pytest.mark.parametrize("W,H,n", SHAPES, ids=SHAPE_IDS)
def test_lockstep_xcd_order(native, oracle, W, H, n, dpl, mode):
    """vdd_xcd on one co-resident launch, both strip mappings, top-down (mode 0) and with the bottom-up pass (mode 1)"""
    def one_launch(m):
        assert n <= m.get_option(f"vdd_frames_per_launch_dpl{dpl}"), "the batch must be one co-resident launch"
        assert m.get_option("lockstep") == 1
    _switch_case(native, oracle, W, H, n, {"vdd_xcd": 1, "vdd_dpl": dpl}, mode=mode, raw=True, before=one_launch)


@pytest.mark.parametrize("W,H,n", SHAPES, ids=SHAPE_IDS)
def test_all_four_switches_off_default(native, oracle, W, H, n):
    _switch_case(native, oracle, W, H, n, {"cost_band": 13, "cost_xcd": 0, "vdd_xcd": 1, "hf_xcd": 1, "hf_persist": 0},
                 cost=True, raw=True)


def test_oversized_lockstep_launch_with_xcd_order(native, oracle):
    """the shapes of test_oversized_lockstep_launch_waits_instead_of_deadlocking (96 frames x 8 strips = 768 workgroups on
    2 x 256 slots) with vdd_xcd = 1.  An over-sized launch makes progress because workgroups become resident in strip
    order; the XCD order would turn a resident prefix into eight ranges of strips and leave a frame that lies across two
    ranges with some strips resident first and the rest last.  launch_vdd therefore drops the XCD order for a launch
    beyond the co-residency bound: no time-out, the oracle's bits."""
    import torch
    W, H, n, nd = 64 + 1000, 48, 96, 3
    want = [_ref(oracle, "disp", W, H, 300 + i) for i in range(nd)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"vdd_dpl": 8, "vdd_launch_frames": n, "vdd_xcd": 1})
    assert m.get_option("vdd_frames_per_launch_dpl8") < n, "the launch must exceed the co-residency bound"
    Ls, Rs = _up(native, W, H, [300 + i % nd for i in range(n)])
    got = m.compute(Ls, Rs)
    assert m.sync_errors() == 0
    for i in range(n):
        assert torch.equal(got[i].cpu(), torch.from_numpy(np.array(want[i % nd]))), f"frame {i}"
    m.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. switching a live handle
# ----------------------------------------------------------------------------------------------------------------------
LIVE_W, LIVE_H = 64 + 136, 60
# each state is the set_option calls that lead to it from the state before; the handle is never re-created
WALK = [
    {"chain_dpl": 8},                                                   # 4 -> 8 while hfused = 1 (persistent k_hfused<8>)
    {"cost_band": 8, "cost_xcd": 0},                                    # k_cost: 3 x 8 x 2 = 48 workgroups
    {"hf_persist": 0, "hf_xcd": 1},                                     # one wave per row group, no ticket
    {"chain_dpl": 4, "cost_band": 9, "cost_xcd": 1},                    # 8 -> 4 while hfused = 1
    {"hsplit": 1, "vdd_dpl": 4, "vdd_xcd": 1},                          # k_hscan + k_hfused<4, 2>: checkpoints in the dpl-4 layout
    {"chain_dpl": 8, "cost_band": 13},                                  # the same with the dpl-8 layout
    {"hsplit": 0, "hfused": 0, "lrm_tiles": 1, "vdd_dpl": 8},           # both horizontal paths as k_chain launches
    {"chain_dpl": 4, "cost_band": 44, "hf_xcd": 0},                     # 8 -> 4 while hfused = 0
    {"chain_dpl": 8, "cost_band": 45, "vdd_xcd": 0},                    # 4 -> 8 while hfused = 0
    {"lockstep": 0, "cost_band": 46, "cost_xcd": 0},                    # every path a k_chain launch
    {"hfused": 1, "hf_persist": 1, "cost_band": 65536, "lrm_tiles": 0}, # back to the ticket counter after calls without it
    {"lockstep": 1, "vdd_dpl": 0, "chain_dpl": 4, "hsplit": 1},
    {"hsplit": 0, "cost_band": 90, "cost_xcd": 1},                      # = DEFAULTS
]
WALK_VALUES = {"chain_dpl": {4, 8}, "hfused": {0, 1}, "hsplit": {0, 1}, "hf_persist": {0, 1}, "lrm_tiles": {0, 1},
               "vdd_dpl": {0, 4, 8}, "cost_band": {90, *COST_BANDS}, "cost_xcd": {0, 1}, "vdd_xcd": {0, 1}, "hf_xcd": {0, 1},
               "lockstep": {0, 1}}


def test_walk_visits_every_value():
    """the walk itself (no GPU work): it passes through every value of every key, changes chain_dpl in both directions under
    hfused = 1 and under hfused = 0, and ends at the defaults"""
    state, seen, dpl_moves = dict(DEFAULTS), {k: {v} for k, v in DEFAULTS.items()}, set()
    for step in WALK:
        if "chain_dpl" in step and step["chain_dpl"] != state["chain_dpl"]:
            dpl_moves.add((step.get("hfused", state["hfused"]), state["chain_dpl"], step["chain_dpl"]))
        state.update(step)
        for k, v in step.items():
            seen[k].add(v)
    assert len(WALK) >= 10 and state == DEFAULTS
    assert seen == WALK_VALUES
    assert dpl_moves >= {(1, 4, 8), (1, 8, 4), (0, 4, 8), (0, 8, 4)}


@pytest.mark.parametrize("mode", [0, 1])
def test_live_handle_walks_its_option_states(native, oracle, mode):
    """v3d_sgbm_set_option is callable at any time: one handle, one geometry, a compute after every change.  No ticket,
    checkpoint, granule or S layout of the state before may reach the next call.  The two batches alternate, so a tile a
    state fails to write holds the other batch's data."""
    W, H = LIVE_W, LIVE_H
    batches = [(500, 501), (502, 503)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2, mode=mode)
    try:
        _compute_checked(native, oracle, m, W, H, batches[1], mode, "defaults")
        state = dict(DEFAULTS)
        for i, step in enumerate(WALK):
            for k, v in step.items():
                m.set_option(k, v)
            state.update(step)
            _compute_checked(native, oracle, m, W, H, batches[i % 2], mode, f"state {i} {state}")
            assert m.sync_errors() == 0, f"state {i} {state}"
        assert {k: m.get_option(k) for k in DEFAULTS} == DEFAULTS
        _compute_checked(native, oracle, m, W, H, batches[len(WALK) % 2], mode, "back at the defaults")
        assert m.sync_errors() == 0
    finally:
        m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_debug_calls_between_computes(native, oracle, mode):
    """the two debug entries share the handle's workspaces with compute: a single-frame debug_raw and debug_cost_volume on
    other images between two batched computes, all four results the oracle's"""
    W, H = LIVE_W, LIVE_H
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2, mode=mode)
    try:
        _compute_checked(native, oracle, m, W, H, (500, 501), mode, "first compute")
        _same(m.debug_raw(*_up(native, W, H, 502)).cpu().numpy(), _ref(oracle, "raw", W, H, 502, mode), "debug_raw")
        _same(m.debug_cost_volume(*_up(native, W, H, 503)).cpu().numpy(), _ref(oracle, "cost", W, H, 503, mode), "debug_cost_volume")
        _compute_checked(native, oracle, m, W, H, (501, 500), mode, "second compute")
        assert m.sync_errors() == 0
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. profiling mode (what bench.py measures)
# ----------------------------------------------------------------------------------------------------------------------
PROF_W, PROF_H = 64 + 136, 45
# both routes in both modes: together they pass every prof_mark site of run_sgbm, sgbm_cost_volume and sgbm_aggregate_wta
ROUTES = [(0, {}), (0, {"lockstep": 0, "hfused": 0}), (1, {}), (1, {"lockstep": 0, "hfused": 0})]
ROUTE_IDS = ["lockstep", "per-direction", "lockstep-hh", "per-direction-hh"]


def _stage_names(native):
    L = native.lib()
    return [L.v3d_sgbm_profile_stage_name(i).decode() for i in range(L.v3d_sgbm_profile_stage_count())]


def _read_checked(native, m, calls):
    """synchronise, read the profile: the count, the stage names in order, totals finite and >= 0 (no duration is judged)"""
    import torch
    torch.cuda.synchronize()
    got_calls, totals = m.read_profile()
    assert got_calls == calls
    assert list(totals) == _stage_names(native)
    vals = np.array(list(totals.values()), np.float64)
    assert np.isfinite(vals).all() and (vals >= 0).all()
    if calls == 0:
        assert (vals == 0).all()
    else:
        assert vals.sum() > 0
    return totals


@pytest.mark.parametrize("mode,options", ROUTES, ids=ROUTE_IDS)
def test_profiled_calls_give_the_same_bits(native, oracle, mode, options):
    W, H, seeds = PROF_W, PROF_H, (400, 401, 402)
    m = native.StereoSGBM(max_width=W, max_height=H, options=options, mode=mode)
    try:
        off = [m.compute(*_up(native, W, H, s)).cpu().numpy() for s in seeds]
        m.profile(True)
        on = [m.compute(*_up(native, W, H, s)) for s in seeds]          # no host read between the calls: events only
        _read_checked(native, m, 3)
        for s, a, b in zip(seeds, off, on):
            _same(b.cpu().numpy(), _ref(oracle, "disp", W, H, s, mode), f"profiled, seed {s}")
            _same(a, _ref(oracle, "disp", W, H, s, mode), f"not profiled, seed {s}")
        assert m.sync_errors() == 0
    finally:
        m.close()


@pytest.mark.parametrize("mode,options", ROUTES, ids=ROUTE_IDS)
def test_profile_counts_full_compute_calls_only_and_resets(native, oracle, mode, options):
    """only v3d_sgbm_compute[_batch] calls are recorded: the debug entries between them leave the count alone (and record
    into the slot the next compute overwrites).  profile(1) resets; profile(0) reads as nothing; computes stay right."""
    W, H = PROF_W, PROF_H
    m = native.StereoSGBM(max_width=W, max_height=H, options=options, mode=mode)
    want = lambda s: _ref(oracle, "disp", W, H, s, mode)
    try:
        _read_checked(native, m, 0)                                      # never enabled
        m.profile(True)
        _same(m.debug_raw(*_up(native, W, H, 402)).cpu().numpy(), _ref(oracle, "raw", W, H, 402, mode), "debug_raw before")
        _read_checked(native, m, 0)
        a = m.compute(*_up(native, W, H, 400))
        _same(m.debug_raw(*_up(native, W, H, 402)).cpu().numpy(), _ref(oracle, "raw", W, H, 402, mode), "debug_raw between")
        b = m.compute(*_up(native, W, H, 401))
        _same(m.debug_cost_volume(*_up(native, W, H, 402)).cpu().numpy(), _ref(oracle, "cost", W, H, 402, mode), "debug_cost_volume between")
        c = m.compute(*_up(native, W, H, 400))
        _read_checked(native, m, 3)
        for got, s in ((a, 400), (b, 401), (c, 400)):
            _same(got.cpu().numpy(), want(s), f"profiled, seed {s}")
        m.profile(True)                                                  # enabling again resets
        _read_checked(native, m, 0)
        _same(m.compute(*_up(native, W, H, 401)).cpu().numpy(), want(401), "after the reset")
        _read_checked(native, m, 1)
        m.profile(False)
        _read_checked(native, m, 0)
        _same(m.compute(*_up(native, W, H, 400)).cpu().numpy(), want(400), "profiling off again")
        _read_checked(native, m, 0)                                      # off: nothing is recorded
        assert m.sync_errors() == 0
    finally:
        m.close()


@pytest.mark.parametrize("options", [{}, {"lockstep": 0, "hfused": 0}], ids=["lockstep", "per-direction"])
def test_profile_stops_at_its_cap(native, oracle, options):
    """more than V3D_PROF_MAX_CALLS calls with profiling on: the count stops at the cap, no event beyond the table is
    touched, and the calls after the cap are still the oracle's"""
    W, H = 69, 1
    m = native.StereoSGBM(max_width=W, max_height=H, options=options)
    try:
        L, R = _up(native, W, H, 600)
        L2, R2 = _up(native, W, H, 601)
        m.profile(True)
        for _ in range(PROF_MAX_CALLS - 1):
            m.compute(L2, R2)
        _read_checked(native, m, PROF_MAX_CALLS - 1)
        at_cap = m.compute(L, R)
        over = [m.compute(L2, R2), m.compute(L, R)]
        _read_checked(native, m, PROF_MAX_CALLS)
        _same(at_cap.cpu().numpy(), _ref(oracle, "disp", W, H, 600), "the call that reaches the cap")
        _same(over[0].cpu().numpy(), _ref(oracle, "disp", W, H, 601), "first call beyond the cap")
        _same(over[1].cpu().numpy(), _ref(oracle, "disp", W, H, 600), "second call beyond the cap")
        m.profile(True)                                                  # the table is reusable after the cap
        _same(m.compute(L2, R2).cpu().numpy(), _ref(oracle, "disp", W, H, 601), "after the reset")
        _read_checked(native, m, 1)
        assert m.sync_errors() == 0
    finally:
        m.close()


def test_profile_read_refusals(native, oracle):
    """a buffer one stage short, a null handle, a null buffer: V3D_ERR_ARG, and nothing is written"""
    import torch
    W, H = PROF_W, PROF_H
    L = native.lib()
    n = L.v3d_sgbm_profile_stage_count()
    assert n == len(set(_stage_names(native))) and n > 1 and L.v3d_sgbm_profile_stage_name(n) == b"" and L.v3d_sgbm_profile_stage_name(-1) == b""
    m = native.StereoSGBM(max_width=W, max_height=H)
    try:
        m.profile(True)
        got = m.compute(*_up(native, W, H, 400))
        torch.cuda.synchronize()
        buf = (C.c_double * (n + 1))(*([-7.0] * (n + 1)))
        assert L.v3d_sgbm_profile_read(m._h, buf, n - 1) == ERR_ARG
        assert L.v3d_sgbm_profile_read(m._h, buf, 0) == ERR_ARG
        assert L.v3d_sgbm_profile_read(m._h, buf, -1) == ERR_ARG
        assert L.v3d_sgbm_profile_read(None, buf, n) == ERR_ARG
        assert L.v3d_sgbm_profile_read(m._h, None, n) == ERR_ARG
        assert list(buf) == [-7.0] * (n + 1), "a refused read wrote to the buffer"
        assert L.v3d_sgbm_profile_read(m._h, buf, n) == 1               # the count survives the refusals
        assert buf[n] == -7.0 and all(np.isfinite(buf[i]) and buf[i] >= 0 for i in range(n))
        assert L.v3d_sgbm_profile(None, 1) == ERR_ARG
        _same(got.cpu().numpy(), _ref(oracle, "disp", W, H, 400), "profiled")
        assert m.sync_errors() == 0
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. the wrap of the 20-bit lock-step launch sequence (through the test hook "vdd_seq")
#
# What these tests cannot show: a missing sweep of the granule ring only misbehaves when a strip polls a granule BEFORE its
# neighbour has written it and finds a stale tag of the same (sequence, row) there -- a matter of timing.  They prove that
# the wrap branch runs (the sequence read back afterwards says which numbers the launches carried), that the sweep is
# ordered correctly against the launches around it on the stream, and that the pass leaves the oracle's bits afterwards;
# they do not prove that every stale tag is gone.
# ----------------------------------------------------------------------------------------------------------------------
def test_sequence_wraps_between_calls(native, oracle):
    """call 1 leaves granules tagged with sequence 1; the hook moves the handle to the end of the sequence; the third call
    wraps (sweep, then sequence 1 again) on a taller frame, over what the first call left"""
    W, HA, HC = 64 + 136, 45, 60                 # three 64-column strips: both edge exchanges
    m = native.StereoSGBM(max_width=W, max_height=HC, options={"vdd_dpl": 4})
    try:
        assert m.get_option("vdd_seq") == 1 and m.get_option("lockstep") == 1
        _compute_checked(native, oracle, m, W, HA, [400], 0, "pair A, sequence 1")
        assert m.get_option("vdd_seq") == 2
        m.set_option("vdd_seq", SEQ_LAST)
        assert m.get_option("vdd_seq") == SEQ_LAST
        _compute_checked(native, oracle, m, W, HA, [401], 0, "pair B, the last sequence number")
        assert m.get_option("vdd_seq") == 1, "the launch after the last sequence number carries 1, never 0"
        _compute_checked(native, oracle, m, W, HC, [500], 0, "pair C, the wrapping launch")
        assert m.get_option("vdd_seq") == 2
        _compute_checked(native, oracle, m, W, HA, [400], 0, "pair A again")
        assert m.get_option("vdd_seq") == 3
        assert m.sync_errors() == 0
    finally:
        m.close()


def test_sequence_wraps_inside_a_call(native, oracle):
    """one frame per launch, three frames: the launches of one call carry 0xFFFFE, 0xFFFFF and, after the sweep, 1 -- the sweep
    sits between two launches of the same call on the stream"""
    W, H = 64 + 136, 45
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=3, options={"vdd_dpl": 4, "vdd_launch_frames": 1})
    try:
        _compute_checked(native, oracle, m, W, H, (420, 421, 422), 0, "before")          # sequence 1, 2, 3 in the ring
        assert m.get_option("vdd_seq") == 4
        m.set_option("vdd_seq", SEQ_LAST - 1)
        _compute_checked(native, oracle, m, W, H, (400, 401, 402), 0, "the wrapping call")
        assert m.get_option("vdd_seq") == 2
        _compute_checked(native, oracle, m, W, H, (402, 400, 401), 0, "the call after")
        assert m.get_option("vdd_seq") == 5
        assert m.sync_errors() == 0
    finally:
        m.close()


def test_sequence_wraps_on_the_bottom_up_pass(native, oracle):
    """mode 1: the top-down pass carries the last sequence number, the bottom-up pass of the same call wraps"""
    W, H = 64 + 136, 45
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2, mode=1, options={"vdd_dpl": 4})
    try:
        assert 2 <= m.get_option("vdd_frames_per_launch_dpl4"), "each pass must be one launch"
        _compute_checked(native, oracle, m, W, H, (420, 421), 1, "before")
        assert m.get_option("vdd_seq") == 3
        m.set_option("vdd_seq", SEQ_LAST)
        _compute_checked(native, oracle, m, W, H, (400, 401), 1, "the wrapping call")
        assert m.get_option("vdd_seq") == 2
        _compute_checked(native, oracle, m, W, H, (401, 400), 1, "the call after")
        assert m.get_option("vdd_seq") == 4
        assert m.sync_errors() == 0
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. service entries
# ----------------------------------------------------------------------------------------------------------------------
def test_stream_wait_lockstep_entry(native, oracle):
    """v3d_sgbm_stream_wait_lockstep: OK before any pass (nothing recorded), after a lock-step compute, and after a compute
    without the pass (the event of the earlier one); a null handle is refused.  Nothing is claimed about the order of the
    two streams: only that the calls succeed and leave the matcher's results alone."""
    import torch
    W, H = PROF_W, PROF_H
    L = native.lib()
    side = torch.cuda.Stream()
    m = native.StereoSGBM(max_width=W, max_height=H)
    try:
        m.stream_wait_lockstep(side)                                     # raises on any return code but V3D_OK
        a = m.compute(*_up(native, W, H, 400))
        m.stream_wait_lockstep(side)
        m.set_lockstep(False)
        b = m.compute(*_up(native, W, H, 401))
        assert m.get_option("lockstep") == 0
        m.stream_wait_lockstep(side)
        assert L.v3d_sgbm_stream_wait_lockstep(None, C.c_void_p(side.cuda_stream)) == ERR_ARG
        side.synchronize()
        torch.cuda.current_stream().synchronize()
        _same(a.cpu().numpy(), _ref(oracle, "disp", W, H, 400), "lock-step compute")
        _same(b.cpu().numpy(), _ref(oracle, "disp", W, H, 401), "per-direction compute")
        m.set_lockstep(True)
        _same(m.compute(*_up(native, W, H, 402)).cpu().numpy(), _ref(oracle, "disp", W, H, 402), "a further compute")
        assert m.sync_errors() == 0
    finally:
        m.close()


def test_workspace_bytes_entry(native, oracle):
    """> 0, whole 256-byte units, strictly growing with max_batch and max_height, 0 for a null handle, and constant over a
    handle's life: no set_option and no compute call allocates"""
    W, H = PROF_W, PROF_H

    def size(h, b):
        m = native.StereoSGBM(max_width=W, max_height=h, max_batch=b)
        s = m.workspace_bytes
        m.close()
        return s
    sizes = {(h, b): size(h, b) for h in (H, H + 1, 2 * H) for b in (1, 2, 3)}
    assert all(s > 0 and s % 256 == 0 for s in sizes.values())
    for h in (H, H + 1, 2 * H):
        assert sizes[h, 1] < sizes[h, 2] < sizes[h, 3]
    for b in (1, 2, 3):
        assert sizes[H, b] < sizes[H + 1, b] < sizes[2 * H, b]
    assert native.lib().v3d_sgbm_workspace_bytes(None) == 0

    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2)
    try:
        ws = m.workspace_bytes
        assert ws == sizes[H, 2]
        for step in WALK:
            for k, v in step.items():
                m.set_option(k, v)
            assert m.workspace_bytes == ws, step
        for k, v in (("reserve_cus", 2), ("reserve_cus", 0), ("vdd_launch_frames", 1), ("vdd_spin_limit", 100000), ("vdd_seq", 77)):
            m.set_option(k, v)
            assert m.workspace_bytes == ws, k
        _compute_checked(native, oracle, m, W, H, (400, 401), 0, "lock-step, one frame per launch")
        assert m.workspace_bytes == ws
        m.profile(True)                                                  # events are host objects, not device workspace
        m.set_option("lockstep", 0); m.set_option("hfused", 0)
        _compute_checked(native, oracle, m, W, H, (401, 402), 0, "per-direction")
        assert m.workspace_bytes == ws
        assert m.sync_errors() == 0
    finally:
        m.close()
