"""k_vdd's two-row strip hand-off ("row cycle"): a strip rebuilds its neighbour's edge column from the
column next to it, published two rows earlier, and the halo column's C.  Bar: the final disparity bit-exact against the CPU
oracle, and the path sum S bit-identical to the one the per-direction launches (k_chain) leave on the same handle.

Shapes: the smallest at which the protocol can go wrong.  Widths put the column a neighbour publishes (the last strip's pixel
1) on the last in-image column, on the first out-of-image one, or inside the image; heights run from fewer rows than the
look-ahead (1, 2), over exactly past it (3) and past the ring of 8 (9), to several turns of it (40)."""
import numpy as np
import pytest

from conftest import mismatch_report, textured_pair

pytestmark = pytest.mark.gpu

WIDTHS = [(8, w1) for w1 in (129, 130, 131, 255, 256, 257)] + [(4, w1) for w1 in (65, 66, 67, 128, 129)]
HEIGHTS = [1, 2, 3, 9, 40]


def _dev(native, a):
    return native.to_device(a)


def _stack(native, pairs):
    return _dev(native, np.stack([p[0] for p in pairs])), _dev(native, np.stack([p[1] for p in pairs]))


def _check_batch(native, oracle, m, pairs, what, params=None):
    """one compute() over `pairs`; every frame against the oracle, no time-out"""
    got = m.compute(*_stack(native, pairs)).cpu().numpy()
    assert m.sync_errors() == 0, f"{what}: lock-step time-outs"
    for i, p in enumerate(pairs):
        want = oracle.sgbm_compute(*p) if params is None else oracle.sgbm_compute(*p, params)
        rep = mismatch_report(got[i], want, f"{what} frame {i}")
        assert not rep, rep


def _check_S(native, m, pair, what):
    """S of the lock-step pass against S of the per-direction launches on the same handle: the same bits"""
    L, R = _dev(native, pair[0]), _dev(native, pair[1])
    raw_v, S_v = m.debug_raw(L, R, want_S=True)
    assert m.sync_errors() == 0, f"{what}: lock-step time-outs"
    assert m.get_option("lockstep") == 1
    m.set_lockstep(False)
    raw_c, S_c = m.debug_raw(L, R, want_S=True)
    assert m.sync_errors() == 0
    m.set_lockstep(True)
    rep = mismatch_report(S_v.cpu().numpy(), S_c.cpu().numpy(), f"{what} S")
    assert not rep, rep
    assert np.array_equal(raw_v.cpu().numpy(), raw_c.cpu().numpy()), f"{what}: raw disparity differs between the routes"


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("dpl,W1", WIDTHS)
def test_strip_edge_widths_and_heights(native, oracle, dpl, W1, H):
    """three frames, then one, on one handle; S of the first frame against the per-direction route"""
    W = 64 + W1
    pairs = [textured_pair(W, H, seed=1000 * dpl + 10 * W1 + H + i) for i in range(3)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=3, options={"lockstep": 1, "vdd_dpl": dpl})
    try:
        _check_batch(native, oracle, m, pairs, f"dpl {dpl} {W}x{H} n=3")
        _check_batch(native, oracle, m, pairs[2:], f"dpl {dpl} {W}x{H} n=1")
        _check_S(native, m, pairs[1], f"dpl {dpl} {W}x{H}")
    finally:
        m.close()


@pytest.mark.parametrize("dpl,W1", [(8, 257), (4, 129)])
def test_consecutive_calls_and_sequence_wrap(native, oracle, dpl, W1):
    """three calls with different content on one handle (a reused ring slot must never deliver an earlier call's granule),
    then one across the wrap of the launch sequence, where the sweep clears the whole ring"""
    W, H, n = 64 + W1, 40, 3
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"lockstep": 1, "vdd_dpl": dpl})
    try:
        for call in range(3):
            pairs = [textured_pair(W, H, seed=7000 + 100 * call + 10 * dpl + i) for i in range(n)]
            _check_batch(native, oracle, m, pairs, f"dpl {dpl} call {call}")
        m.set_option("vdd_seq", 0xFFFFF)
        pairs = [textured_pair(W, H, seed=7900 + 10 * dpl + i) for i in range(n)]
        _check_batch(native, oracle, m, pairs, f"dpl {dpl} last sequence number")
        _check_batch(native, oracle, m, pairs[::-1], f"dpl {dpl} after the wrap")
        assert m.get_option("vdd_seq") == 2, "the launch after the last sequence number carries 1, never 0"
        _check_S(native, m, pairs[0], f"dpl {dpl} after the wrap")
    finally:
        m.close()


@pytest.mark.parametrize("dpl,W1", [(8, 257), (4, 129)])
def test_mode_hh_bottom_up_pass(native, oracle, dpl, W1):
    """MODE_HH: the bottom-up pass runs the same two-row hand-off, mirrored in y, and adds to the top-down S"""
    W, H, n = 64 + W1, 40, 3
    pairs = [textured_pair(W, H, seed=8000 + 10 * dpl + i) for i in range(n)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"lockstep": 1, "vdd_dpl": dpl}, mode=1)
    try:
        _check_batch(native, oracle, m, pairs, f"HH dpl {dpl}", oracle.default_params(mode=1))
        _check_S(native, m, pairs[0], f"HH dpl {dpl}")
    finally:
        m.close()


def test_oversized_launch_waits(native, oracle):
    """a launch of more frames than are co-resident: whole frames run first, the partial one waits (bounded) with its
    strips now up to two rows apart, no time-out and the oracle's bits"""
    import torch
    W, H, n, nd = 64 + 1000, 24, 96, 3
    pairs = [textured_pair(W, H, seed=8100 + i) for i in range(nd)]
    want = [torch.from_numpy(oracle.sgbm_compute(*p)) for p in pairs]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"lockstep": 1, "vdd_dpl": 8, "vdd_launch_frames": n})
    try:
        assert m.get_option("vdd_frames_per_launch_dpl8") < n, "the launch must exceed the co-residency bound"
        got = m.compute(*_stack(native, [pairs[i % nd] for i in range(n)])).cpu()
        assert m.sync_errors() == 0
        for i in range(n):
            assert torch.equal(got[i], want[i % nd]), f"frame {i}"
    finally:
        m.close()
