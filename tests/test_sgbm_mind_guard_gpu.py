"""Memory behaviour of v3d_sgbm_compute_batch with a negative search window, on tests/guard_arena.py buffers driven directly (no
entry is added to the header, so test_abi_guard_gpu.CASES keeps its keys): m = -64 (the left image's column 0 is read, 64 output
columns on the right are invalid) and m = -17 (odd: the row march splits its pixel pairs), three frames, in the four placements
of test_abi_guard_gpu.py and over two poison bytes.  Every run asserts rc == 0, the expected disparity bit for bit, and that no
byte outside the output changed."""
import numpy as np
import pytest

import sgbm_mind_ref as ref
from test_abi_guard_gpu import PLACEMENTS, SGBM_ROUTES, Kit, _p, _stream

pytestmark = pytest.mark.gpu

N = 3
SHAPES = {-17: (184, 33), -64: (134, 12)}        # even widths: the row march on one route, the tiles on the other
_cases = {}


def _case(oracle, m):
    """(left [n,H,W], right, expected final disparity), computed once per m: the oracle through the identity for -17, the NumPy
    restatement for -64"""
    if m not in _cases:
        W, H = SHAPES[m]
        pairs = [ref.window_pair(W, H, 700 + i, m) for i in range(N)]
        if m > -63:
            pairs = [(ref.band_left(L, m), R) for L, R in pairs]
            want = [ref.finish(ref.from_oracle(oracle.sgbm_raw, L, R, m), m, oracle) for L, R in pairs]
        else:
            want = [ref.compute(L, R, m, oracle) for L, R in pairs]
        _cases[m] = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), np.stack(want)
    return _cases[m]


def _run(native, oracle, m, route, place, poison):
    import torch
    Ls, Rs, want = _case(oracle, m)
    _, H, W = Ls.shape
    k = Kit(place, poison, native, oracle)
    l, r = k.inp("left", Ls, pitch=True, stride=True), k.inp("right", Rs, pitch=True, stride=True)
    o = k.out("disp16", np.int16, (N, H, W))
    h = native.StereoSGBM(max_width=W, max_height=H, max_batch=N, options=SGBM_ROUTES[route], minDisparity=m)
    k.arena.fill().snapshot()
    try:
        rc = native.lib().v3d_sgbm_compute_batch(h._h, _p(l), _p(r), N, W, H, l.pitch_bytes, l.frame_stride_bytes, _p(o), _stream())
        torch.cuda.synchronize()
    finally:
        errs = h.sync_errors()
        h.close()
    assert rc == 0, native.lib().v3d_last_error().decode()
    assert errs == 0, f"{errs} lock-step time-outs"
    got = o.get()
    assert np.array_equal(got, want), f"m={m} {route} {place} poison 0x{poison:02x}: {int((got != want).sum())} pixels differ"
    k.arena.check()
    return got


@pytest.mark.parametrize("place", PLACEMENTS)
@pytest.mark.parametrize("route", list(SGBM_ROUTES))
@pytest.mark.parametrize("m", [-64, -17])
def test_guarded_batch(native, oracle, m, route, place):
    _run(native, oracle, m, route, place, 0xA5)


@pytest.mark.parametrize("place", ["aligned", "padodd"])
@pytest.mark.parametrize("route", list(SGBM_ROUTES))
@pytest.mark.parametrize("m", [-64, -17])
def test_two_poisons(native, oracle, m, route, place):
    a = _run(native, oracle, m, route, place, 0xA5)
    b = _run(native, oracle, m, route, place, 0xFF)
    assert np.array_equal(a, b), f"m={m} {route} {place}: the output depends on the poison"
