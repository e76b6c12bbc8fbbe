"""The matcher with a negative search window (v3d_sgbm_params.minDisparity in [-64, 0]) on the device: final disparity, the raw
image (v3d_sgbm_debug_raw) and the cost volume (v3d_sgbm_debug_cost_volume), bit-exact.

  m in {-1, -17, -32, -62}   against the C oracle through the identity of tests/sgbm_mind_ref.py (the oracle on the shifted left
                             image, re-placed), on the k_cost strip / 64 x 16 tile edge shapes, the 16-pixels-per-thread row
                             march and the smallest accepted frame
  m in {-63, -64}            against the NumPy restatement (the left image's border column is read: no identity)

The smallest frame here is 69 x 9 (five cost columns): the handle refuses W <= 68 at every m (test_narrow_frames_stay_refused).
Every handle switch that changes the route must give the same bits; every test ends with sync_errors() == 0."""
import ctypes as C

import numpy as np
import pytest

import sgbm_mind_ref as ref
from conftest import mismatch_report

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -3
ORACLE_M = [-1, -17, -32, -62]
ORACLE_SHAPES = [(184, 33), (253, 33), (505, 17), (2050, 6), (69, 9)]
REF_M = [-63, -64]
REF_SHAPES = [(200, 14), (69, 9)]
# lrm_tiles 0/1, lockstep 0/1, hfused 0/1: the default, each switch alone, all three together
ROUTES = [{}, {"lrm_tiles": 1}, {"lockstep": 0}, {"hfused": 0}, {"lrm_tiles": 1, "lockstep": 0, "hfused": 0}]


def _expected_oracle(oracle, L, R, m, mode):
    """(cost volume, raw, {speckle window: final}) through the identity; L carries the band already"""
    p = oracle.default_params(mode=mode)
    raw = ref.from_oracle(oracle.sgbm_raw, L, R, m, params=p)
    return oracle.cost_volume(ref.shift_left(L, m), R, p), raw, {sw: ref.finish(raw, m, oracle, sw) for sw in (100, 0)}


def _expected_ref(oracle, L, R, m, mode):
    raw = ref.raw(L, R, m, mode)
    return ref.cost_volume(L, R, m).astype(np.int16), raw, {sw: ref.finish(raw, m, oracle, sw) for sw in (100, 0)}


def _check_all_routes(native, L, R, m, mode, want):
    want_C, want_raw, want_final = want
    H, W = L.shape
    dl, dr = native.to_device(L), native.to_device(R)
    bad = []
    for options in ROUTES:
        for sw in (100, 0):
            h = native.StereoSGBM(max_width=W, max_height=H, options=options, minDisparity=m, mode=mode, speckleWindowSize=sw)
            name = f"m={m} mode={mode} {options} speckle={sw} {W}x{H}"
            bad.append(mismatch_report(h.compute(dl, dr).cpu().numpy(), want_final[sw], f"{name} final"))
            if sw == 100:
                bad.append(mismatch_report(h.debug_raw(dl, dr).cpu().numpy(), want_raw, f"{name} raw"))
                bad.append(mismatch_report(h.debug_cost_volume(dl, dr).cpu().numpy(), want_C, f"{name} C"))
            errs = h.sync_errors()
            h.close()
            assert errs == 0, f"{name}: {errs} lock-step time-outs"
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,H", ORACLE_SHAPES)
@pytest.mark.parametrize("m", ORACLE_M)
def test_against_the_oracle_through_the_identity(native, oracle, m, W, H, mode):
    L, R = ref.window_pair(W, H, 3 * W + H, m)
    L = ref.band_left(L, m)
    want = _expected_oracle(oracle, L, R, m, mode)
    assert (want[1][:, 64 + m:W + m] != ref.invalid(m)).any(), "the pair has no valid pixel: the test would see nothing"
    _check_all_routes(native, L, R, m, mode, want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,H", REF_SHAPES)
@pytest.mark.parametrize("m", REF_M)
def test_against_the_restatement(native, oracle, m, W, H, mode):
    L, R = ref.window_pair(W, H, 3 * W + H, m)
    _check_all_routes(native, L, R, m, mode, _expected_ref(oracle, L, R, m, mode))


@pytest.mark.parametrize("W,H", [(184, 33), (253, 33)])
@pytest.mark.parametrize("m", [-17, -64])
def test_batch_equals_single_calls_with_a_padded_pitch(native, oracle, m, W, H):
    """three frames at pitch W + 13 and a frame stride of H * pitch + 7 through v3d_sgbm_compute_batch: each frame is what
    a single dense call gives (and, for m = -17, what the oracle gives through the identity)"""
    import torch
    n, pitch = 3, W + 13
    stride = H * pitch + 7
    pairs = [ref.window_pair(W, H, 50 + i, m) for i in range(n)]
    if m > -63:
        pairs = [(ref.band_left(L, m), R) for L, R in pairs]
    bufs = []
    for side in (0, 1):
        flat = torch.full((n * stride,), 0x5A, dtype=torch.uint8, device="cuda")
        for i, p in enumerate(pairs):
            flat[i * stride:i * stride + H * pitch].view(H, pitch)[:, :W] = native.to_device(p[side])
        bufs.append(flat)
    out = torch.full((n, H, W), 0x5A5A, dtype=torch.int16, device="cuda")
    h = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, minDisparity=m)
    P = C.c_void_p
    rc = native.lib().v3d_sgbm_compute_batch(h._h, P(bufs[0].data_ptr()), P(bufs[1].data_ptr()), n, W, H, pitch, stride, P(out.data_ptr()),
                                            P(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, native.lib().v3d_last_error().decode()
    got = out.cpu().numpy()
    bad = []
    for i, (L, R) in enumerate(pairs):
        single = h.compute(native.to_device(L), native.to_device(R)).cpu().numpy()
        bad.append(mismatch_report(got[i], single, f"m={m} frame {i}: batch vs single"))
        if m > -63:
            bad.append(mismatch_report(single, _expected_oracle(oracle, L, R, m, 0)[2][100], f"m={m} frame {i}: single vs oracle"))
    assert h.sync_errors() == 0
    h.close()
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad)


def test_m0_is_the_oracle_bit_for_bit(native, oracle):
    """minDisparity = 0 given explicitly: the handle the suite has always tested"""
    from conftest import textured_pair
    L, R = textured_pair(184, 33, seed=9)
    h = native.StereoSGBM(max_width=184, max_height=33, minDisparity=0)
    got = h.compute(native.to_device(L), native.to_device(R)).cpu().numpy()
    assert h.sync_errors() == 0
    h.close()
    assert np.array_equal(got, oracle.sgbm_compute(L, R))


def _create_rc(native, W=134, H=40, **kw):
    import torch
    h = C.c_void_p()
    p = native.default_params(**kw)
    return native.lib().v3d_sgbm_create(C.byref(p), torch.cuda.current_device(), W, H, 1, C.byref(h)), h


@pytest.mark.parametrize("m", [1, -65, 16, -128])
def test_values_outside_the_range_are_refused(native, m):
    rc, h = _create_rc(native, minDisparity=m)
    assert rc == ERR_UNSUPPORTED and not h.value
    assert b"-64 <= minDisparity <= 0" in native.lib().v3d_last_error()
    with pytest.raises(native.NativeError, match="minDisparity"):
        native.StereoSGBM(max_width=134, max_height=40, minDisparity=m)
    for ok in (0, -64):
        rc, h = _create_rc(native, minDisparity=ok)
        assert rc == 0 and h.value
        assert native.lib().v3d_sgbm_sync_errors(h) == 0
        native.lib().v3d_sgbm_destroy(h)


def test_narrow_frames_stay_refused(native):
    """W1 = 1 (65 x 9) is outside the handle's geometry at every m, as at m = 0: the smallest frame is 69 columns wide"""
    rc, h = _create_rc(native, W=65, H=9, minDisparity=-32)
    assert rc == ERR_ARG and not h.value
    m = native.StereoSGBM(max_width=69, max_height=9, minDisparity=-32)
    z = native.to_device(np.zeros((9, 65), np.uint8))
    with pytest.raises(native.NativeError):
        m.compute(z, z)
    assert m.sync_errors() == 0
    m.close()
