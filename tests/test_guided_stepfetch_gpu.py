"""The fused guided filter's integer stage 1 fetches its inputs once per STEP of four 4K rows (3 or 4 source rows x 2 columns and
four guide bytes, raw buffer loads at a scalar row offset) and forms 256 p separably.  A band may start on any 4K row, so the
row -> source-row map depends on the parity of the step's first row; these cases take every residue of the band start modulo 4,
a second band of 6 or 2 rows behind a 432-row one, last strips of 6 or 2 columns, partial last steps and images smaller than the
window, and hold the route bit for bit to the f64 stage 1 and, at test_guided_gpu.py's bound, to the f64 oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-3                                   # test_guided_gpu.py's bound
EPS = 1e-3
SIZES = [(115, 219), (113, 217), (9, 10), (3, 2)]          # (Wlo, Hlo): 4K 230 x 438, 226 x 434, 18 x 20, 6 x 4
BANDS = [8, 9, 10, 11, 432]


def _rel_err(got, want):
    scale = np.maximum(np.abs(want), 1e-6 * max(float(np.abs(want).max()), 1e-30))
    return np.abs(got - want) / scale


@functools.lru_cache(maxsize=None)
def _inputs(Wlo, Hlo, n=1):
    """int16 disparities in [-16, 1023], about 20 % of them <= 0, and a random guide"""
    rng = np.random.default_rng(1000 * Wlo + Hlo)
    d = rng.integers(1, 1024, (n, Hlo, Wlo)).astype(np.int16)
    hole = rng.random(d.shape) < 0.2
    d[hole] = rng.integers(-16, 1, int(hole.sum())).astype(np.int16)
    g = rng.integers(0, 256, (n, 2 * Hlo, 2 * Wlo)).astype(np.uint8)
    d.setflags(write=False)
    g.setflags(write=False)
    return d, g


_want = {}


def _oracle(oracle, Wlo, Hlo, r):
    """the f64 reference of a case: computed once, shared, never written"""
    key = (Wlo, Hlo, r)
    if key not in _want:
        d, g = _inputs(Wlo, Hlo)
        w = oracle.guided_upscale(oracle.disp_to_depth(d[0].copy()), g[0].copy(), r, EPS)
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


_got = {}


def _routes(native, Wlo, Hlo, r, band, cols):
    """(f64 stage 1, integer stage 1) of a case on the device, computed once for the two tests that look at it"""
    key = (Wlo, Hlo, r, band, cols)
    if key not in _got:
        d, g = _inputs(Wlo, Hlo)
        dd, gg = native.to_device(d), native.to_device(g)
        try:
            native.set_option("gf_band", band)
            native.set_option("gf_cols", cols)
            native.set_option("gf_int1", 0)
            a = native.guided_upscale_batch(dd, gg, r, EPS)
            native.set_option("gf_int1", 1)
            b = native.guided_upscale_batch(dd, gg, r, EPS)
        finally:
            native.set_option("gf_int1", 1)
            native.set_option("gf_band", 432)
            native.set_option("gf_cols", 256)
        _got[key] = (a[0].cpu(), b[0].cpu())
    return _got[key]


CASES = [(Wlo, Hlo, r, band, cols) for (Wlo, Hlo) in SIZES for r in (4, 8) for band in BANDS for cols in (256, 512)]


@pytest.mark.parametrize("Wlo,Hlo,r,band,cols", CASES)
def test_step_fetch_equals_the_f64_stage1_bit_for_bit(native, Wlo, Hlo, r, band, cols):
    import torch
    a, b = _routes(native, Wlo, Hlo, r, band, cols)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} pixels differ, first at {np.argwhere((a != b).numpy())[:3].tolist()}"


@pytest.mark.parametrize("Wlo,Hlo,r,band,cols", CASES)
def test_step_fetch_matches_the_oracle(native, oracle, Wlo, Hlo, r, band, cols):
    _, b = _routes(native, Wlo, Hlo, r, band, cols)
    want = _oracle(oracle, Wlo, Hlo, r)
    err = _rel_err(b.numpy().astype(np.float64), want)
    print(f"max rel err {err.max():.3e}")
    assert err.max() <= RTOL, f"max rel err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"


@pytest.mark.parametrize("band", [9, 432])
def test_u16_output_kernel_equals_the_float_kernel_rounded(native, oracle, band):
    """The one-pass pipeline's kernel (16-bit samples in and out).  Its stage 1 runs in f64 on every route -- sum g * P of
    16-bit samples does not fit the integer stage's int32, so `gf_int1` does not reach it and there is no integer route to
    compare -- but it shares the run addresses, the single-branch a/b solve and stage 2 with the other instantiations.  It is
    held bit for bit to the float32 kernel on the same samples followed by round_to_u16, and to the oracle within the half
    unit that rounding may add to the float bound."""
    import torch
    Wlo, Hlo, r = 115, 219, 8
    rng = np.random.default_rng(7)
    smp = rng.integers(0, 65536, (1, Hlo, Wlo)).astype(np.uint16)
    g = _inputs(Wlo, Hlo)[1]
    d16, gg = native.to_device(smp.view(np.int16)), native.to_device(g)
    try:
        native.set_option("gf_band", band)
        got = native.guided_upscale_u16_batch(d16, gg, r, EPS)
        ref = native.round_to_u16(native.guided_upscale_batch(native.to_device(smp.astype(np.float32)), gg, r, EPS))
    finally:
        native.set_option("gf_band", 432)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {got.numel()} samples differ"
    want = oracle.guided_upscale(smp[0].astype(np.float32), g[0].copy(), r, EPS)
    q = got[0].cpu().numpy().view(np.uint16).astype(np.float64)
    err = np.abs(q - np.clip(want, 0, 65535))
    bound = RTOL * np.maximum(np.abs(want), 1e-6 * np.abs(want).max()) + 0.5
    print(f"max abs err {err.max():.3f} samples, range {q.min():.0f} .. {q.max():.0f}")
    assert (err <= bound).all() and q.max() > 1000


@pytest.mark.parametrize("band", [9, 432])
def test_strided_batch_at_odd_offsets_equals_single_frames(native, band):
    """three frames, frame strides larger than a frame, base pointers at an odd element offset: each frame as alone"""
    import torch
    Wlo, Hlo, n, r = 113, 217, 3, 8
    W, H = 2 * Wlo, 2 * Hlo
    d, g = _inputs(Wlo, Hlo, n)
    ds, gs = Wlo * Hlo + 37, W * H + 101                       # frame strides (elements, bytes)
    dbuf = torch.full((3 + n * ds,), -7, dtype=torch.int16, device="cuda")
    gbuf = torch.full((5 + n * gs,), 93, dtype=torch.uint8, device="cuda")
    for f in range(n):
        dbuf[3 + f * ds: 3 + f * ds + Wlo * Hlo] = native.to_device(d[f]).reshape(-1)
        gbuf[5 + f * gs: 5 + f * gs + W * H] = native.to_device(g[f]).reshape(-1)
    out = torch.empty((n, H, W), dtype=torch.float32, device="cuda")
    ws = torch.empty((int(native.lib().v3d_guided_upscale_ws_bytes(W, H)) * n,), dtype=torch.uint8, device="cuda")
    assert (dbuf.data_ptr() + 6) % 4 == 2 and (gbuf.data_ptr() + 5) % 2 == 1
    try:
        native.set_option("gf_band", band)
        rc = native.lib().v3d_guided_upscale_disp16_batch(
            C.c_void_p(dbuf.data_ptr() + 6), Wlo, Hlo, ds, C.c_void_p(gbuf.data_ptr() + 5), W, H, gs, n, r, EPS,
            C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, native.lib().v3d_last_error()
        torch.cuda.synchronize()
        for f in range(n):
            alone = native.guided_upscale_batch(native.to_device(d[f:f + 1]), native.to_device(g[f:f + 1]), r, EPS)
            assert torch.equal(out[f], alone[0]), f"frame {f}: {int((out[f] != alone[0]).sum())} pixels differ"
    finally:
        native.set_option("gf_band", 432)
