"""Robust depth range on the MI355X: v3d_depth_robust_minmax_batch, its chain into the existing range and normalisation entries,
the streaming driver and the one-pass pipeline against the NumPy contract (tests/range_ref.py), bit for bit."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import range_ref as RR
import stereo_ref as SR
import temporal_ref as TR
from conftest import mismatch_report

pytestmark = pytest.mark.gpu

QS = (5000, 9000, 9800, 9999, 10000)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _view(a, pad=0, offset=0):
    """[T,H,W] float32 array -> device view whose frames lie `pad` elements further apart than their size and whose first
    element sits `offset` elements (4 bytes each) behind a 16-byte boundary"""
    T, H, W = a.shape
    buf = torch.zeros(offset + T * (H * W + pad), dtype=torch.float32, device="cuda")
    v = torch.as_strided(buf, (T, H, W), (H * W + pad, W, 1), offset)
    v.copy_(_dev(a))
    return v


def _check(native, d, what, pad=0, offset=0, qs=QS):
    dd = _view(d, pad, offset)
    assert dd.data_ptr() % 16 == (4 * offset) % 16
    for q in qs:
        got = native.depth_robust_minmax_batch(dd, q).cpu().numpy()
        want = RR.robust_minmax(d, q)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want), f"{what} pad {pad} offset {offset} q {q}: got {got[got != want][:4]} want {want[got != want][:4]}"
        for t in range(len(d)):                                # at most n_valid - k valid pixels above the frame's own hi
            n_valid, k, _ = RR.select(RR.histogram(d[t]), q)
            assert RR.above(d[t], got[t, 1]) <= n_valid - k


def _clip(rng, T, H, W, kind):
    if kind == "stereo":                                  # multiples of 1/16 like the matcher's, a fifth invalid, a few outliers
        d = (rng.integers(16, 700, (T, H, W)) / 16.0).astype(np.float32)
        d[rng.random((T, H, W)) < 0.2] = 0.0
        d[rng.random((T, H, W)) < 0.002] = np.float32(60.5)
    elif kind == "smooth":                                # piecewise smooth: neighbouring pixels share their bin
        x = np.linspace(4, 60, W, dtype=np.float32)[None, None, :] + np.arange(T, dtype=np.float32)[:, None, None] * 0.25
        d = (np.rint((x + np.zeros((T, H, W), np.float32)) * 16) / 16).astype(np.float32)
        d[:, : max(H // 5, 1)] = 0.0
    elif kind == "blend":                                 # non-integer floats like the hybrid blend, some negative
        d = rng.uniform(-1.0, 64.0, (T, H, W)).astype(np.float32)
    elif kind == "saturating":                            # d16 up to 3200 and beyond: the last bin
        d = (rng.integers(0, 4096, (T, H, W)) / 16.0).astype(np.float32)
        d[0] = 200.0
    else:                                                 # "holes": whole frames invalid
        d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
        d[::2] = 0.0
        d[1::4] = -1.0
    return d


# ---------------------------------------------------------------- the entry

@pytest.mark.timeout(900)
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (5, 7), (63, 5), (257, 33), (256, 32), (1000, 9), (480, 270)])
def test_entry_small_sizes_strides_and_misaligned_views(native, size):
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    for T in (1, 2, 5, 34):
        if T == 34 and W * H > 10000:
            continue
        for kind in ("stereo", "smooth", "blend", "saturating", "holes"):
            d = _clip(rng, T, H, W, kind)
            _check(native, d, f"{W}x{H} T={T} {kind}")
            _check(native, d, f"{W}x{H} T={T} {kind}", pad=4, qs=(9800,))            # vector-friendly stride
            _check(native, d, f"{W}x{H} T={T} {kind}", pad=5, qs=(9800,))            # odd stride: element-wise
            _check(native, d, f"{W}x{H} T={T} {kind}", offset=1, qs=(9000, 10000))   # 4-byte-misaligned base: element-wise
            _check(native, d, f"{W}x{H} T={T} {kind}", pad=3, offset=3, qs=(9800,))


@pytest.mark.timeout(900)
def test_entry_1080p_batches(native):
    rng = np.random.default_rng(11)
    W, H = 1920, 1080
    _check(native, _clip(rng, 34, H, W, "stereo"), "1080p x 34 stereo", qs=(9800, 10000))
    _check(native, _clip(rng, 3, H, W, "smooth"), "1080p x 3 smooth")
    _check(native, _clip(rng, 2, H, W, "blend"), "1080p x 2 blend", qs=(5000, 9999))
    _check(native, _clip(rng, 2, H, W, "stereo"), "1080p x 2 misaligned", offset=2, qs=(9800,))
    _check(native, _clip(rng, 1, H, W + 1, "stereo"), "1921x1080: n & 3 != 0", qs=(9800,))


@pytest.mark.timeout(600)
def test_constant_all_invalid_and_saturating_frames(native):
    W, H = 1920, 1080
    d = np.empty((6, H, W), np.float32)
    d[0] = 7.25                      # constant: every lane of every wave adds to one bin
    d[1] = 0.0                       # all invalid
    d[2] = -3.0
    d[3] = 200.0                     # every pixel saturates
    d[4] = 7.26                      # one bin whose value lies below the min: hi = mn
    d[5] = 0.0
    d[5, 500, 600] = 33.0            # one valid pixel
    _check(native, d, "constant / invalid / saturating 1080p")
    got = native.depth_robust_minmax_batch(_dev(d), 9800).cpu().numpy()
    assert np.array_equal(got, np.float32([[7.25, 7.25], [0.0, 0.0], [-3.0, -3.0], [200.0, 200.0], [7.26, 7.26], [0.0, 33.0]]))
    u = _u16(native.depth_to_u16_range_batch(_dev(d), native.depth_robust_minmax_batch(_dev(d), 9800)))
    assert not u[:5].any() and u[5].sum() == 65535 and u[5, 500, 600] == 65535


@pytest.mark.timeout(300)
def test_off_returns_the_maximum_on_fixed_point_depths(native):
    rng = np.random.default_rng(12)
    d = (rng.integers(0, 2047, (5, 131, 257)) / 16.0).astype(np.float32)
    d[0, 0, 0] = 2046 / 16.0
    dd = _dev(d)
    got = native.depth_robust_minmax_batch(dd, 10000)
    assert np.array_equal(got.cpu().numpy(), native.depth_minmax_batch(dd).cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), TR.minmax(d))


@pytest.mark.parametrize("shape,pad", [((3, 5, 67), 0), ((2, 33, 257), 5)])
def test_mixed_sign_frames_one_range_and_one_sample_on_every_route(native, oracle, shape, pad):
    """frames whose values change sign (multiples of 1/16 in [-40, 40], so the histogram's white point at q = 10000 IS the
    maximum): the three reductions -- v3d_depth_minmax_batch, v3d_depth_robust_minmax_batch and the one inside
    v3d_depth_to_u16_batch -- give NumPy's per-frame min and max, and the u16 samples are the same bits whichever supplies the
    range.  Frame pad 5 makes the stride odd: the element-wise instantiation of the histogram kernel."""
    rng = np.random.default_rng(shape[2])
    d = (rng.integers(-640, 641, shape) / 16.0).astype(np.float32)
    want_mm = np.stack([d.reshape(shape[0], -1).min(axis=1), d.reshape(shape[0], -1).max(axis=1)], axis=1)
    assert (want_mm[:, 0] < 0).all() and (want_mm[:, 1] > 0).all()
    dd = _view(d, pad)
    assert dd.stride(0) == shape[1] * shape[2] + pad
    mm, rmm = native.depth_minmax_batch(dd), native.depth_robust_minmax_batch(dd, 10000)
    assert np.array_equal(mm.cpu().numpy(), want_mm)
    assert np.array_equal(rmm.cpu().numpy(), want_mm)
    want = np.stack([oracle.depth_to_u16(f) for f in d])                     # the oracle reduces its own min and max
    out = torch.empty(shape, dtype=torch.int16, device="cuda")                # the C entry itself: the binding takes dense clips only
    ws = torch.empty(2 * shape[0], dtype=torch.float32, device="cuda")
    assert native.lib().v3d_depth_to_u16_batch(C.c_void_p(dd.data_ptr()), shape[0], C.c_size_t(shape[1] * shape[2]), C.c_size_t(dd.stride(0)),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(0)) == 0
    own = _u16(out)
    assert np.array_equal(own, _u16(native.depth_to_u16_batch(dd.contiguous())))
    assert not mismatch_report(own, want, f"own range {shape}")
    assert not mismatch_report(_u16(native.depth_to_u16_range_batch(dd, mm)), want, f"min/max entry's range {shape} pad {pad}")
    assert not mismatch_report(_u16(native.depth_to_u16_range_batch(dd, rmm)), want, f"histogram entry's range {shape} pad {pad}")
    assert np.array_equal(want, TR.to_u16_range(d, want_mm))


def _matched_clip(native, W, H, T, **kw):
    """the synthetic clip through the GPU matcher -> (depth f32 [T,H,W], left gray u8 [T,H,W]) as NumPy"""
    from video_3d_pipeline import synthetic as syn
    L, Rr, _ = syn.temporal_clip(W, H, T, **kw)
    m = native.StereoSGBM(W, H, T)
    depth = native.disp_to_depth(m.compute(_dev(L), _dev(Rr))).cpu().numpy()
    m.close()
    return depth, L


@pytest.mark.timeout(600)
def test_matcher_output_and_the_chain_into_range_and_normalisation(native):
    depth, gray = _matched_clip(native, 320, 120, 9, cut_at=5)
    assert (depth > 0).mean() > 0.5
    _check(native, depth, "matcher output")
    dd = _dev(depth)
    cut = TR.cuts(gray, 20)
    for q in QS:
        mm = native.depth_robust_minmax_batch(dd, q)
        want_mm = RR.robust_minmax(depth, q)
        # radius 0: every frame against its own robust range
        assert not mismatch_report(_u16(native.depth_to_u16_range_batch(dd, mm)), RR.to_u16(depth, q), f"own range q={q}")
        for R in (1, 2, 8):
            lohi = native.temporal_range(mm, _dev(cut), R)
            assert np.array_equal(lohi.cpu().numpy(), TR.ranges(want_mm, cut, R))
            filt = native.temporal_filter_batch(dd, _dev(gray), R, 12, _dev(cut), True)
            assert not mismatch_report(_u16(native.depth_to_u16_range_batch(filt, lohi)), RR.stabilize(depth, gray, R, q=q), f"chain R={R} q={q}")
    # off: the matcher's depths are multiples of 1/16 below 2047/16, so the samples are the per-frame entry's
    assert np.array_equal(_u16(native.depth_to_u16_range_batch(dd, native.depth_robust_minmax_batch(dd, 10000))), _u16(native.depth_to_u16_batch(dd)))
    # and on, the 98th percentile moves the white point of this clip
    assert (RR.robust_minmax(depth, 9800)[:, 1] < TR.minmax(depth)[:, 1]).any()


def test_bad_arguments_are_refused(native):
    lib = native.lib()
    d = torch.zeros((2, 4, 8), dtype=torch.float32, device="cuda")
    ws = torch.zeros(lib.v3d_depth_robust_minmax_ws_bytes(2) + 16, dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    assert lib.v3d_depth_robust_minmax_ws_bytes(0) == 0 and lib.v3d_depth_robust_minmax_ws_bytes(34) == 34 * (2048 + 2) * 4
    p, w, o, st = C.c_void_p(d.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(0)

    def call(depth=p, T=2, n=32, stride=32, q=9800, wsp=w, outp=o):
        return lib.v3d_depth_robust_minmax_batch(depth, T, n, stride, q, wsp, outp, st)

    assert call() == 0
    for kw in (dict(depth=None), dict(wsp=None), dict(outp=None), dict(T=0), dict(T=65536), dict(n=0), dict(q=4999), dict(q=10001),
               dict(stride=31), dict(wsp=C.c_void_p(ws.data_ptr() + 4))):
        assert call(**kw) == -1, kw
        assert lib.v3d_last_error()
    torch.cuda.synchronize()
    for bad in (4999, 10001, 98.5, True):
        with pytest.raises(ValueError):
            native.depth_robust_minmax_batch(d, bad)


# ---------------------------------------------------------------- the streaming driver and the pipeline

@pytest.mark.timeout(600)
def test_streaming_driver_equals_one_whole_clip_call(native):
    from video_3d_pipeline.depth import HipStereoBackend
    from video_3d_pipeline.temporal import TemporalStabilizer
    be = HipStereoBackend()
    depth, gray = _matched_clip(native, 320, 64, 11, cut_at=6)
    dd, gd = _dev(depth), _dev(gray)
    q = 9800
    assert not mismatch_report(_u16(be.depth_to_u16_robust(dd, q)), RR.to_u16(depth, q), "radius 0 backend method")
    for R in (1, 2, 8):
        want = RR.stabilize(depth, gray, R, q=q)
        whole = _u16(be.temporal_stabilize(dd, gd, 0, len(depth), R, 12, 20, True, q))
        assert not mismatch_report(whole, want, f"whole clip R={R}")
        assert np.array_equal(_u16(be.temporal_stabilize(dd, gd, 0, len(depth), R, 12, 20, True)), TR.stabilize(depth, gray, R))
        for step in (1, 2, 3, 5, 11):
            st = TemporalStabilizer(be, R, range_quantile=q)
            parts = []
            for i in range(0, len(depth), step):
                staging_d, staging_g = dd[i:i + step].clone(), gd[i:i + step].clone()
                out = st.push(staging_d, staging_g)
                staging_d.zero_()
                staging_g.zero_()
                if out is not None:
                    parts.append(_u16(out))
            out = st.finish()
            if out is not None:
                parts.append(_u16(out))
            assert np.array_equal(np.concatenate(parts), want), (R, step)


@pytest.mark.timeout(900)
def test_pipeline_with_temporal_radius_range_percentile_and_stereo_output(native, tmp_path):
    """one-pass pipeline, --temporal-radius 2 --range-percentile 98 --stereo-output: the 1080p-side u16 maps equal the NumPy
    contract on the backend's own per-frame depth and left gray; the 4K maps equal the existing guided entry on those samples;
    the 3D frames equal tests/stereo_ref.py on the 4K frames and 4K maps.  Then --range-percentile 98 alone (radius 0), and the
    depth CLI's files for both."""
    from video_3d_pipeline import pipeline as pipe_mod, synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.pipeline import HipPipelineBackend
    from video_3d_pipeline.utils import iter_frames, read_png16
    SW, SH, T = 384, 96, 9
    sbs = syn.temporal_sbs_clip(SW, SH, T, cut_at=5)
    rng = np.random.default_rng(4)
    v4k = rng.integers(0, 256, (T, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)
    sbs_p, v4k_p = str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy")

    be = HipPipelineBackend()
    depth = be.sbs_to_disparity(list(sbs), True).cpu().numpy()
    gray = be.left_gray(T).cpu().numpy()
    luma = be.guide_luma(list(v4k), 2 * SH, 2 * SW, T)
    gains = SR.stereo_gains()
    assert (RR.robust_minmax(depth, 9800)[:, 1] < TR.minmax(depth)[:, 1]).any()

    for R in (2, 0):
        want_lo = RR.stabilize(depth, gray, R, q=9800) if R else RR.to_u16(depth, 9800)
        assert (want_lo != (TR.stabilize(depth, gray, R) if R else TR.to_u16_range(depth, TR.minmax(depth)))).any()
        want_hi = _u16(native.guided_upscale_u16_batch(_dev(want_lo.view(np.int16)), luma, 8, 1e-3))
        # through the command line: the flags reach the run
        argv = [sbs_p, v4k_p, "--work-dir", str(tmp_path / f"w{R}"), "--batch-size", "4", "--stereo-only", "--output", str(tmp_path / f"d{R}.json"),
                "--keep-depth-maps", "--stereo-output", str(tmp_path / f"s{R}.json"), "--temporal-radius", str(R), "--range-percentile", "98"]
        assert pipe_mod.main(argv) == 0
        man = json.loads((tmp_path / f"d{R}.json").read_text())
        entry = {"radius": R, "tau": 12, "cut_threshold": 20, "fill": True, "range_quantile": 9800}
        assert man["count"] == T and man["temporal"] == entry
        ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / f"w{R}"), cache_dir=str(tmp_path / f"w{R}"), batch_size=4, stereo_only=True,
                                        temporal_radius=R, range_percentile=98)
        cache = ex.get_cache_path(sbs_p, 0, T)
        assert json.loads((cache / "temporal.json").read_text()) == entry
        sman = json.loads((tmp_path / f"s{R}.json").read_text())
        got3d = list(iter_frames(sman["frames_dir"]))
        assert sman["count"] == T == len(got3d)
        for i in range(T):
            assert not mismatch_report(read_png16(cache / f"depth_{i:06d}.png"), want_lo[i], f"R={R} 1080p-side map {i}")
            assert not mismatch_report(read_png16(f"{man['frames_dir']}/depth4k_{i:06d}.png"), want_hi[i], f"R={R} 4K map {i}")
            assert np.array_equal(got3d[i], SR.render(v4k[i], want_hi[i], *gains, SR.FULL_SBS)), (R, i)
        # the depth CLI writes the same 1080p-side maps
        ddir = ex.process_video_sbs(sbs_p, force_reprocess=True)
        assert ddir == cache
        for i in range(T):
            assert not mismatch_report(read_png16(ddir / f"depth_{i:06d}.png"), want_lo[i], f"R={R} depth CLI map {i}")
