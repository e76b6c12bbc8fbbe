"""Temporal depth stabilisation on the MI355X: every new entry, the streaming driver and the one-pass pipeline against the
NumPy contract (tests/temporal_ref.py), bit for bit."""
import json

import numpy as np
import pytest
import torch

import launch_plan as LP
import stereo_ref as SR
import temporal_ref as TR
from conftest import mismatch_report

pytestmark = pytest.mark.gpu


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(a, pad):
    """[T,H,W] array -> device tensor whose frames lie `pad` elements further apart than their size"""
    T, H, W = a.shape
    buf = torch.zeros((T, H * W + pad), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    buf[:, :H * W] = _dev(a.reshape(T, H * W))
    return buf[:, :H * W].view(T, H, W)


def _gray_clip(rng, T, H, W, spread=20):
    base = rng.integers(0, 256, (H, W))
    return np.clip(base[None] + rng.integers(-spread, spread + 1, (T, H, W)), 0, 255).astype(np.uint8)


def _depth_clip(rng, T, H, W, kind):
    if kind == "stereo":                                  # multiples of 1/16 like the matcher's, invalid = 0
        d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
        d[rng.random((T, H, W)) < 0.2] = 0.0
    elif kind == "blend":                                 # non-integer floats like the hybrid blend
        d = rng.uniform(0.0, 64.0, (T, H, W)).astype(np.float32)
        d[rng.random((T, H, W)) < 0.1] = 0.0
    elif kind == "full":                                  # the whole d16 range 0..32767
        d = (rng.integers(0, 32768, (T, H, W)) / 16.0).astype(np.float32)
    else:                                                 # "holes": whole frames invalid
        d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
        d[::2] = 0.0
        d[1::4] = -1.0
    return d


def _check_filter(native, depth, gray, R, tau, cut, fill, t0=0, n=None, pad=(0, 0), what=""):
    d = _strided(depth, pad[0]) if pad[0] else _dev(depth)
    g = _strided(gray, pad[1]) if pad[1] else _dev(gray)
    got = native.temporal_filter_batch(d, g, R, tau, _dev(cut), fill, t0, n).cpu().numpy()
    want = TR.filter_clip(depth, gray, R, tau, cut, fill, t0, n)
    # the outputs are exact multiples of 1/16: compare the integers
    rep = mismatch_report((got * 16).astype(np.int64), (want * 16).astype(np.int64), what)
    assert not rep and np.array_equal(got, want), rep


# ---------------------------------------------------------------- cuts, min/max, range, normalisation

@pytest.mark.timeout(300)
def test_cuts(native):
    rng = np.random.default_rng(0)
    for (T, H, W, pad) in ((1, 1, 1, 0), (2, 1, 1, 0), (5, 3, 2, 0), (7, 33, 257, 0), (6, 33, 257, 7), (4, 64, 256, 16), (9, 270, 480, 0)):
        g = _gray_clip(rng, T, H, W, spread=12)
        if T > 3:
            g[T // 2:] = 255 - g[T // 2:]                 # a real scene change
        gd = _strided(g, pad) if pad else _dev(g)
        for c in (0, 5, 20, 256):
            got = native.temporal_cuts(gd, c).cpu().numpy()
            assert not mismatch_report(got, TR.cuts(g, c), f"cuts {T}x{H}x{W} pad {pad} c={c}")
    # frames that differ in one pixel around the threshold: mean difference exactly c is no cut, one level more is
    for (H, W) in ((4, 5), (33, 257), (128, 256)):
        g = np.zeros((4, H, W), np.uint8)
        g[1:] = 20
        g[2, H // 2, W // 3] = 21
        g[3, H // 2, W // 3] = 21
        g[3, 0, 0] = 19
        for c in (19, 20, 21):
            assert not mismatch_report(native.temporal_cuts(_dev(g), c).cpu().numpy(), TR.cuts(g, c), f"one pixel {H}x{W} c={c}")
        g[1, -1, -1] = 21
        assert list(native.temporal_cuts(_dev(g), 20).cpu().numpy()) == list(TR.cuts(g, 20)) == [0, 1, 0, 0]


def test_cuts_where_a_lane_strides(native):
    """LP.CUTS_CASE (tests/test_launch_plan_host.py holds its regime): 66 frames, so 32 workgroups a pair, of 515 x 255: a lane's
    second step in the 16-byte loop when the clip is aligned (frames 3 elements apart: a stride of 16 k), 17 steps in the byte
    loop when it is not (dense: 131 325 = 13 mod 16).  Every pair differs by 20 in every pixel, so a pixel left out or read twice
    moves the pair across the threshold of 20; single pixels one level off sit in the 16-byte loop's first and second step, in
    its 13-pixel tail and at both ends"""
    T, W, H = LP.CUTS_CASE
    g = np.zeros((T, H, W), np.uint8)
    g[1::2] = 20
    flat = g.reshape(T, -1)
    flat[5, 16 * 8192 + 7] = flat[11, -1] = flat[21, 0] = flat[41, 70001] = 21
    flat[31, 16 * 8200 + 3] = flat[51, -13] = 19
    want = {c: TR.cuts(g, c) for c in (19, 20, 21)}
    assert want[20].sum() == 8 and want[19].sum() == T - 1 and want[21].sum() == 0
    rng = np.random.default_rng(66)
    noisy = _gray_clip(rng, T, H, W, spread=12)
    noisy[40:] = 255 - noisy[40:]
    for pad in (3, 0):
        gd = _strided(g, pad) if pad else _dev(g)
        assert (gd.data_ptr() % 16 == 0 and gd.stride(0) % 16 == 0) == (pad == 3)
        for c in (19, 20, 21):
            assert not mismatch_report(native.temporal_cuts(gd, c).cpu().numpy(), want[c], f"strided grid pad {pad} c={c}")
        nd = _strided(noisy, pad) if pad else _dev(noisy)
        assert not mismatch_report(native.temporal_cuts(nd, 20).cpu().numpy(), TR.cuts(noisy, 20), f"scene change pad {pad}")


@pytest.mark.timeout(300)
def test_minmax_and_range(native):
    rng = np.random.default_rng(1)
    for (T, H, W, pad) in ((1, 1, 1, 0), (3, 2, 3, 0), (12, 33, 257, 5), (20, 135, 240, 0)):
        d = (rng.random((T, H, W)) * rng.choice([1e-3, 1, 3e3], (T, 1, 1))).astype(np.float32)
        d[T // 2] = -2.5
        dd = _strided(d, pad) if pad else _dev(d)
        mm = native.depth_minmax_batch(dd)
        want_mm = TR.minmax(d)
        assert np.array_equal(mm.cpu().numpy(), want_mm)
        for R in (0, 1, 2, 4, 8):
            for trial in range(3):
                cut = (rng.random(T) < (0, 0.2, 0.6)[trial]).astype(np.uint8)
                cut[0] = 0
                t0 = int(rng.integers(0, T))
                n = int(rng.integers(1, T - t0 + 1))
                got = native.temporal_range(mm, _dev(cut), R, t0, n).cpu().numpy()
                assert np.array_equal(got, TR.ranges(want_mm, cut, R, t0, n)), (T, R, trial)


@pytest.mark.timeout(300)
def test_range_normalisation(native, oracle):
    rng = np.random.default_rng(2)
    # the last: LP.RANGE_FLOOR_CASE, 64 blocks a frame (the floor) for the 127 its elements fill, in k_minmax and k_norm_u16 alike
    for (n, H, W, pad) in ((1, 1, 1, 0), (4, 7, 255, 0), (5, 131, 257, 3), (3, 1080, 1920, 0), LP.RANGE_FLOOR_CASE + (0,)):
        d = (rng.random((n, H, W)) * 64).astype(np.float32)
        if n > 2:
            d[1] = 7.25                                     # constant frame -> 0
        dd = _strided(d, pad) if pad else _dev(d)
        own = native.depth_minmax_batch(dd)
        got = _u16(native.depth_to_u16_range_batch(dd, own))
        assert np.array_equal(got, _u16(native.depth_to_u16_batch(_dev(d))))           # own range == the per-frame entry's bits
        assert np.array_equal(got, np.stack([oracle.depth_to_u16(f) for f in d]))
        if n > 2:
            assert not got[1].any()
        lohi = np.stack([d.min(axis=(1, 2)) + 3.0, d.max(axis=(1, 2)) - 5.0], axis=1).astype(np.float32)   # values outside: clamped
        lohi[0] = (2.0, 2.0)                                                             # hi == lo -> 0
        got = _u16(native.depth_to_u16_range_batch(dd, _dev(lohi)))
        assert not mismatch_report(got, TR.to_u16_range(d, lohi), f"range {n}x{H}x{W}")


# ---------------------------------------------------------------- the filter

@pytest.mark.timeout(900)
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (63, 5), (257, 33), (256, 32), (1000, 9)])
def test_filter_small_sizes(native, size):
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    i = 0
    for R in (0, 1, 2, 4, 8):
        for T in sorted({1, 2, R + 1, 2 * R + 1, 2 * R + 4}):
            for kind in ("stereo", "blend", "full", "holes"):
                tau, fill = (1, 12, 255)[i % 3], (i // 3) % 2
                i += 1
                depth, gray = _depth_clip(rng, T, H, W, kind), _gray_clip(rng, T, H, W, spread=(3, 20, 120)[i % 3])
                cut = (rng.random(T) < 0.25).astype(np.uint8)
                cut[0] = 0
                _check_filter(native, depth, gray, R, tau, cut, fill, what=f"{W}x{H} T={T} R={R} tau={tau} fill={fill} {kind}")


@pytest.mark.timeout(600)
def test_filter_cuts_at_every_position_targets_and_strides(native):
    rng = np.random.default_rng(7)
    W, H, R = 260, 12, 2
    T = 2 * R + 4
    depth, gray = _depth_clip(rng, T, H, W, "stereo"), _gray_clip(rng, T, H, W)
    for pos in range(1, T):
        cut = np.zeros(T, np.uint8)
        cut[pos] = 1
        _check_filter(native, depth, gray, R, 12, cut, 1, what=f"cut at {pos}")
    cut = np.zeros(T, np.uint8)
    cut[1::2] = 1
    _check_filter(native, depth, gray, 8, 12, cut, 1, what="cuts at every other frame")
    _check_filter(native, depth, gray, 8, 12, np.r_[0, np.ones(T - 1)].astype(np.uint8), 0, what="cuts everywhere")
    cut = np.zeros(T, np.uint8)
    cut[3] = 1
    for (t0, n) in ((0, 1), (T - 1, 1), (2, 3), (1, T - 1), (3, 2)):
        for pad in ((0, 0), (4, 4), (1, 3), (8, 0), (0, 5)):           # dense, vector-friendly and odd frame strides
            _check_filter(native, depth, gray, R, 12, cut, 1, t0, n, pad, what=f"targets {t0}+{n} pad {pad}")
    # a width the vector path takes, unaligned only through the view's offset
    buf = torch.zeros(T * H * 256 + 1, dtype=torch.uint8, device="cuda")
    g = _gray_clip(rng, T, H, 256)
    d = _depth_clip(rng, T, H, 256, "blend")
    buf[1:] = _dev(g.reshape(-1))
    got = native.temporal_filter_batch(_dev(d), buf[1:].view(T, H, 256), R, 12, _dev(cut), 1).cpu().numpy()
    assert np.array_equal(got, TR.filter_clip(d, g, R, 12, cut, 1))


@pytest.mark.timeout(900)
def test_filter_1080p(native):
    rng = np.random.default_rng(8)
    W, H, T = 1920, 1080, 6
    for (R, kind, tau, fill, t0, n) in ((2, "stereo", 12, 1, 0, 6), (4, "blend", 12, 0, 2, 2), (8, "full", 255, 1, 5, 1)):
        depth, gray = _depth_clip(rng, T, H, W, kind), _gray_clip(rng, T, H, W, spread=8)
        cut = np.zeros(T, np.uint8)
        cut[4] = 1
        _check_filter(native, depth, gray, R, tau, cut, fill, t0, n, what=f"1080p R={R} {kind}")


def _matched_clip(native, W, H, T, **kw):
    """the synthetic clip through the GPU matcher -> (depth f32 [T,H,W], left gray u8 [T,H,W]) as NumPy"""
    from video_3d_pipeline import synthetic as syn
    L, Rr, _ = syn.temporal_clip(W, H, T, **kw)
    m = native.StereoSGBM(W, H, T)
    depth = native.disp_to_depth(m.compute(_dev(L), _dev(Rr))).cpu().numpy()
    m.close()
    return depth, L


@pytest.mark.timeout(600)
def test_filter_and_stage_on_matcher_output(native):
    depth, gray = _matched_clip(native, 320, 120, 9, cut_at=5)
    assert (depth > 0).mean() > 0.5
    cut = TR.cuts(gray, 20)
    assert list(cut) == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(native.temporal_cuts(_dev(gray), 20).cpu().numpy(), cut)
    for R in (1, 2, 4):
        _check_filter(native, depth, gray, R, 12, cut, 1, what=f"matcher output R={R}")
    _check_filter(native, depth, gray, 2, 12, cut, 0, what="matcher output, no fill")


# ---------------------------------------------------------------- the streaming driver and the pipeline

@pytest.mark.timeout(600)
def test_streaming_driver_equals_one_whole_clip_call(native):
    from video_3d_pipeline.depth import HipStereoBackend
    from video_3d_pipeline.temporal import TemporalStabilizer
    be = HipStereoBackend()
    depth, gray = _matched_clip(native, 320, 64, 11, cut_at=6)
    dd, gd = _dev(depth), _dev(gray)
    for R in (1, 2, 8):
        want = TR.stabilize(depth, gray, R)
        whole = _u16(be.temporal_stabilize(dd, gd, 0, len(depth), R, 12, 20, True))
        assert not mismatch_report(whole, want, f"whole clip R={R}")
        for step in (1, 2, 3, 5, 11):
            st = TemporalStabilizer(be, R)
            parts = []
            for i in range(0, len(depth), step):
                staging_d, staging_g = dd[i:i + step].clone(), gd[i:i + step].clone()
                out = st.push(staging_d, staging_g)
                staging_d.zero_()                          # the driver must have copied what it keeps
                staging_g.zero_()
                if out is not None:
                    parts.append(_u16(out))
            out = st.finish()
            if out is not None:
                parts.append(_u16(out))
            assert np.array_equal(np.concatenate(parts), want), (R, step)


@pytest.mark.timeout(900)
def test_pipeline_with_temporal_radius_and_stereo_output(native, tmp_path):
    """one-pass pipeline, --temporal-radius 2 --stereo-output: the 1080p-side u16 maps equal the NumPy reference on the
    backend's own per-frame depth and left gray; the 4K maps equal the existing guided entry on those samples; the 3D frames
    equal tests/stereo_ref.py on the 4K frames and 4K maps"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend, SbsTo4kDepthPipeline
    from video_3d_pipeline.utils import iter_frames, read_png16
    SW, SH, T = 384, 96, 9
    sbs = syn.temporal_sbs_clip(SW, SH, T, cut_at=5)
    rng = np.random.default_rng(4)
    v4k = rng.integers(0, 256, (T, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)

    be = HipPipelineBackend()
    depth = be.sbs_to_disparity(list(sbs), True).cpu().numpy()
    gray = be.left_gray(T).cpu().numpy()
    want_lo = TR.stabilize(depth, gray, 2)
    assert TR.cuts(gray, 20)[5] == 1
    luma = be.guide_luma(list(v4k), 2 * SH, 2 * SW, T)
    want_hi = _u16(native.guided_upscale_u16_batch(_dev(want_lo.view(np.int16)), luma, 8, 1e-3))
    gains = SR.stereo_gains()

    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w"), batch_size=4, stereo_only=True, guide_batch=3, temporal_radius=2)
    out = pipe.run(str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), output_path=str(tmp_path / "d.json"), keep_depth_maps=True,
                   stereo_output=str(tmp_path / "s.json"))
    man = json.loads(open(out).read())
    assert man["count"] == T and man["temporal"] == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True}
    cache = pipe.extractor.get_cache_path(str(tmp_path / "sbs.npy"), 0, T)
    sman = json.loads((tmp_path / "s.json").read_text())
    got3d = list(iter_frames(sman["frames_dir"]))
    assert sman["count"] == T == len(got3d)
    for i in range(T):
        assert not mismatch_report(read_png16(cache / f"depth_{i:06d}.png"), want_lo[i], f"1080p-side map {i}")
        assert not mismatch_report(read_png16(f"{man['frames_dir']}/depth4k_{i:06d}.png"), want_hi[i], f"4K map {i}")
        assert np.array_equal(got3d[i], SR.render(v4k[i], want_hi[i], *gains, SR.FULL_SBS)), i
    # and with the stage off the same call writes what it always wrote: other bytes than with it on
    off = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w0"), batch_size=4, stereo_only=True, guide_batch=3)
    man0 = json.loads(open(off.run(str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), output_path=str(tmp_path / "d0.json"))).read())
    assert "temporal" not in man0
    per_frame = np.stack([read_png16(f"{man0['frames_dir']}/depth4k_{i:06d}.png") for i in range(T)])
    assert (per_frame != want_hi).any()
