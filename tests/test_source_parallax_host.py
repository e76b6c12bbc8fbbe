"""Host logic of source-faithful 3D on the CPU: --depth-range metric of the depth CLI and the one-pass pipeline, --parallax source
and --fill-from-source of the convert step.  Stand-in backends over the NumPy contracts take the place of the HIP ones, as in
tests/test_convert_pack_host.py; test_source_parallax_quality is the experiment of DESIGN.md §4, "Source-faithful 3D", done with
the references."""
import json
import math

import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_ref as R
import stereo_source_ref as X
import temporal_ref as TR
from test_convert_host import H4, W4, RefStereoPipelineBackend, _pngs, _read_clip, inputs, sbs_clips  # noqa: F401
from test_host import OracleStereoBackend, OracleUpscaleBackend
from test_pipeline_host import SW, SH


class MetricStereoBackend(OracleStereoBackend):
    """the depth stand-in plus the metric normalisation; every range-related call is recorded"""

    def __init__(self):
        self.calls = []

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None, fill_holes=False, min_disparity=0):
        return super().sbs_to_disparity(frames, unsqueeze, mono_provider)      # the depth itself is not what these tests look at

    def depth_to_u16_batch(self, depth):
        self.calls.append("minmax")
        return super().depth_to_u16_batch(depth)

    def depth_to_u16_robust(self, depth, q):
        self.calls.append("robust")
        raise AssertionError("no robust range in these tests")

    def depth_to_u16_metric(self, depth):
        self.calls.append("metric")
        d = np.asarray(depth, np.float32)
        return TR.to_u16_range(d, np.tile(np.array([[0, 64]], np.float32), (len(d), 1)))

    def left_gray(self, n):
        return np.zeros((n, SH, SW), np.uint8)

    def temporal_concat(self, held, new):
        return np.array(new) if held is None else np.concatenate([held, new])

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill, range_quantile=10000, metric=False):
        self.calls.append(("stabilize", bool(metric)))
        cut = TR.cuts(gray, cut_threshold)
        filt = TR.filter_clip(depth, gray, radius, tau, cut, fill, t0, n)
        if metric:
            return TR.to_u16_range(filt, np.tile(np.array([[0, 64]], np.float32), (n, 1)))
        self.calls.append("range")
        return TR.to_u16_range(filt, TR.ranges(TR.minmax(np.asarray(depth, np.float32).reshape(len(depth), -1)), cut, radius, t0, n))


class MetricPipelineBackend(RefStereoPipelineBackend, MetricStereoBackend):
    def __init__(self):
        RefStereoPipelineBackend.__init__(self)
        MetricStereoBackend.__init__(self)


class SourceRenderBackend:
    """test-only stand-in for convert.HipRenderBackend over tests/stereo_source_ref.py; records the calls' source keyword"""

    def __init__(self):
        self.calls = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        self.calls.append(None if source is None else (len(source["frames"]), source["fill_eyes"], tuple(source["q"])))
        if source is None:
            return np.stack([P.render(f, d, gain_left, gain_right, conv, layout, subpixel) for f, d in zip(frames, depths)])
        return np.stack([X.render(f, d, gain_left, gain_right, conv, layout, subpixel, s, source["fill_eyes"], *source["q"])
                         for f, d, s in zip(frames, depths, source["frames"])])


def _extractor(tmp, tag, backend=None, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp / f"d_{tag}")
    return HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True,
                                      backend=backend or MetricStereoBackend(), **kw)


def _convert(args, backend):
    from video_3d_pipeline import convert
    return convert.main([str(a) for a in args], backend=backend)


# ------------------------------------------------------------------------------------------------------------------------
# the gains
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, -32, -64])
@pytest.mark.parametrize("num,den", [(1, 1), (2, 1), (3840, 1856)])
@pytest.mark.parametrize("K", [1.0, 0.5, 2.0])
def test_gains_give_the_films_parallax(m, num, den, K):
    """eye_split 0, max_shift = K s 64 65536 / 65535, convergence = -m / 64 through stereo_gains: a sample v = 65535 r / 64 (rebiased
    disparity r = d - m) then moves by round(K s d) to within the rounding of the gain and of the sample"""
    from video_3d_pipeline._native import stereo_gains
    from video_3d_pipeline.convert import source_parallax
    W_eye = 1856 if den != 1 else 960
    Whi = W_eye * num // den
    s = Whi / W_eye
    p = source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": m, "eye_width": W_eye}, Whi, None, K)
    assert p["eye_split"] == 0 and p["scale"] == s and p["gain"] == K
    assert p["max_shift"] == K * s * 64 * 65536 / 65535 and p["convergence"] == -m / 64
    gl, gr, conv = stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    assert gl == 0 and gr == -math.floor(p["max_shift"] * 256 + 0.5) and conv == math.floor(-m / 64 * 65535 + 0.5)
    assert abs(gr) < 1 << 24
    for d16 in range(16 * m, 16 * (m + 64), 7):                 # the matcher's own disparity in 1/16 px
        v = math.floor((d16 - 16 * m) / 16 / 64 * 65535 + 0.5)
        shift = (gr * (v - conv) + (1 << 23)) >> 24
        # |error| <= 1/2 (the rounding to a pixel) + the quantisation of v (64 K s / 65535 / 2 px) and of the gain (1/512 px over the range)
        assert abs(shift + K * s * d16 / 16) <= 0.5 + K * s * 64 / 65535 + 1 / 256, (d16, shift)
    with_map = source_parallax({"mode": "metric", "min_disparity": m, "eye_width": W_eye}, Whi, (0.5, 0.25, 1.0, 0.0), K)
    assert with_map["scale"] == 2 * s                          # the map shows half of the eye across the whole 4K frame


def test_source_parallax_refusals():
    from video_3d_pipeline.convert import DepthTo3DConverter, source_parallax
    ok = {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": 960}
    for block in (None, {}, {"mode": "frame"}, dict(ok, mode="window")):
        with pytest.raises(ValueError, match="--depth-range metric"):
            source_parallax(block, 3840)
    for block in (dict(ok, eye_width=None), dict(ok, eye_width=0), dict(ok, min_disparity="auto"), dict(ok, min_disparity=-65)):
        with pytest.raises(ValueError):
            source_parallax(block, 3840)
    for K in (-1.0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError):
            source_parallax(ok, 3840, None, K)
    with pytest.raises(ValueError, match="2\\^24"):                # s = 8192 / 2, K = 1/4: 64 K s = 65536 px = 2^24 / 256
        source_parallax(dict(ok, eye_width=2), 8192, None, 0.25)
    assert 65000 < source_parallax(dict(ok, eye_width=2), 8192, None, 0.2499)["max_shift"] < 65536
    with pytest.raises(ValueError, match="--parallax source"):
        DepthTo3DConverter(backend=SourceRenderBackend(), fill_from_source="sbs.npy")
    with pytest.raises(ValueError):
        DepthTo3DConverter(backend=SourceRenderBackend(), parallax="film")
    with pytest.raises(ValueError):
        DepthTo3DConverter(backend=SourceRenderBackend(), parallax="source", parallax_gain=-2)
    with pytest.raises(ValueError):
        DepthTo3DConverter(backend=SourceRenderBackend(), parallax="source", fill_from_source="s.npy", source_start_frame=-1)
    conv = DepthTo3DConverter(backend=SourceRenderBackend(), parallax="source")
    with pytest.raises(ValueError, match="set_source_parallax"):
        conv.render_frame(np.zeros((2, 4, 3), np.uint8), np.zeros((2, 4), np.uint16))


def test_cli_refusals(inputs, capsys):
    tmp, _, _ = inputs
    base = [tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "o.json"]
    for extra, word in ((["--parallax", "source", "--max-shift", "30"], "--max-shift"),
                        (["--parallax", "source", "--convergence", "0.5"], "--convergence"),
                        (["--parallax", "source", "--eye-split", "0.5"], "--eye-split"),
                        (["--parallax-gain", "2"], "--parallax source"),
                        (["--fill-from-source", tmp / "v4k.npy"], "--parallax source"),
                        (["--source-start-frame", "2"], "--fill-from-source"),
                        (["--parallax", "source"], "--depth-range metric")):        # a depth directory carries no depth_range block
        be = SourceRenderBackend()
        assert _convert(base + extra, be) == 1 and not be.calls, extra
        assert word in capsys.readouterr().out, extra
    assert not (tmp / "o.json").exists()
    from video_3d_pipeline import pipeline
    assert pipeline.main(["a.npy", "b.npy", "--stereo-output", "x.json", "--parallax", "source", "--max-shift", "3", "--device", "cpu"]) == 1
    assert "--max-shift" in capsys.readouterr().out


def test_metric_with_a_percentile_is_refused_before_anything_is_decoded(tmp_path, capsys):
    from video_3d_pipeline import depth
    with pytest.raises(ValueError, match="--range-percentile"):
        _extractor(tmp_path, "bad", depth_range="metric", range_percentile=98.0)
    with pytest.raises(ValueError):
        _extractor(tmp_path, "bad2", depth_range="window")
    assert depth.main(["no_such_clip.npy", "--depth-range", "metric", "--range-percentile", "98", "--device", "cpu"]) == 1
    assert "--range-percentile" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------------------------
# the depth side: calls, keys, files
# ------------------------------------------------------------------------------------------------------------------------
def test_metric_depth_cli_calls_keys_and_files(sbs_clips, capsys):
    tmp, sbs, v4k, _ = sbs_clips
    plain_be, metric_be = MetricStereoBackend(), MetricStereoBackend()
    plain = _extractor(tmp, "plain", plain_be)
    capsys.readouterr()
    metric = _extractor(tmp, "metric", metric_be, depth_range="metric", fill_holes=False)
    assert capsys.readouterr().out.count("far end of the search window") == 1
    # the cache key: unchanged by default, `_metric` appended with the flag
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    legacy = HybridStereoDepthExtractor(work_dir=str(tmp / "d_plain"), cache_dir=str(tmp / "d_plain"), batch_size=2, stereo_only=True,
                                        backend=OracleStereoBackend())
    assert plain.get_cache_path(sbs, 0, 5) == legacy.get_cache_path(sbs, 0, 5)
    import hashlib
    key = f"{sbs}_0_5_{plain.model_checkpoint}_True"
    assert plain.get_cache_path(sbs, 0, 5).name == "depth_" + hashlib.md5(key.encode()).hexdigest()[:16]
    assert metric.get_cache_path(sbs, 0, 5).name == "depth_" + hashlib.md5((key + "_metric").encode()).hexdigest()[:16]
    d_plain, d_metric = plain.process_video_sbs(sbs), metric.process_video_sbs(sbs)
    assert set(plain_be.calls) == {"minmax"} and set(metric_be.calls) == {"metric"}
    assert not (d_plain / "depth_range.json").exists() and "depth_range" not in plain.manifest_extra()
    block = json.loads((d_metric / "depth_range.json").read_text())
    assert block == {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": SW} == metric.manifest_extra()["depth_range"]
    # a sample means 64 s / 65535 pixels whatever else is in the frame
    from oracle import oracle as O
    from video_3d_pipeline.utils import iter_frames, read_png16
    f0 = next(iter_frames(sbs))
    want = O.disp_to_depth(O.sgbm_compute(*O.sbs_to_gray(f0, True)))
    got = read_png16(d_metric / "depth_000000.png").astype(np.float64) * 64 / 65535
    assert np.abs(got - want).max() <= 64 / 65535
    # the upscale CLI copies the block into the 4K manifest; without the side file the manifest has no such key
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    man = json.loads(open(up.process_depth_upscaling(str(d_metric), v4k, output_path=str(tmp / "up_m.json"))).read())
    assert man["depth_range"] == block
    man = json.loads(open(up.process_depth_upscaling(str(d_plain), v4k, output_path=str(tmp / "up_p.json"))).read())
    assert "depth_range" not in man


def test_metric_with_a_radius_replaces_only_the_range(sbs_clips):
    tmp, sbs, _, _ = sbs_clips
    be = MetricStereoBackend()
    _extractor(tmp, "tm", be, depth_range="metric", fill_holes=True, temporal_radius=1, min_disparity=-32).process_video_sbs(sbs)
    assert be.calls and all(c == ("stabilize", True) for c in be.calls)
    be = MetricStereoBackend()
    ex = _extractor(tmp, "tp", be, temporal_radius=1)
    ex.process_video_sbs(sbs)
    assert ("stabilize", False) in be.calls and "range" in be.calls and "depth_range" not in ex.manifest_extra()


def test_no_half_eye_width_with_no_unsqueeze(sbs_clips):
    tmp, sbs, _, _ = sbs_clips
    ex = _extractor(tmp, "nu", depth_range="metric", fill_holes=True, unsqueeze_sbs=False, min_disparity=-32)
    ex.process_video_sbs(sbs)
    assert ex.manifest_extra()["depth_range"] == {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": -32, "eye_width": SW // 2}


# ------------------------------------------------------------------------------------------------------------------------
# pipeline and convert CLI
# ------------------------------------------------------------------------------------------------------------------------
def _pipeline(tmp, sbs, v4k, tag, backend, ctor=None, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp / f"w_{tag}"), batch_size=2, stereo_only=True, guide_batch=3, backend=backend, **(ctor or {}))
    return json.loads(open(pipe.run(sbs, v4k, output_path=str(tmp / f"depth_{tag}.json"), **kw)).read())


class _PackPipelineBackend(MetricPipelineBackend):
    def render_stereo(self, u16_4k, gains, layout, subpixel=False):
        return [None if f is None else P.render(f, q, *gains, layout, subpixel) for f, q in zip(self.staged, u16_4k)]


def test_pipeline_source_parallax_equals_the_convert_cli(sbs_clips):
    tmp, sbs, v4k, _ = sbs_clips
    with pytest.raises(ValueError, match="--depth-range metric"):
        _pipeline(tmp, sbs, v4k, "bad", _PackPipelineBackend(), stereo_output=str(tmp / "bad3d.json"), stereo_options=dict(parallax="source"))
    be = _PackPipelineBackend()
    man = _pipeline(tmp, sbs, v4k, "m", be, ctor=dict(depth_range="metric", fill_holes=False, min_disparity=-32), guide_start_frame=1,
                    stereo_output=str(tmp / "m3d.json"), stereo_options=dict(parallax="source", parallax_gain=1.5, layout="half-tb"))
    assert set(c for c in be.calls) == {"metric"}
    assert man["depth_range"] == {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": -32, "eye_width": SW}
    got = json.loads((tmp / "m3d.json").read_text())
    s = W4 / SW
    assert (got["parallax"], got["parallax_scale"], got["parallax_gain"]) == ("source", s, 1.5)
    assert got["eye_split"] == 0 and got["convergence"] == 0.5 and got["max_shift"] == 1.5 * s * 64 * 65536 / 65535
    assert got["gain_left"] == 0 and got["gain_right"] == -math.floor(got["max_shift"] * 256 + 0.5)
    crb = SourceRenderBackend()
    assert _convert([v4k, tmp / "depth_m.json", "--output", tmp / "cli3d.json", "--guide-start-frame", "1", "--layout", "half-tb",
                     "--parallax", "source", "--parallax-gain", "1.5"], crb) == 0
    want = json.loads((tmp / "cli3d.json").read_text())
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"]) and len(_pngs(got["frames_dir"])) == 6
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    assert crb.calls == [None, None]                           # no source keyword without --fill-from-source


def test_nothing_changes_without_the_flags(sbs_clips):
    """manifest keys, backend calls and output bytes of the default run: those of a backend that predates every new keyword"""
    tmp, sbs, v4k, _ = sbs_clips
    opts = dict(max_shift=25.0, convergence=0.4, eye_split=0.7, layout="full-sbs")
    old = _pipeline(tmp, sbs, v4k, "old", RefStereoPipelineBackend(), guide_start_frame=1, stereo_output=str(tmp / "old3d.json"),
                    stereo_options=opts)
    be = MetricPipelineBackend()
    new = _pipeline(tmp, sbs, v4k, "new", be, guide_start_frame=1, stereo_output=str(tmp / "new3d.json"), stereo_options=opts)
    assert set(be.calls) == {"minmax"} and sorted(old) == sorted(new) and "depth_range" not in new
    assert _pngs(old["frames_dir"]) == _pngs(new["frames_dir"])
    a, b = json.loads((tmp / "old3d.json").read_text()), json.loads((tmp / "new3d.json").read_text())
    assert sorted(a) == sorted(b) and not {"parallax", "parallax_scale", "parallax_gain", "fill_from_source"} & set(b)
    assert _pngs(a["frames_dir"]) == _pngs(b["frames_dir"])
    from test_convert_host import RefRenderBackend                 # its render_batch knows neither subpixel= nor source=
    assert _convert([v4k, tmp / "depth_new.json", "--output", tmp / "c.json", "--guide-start-frame", "1", "--max-shift", "25",
                     "--convergence", "0.4", "--eye-split", "0.7"], RefRenderBackend()) == 0
    c = json.loads((tmp / "c.json").read_text())
    assert _pngs(c["frames_dir"]) == _pngs(a["frames_dir"]) and sorted(c) == sorted(a)


def test_fill_from_source_on_the_convert_cli(sbs_clips):
    tmp, sbs, v4k, _ = sbs_clips
    _pipeline(tmp, sbs, v4k, "f", _PackPipelineBackend(), ctor=dict(depth_range="metric", fill_holes=True))
    be = SourceRenderBackend()
    assert _convert([v4k, tmp / "depth_f.json", "--output", tmp / "f3d.json", "--parallax", "source", "--fill-from-source", sbs,
                     "--source-start-frame", "1"], be) == 0
    from video_3d_pipeline.register import map_to_q16
    q = map_to_q16(1, 0, SW // 2, W4) + map_to_q16(1, 0, SH, H4)
    assert q[:2] == (65536 * (SW // 2) // W4, (65536 * (SW // 2) // W4 - 65536) // 2) and map_to_q16(1, 0, 240, 480) == (32768, -16384)
    assert be.calls == [(4, 2, q)]                             # SBS frames 1 .. 4: the clip ends, so does the render, with a warning
    man = json.loads((tmp / "f3d.json").read_text())
    assert man["count"] == 4 and man["fill_from_source"] == sbs and man["source_start_frame"] == 1 and man["parallax"] == "source"
    frames4k, sbs_frames = _read_clip(v4k), _read_clip(sbs)
    from video_3d_pipeline.utils import read_png16
    dman = json.loads((tmp / "depth_f.json").read_text())
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    got = _read_clip(man["frames_dir"])
    for i in range(4):
        d = read_png16(f"{dman['frames_dir']}/depth4k_{i:06d}.png")
        assert np.array_equal(got[i], X.render(frames4k[i], d, *gains, P.FULL_SBS, False, sbs_frames[1 + i], 2, *q)), i
    # the NumPy surface
    from video_3d_pipeline.convert import DepthTo3DConverter
    conv = DepthTo3DConverter(backend=SourceRenderBackend(), parallax="source")
    conv.set_source_parallax(dman["depth_range"], W4)
    d = read_png16(f"{dman['frames_dir']}/depth4k_000000.png")
    assert np.array_equal(conv.render_frame(frames4k[0], d, source=sbs_frames[1]), got[0])
    assert np.array_equal(conv.render_frame(frames4k[0], d), P.render(frames4k[0], d, *gains, P.FULL_SBS))


# ------------------------------------------------------------------------------------------------------------------------
# the experiment
# ------------------------------------------------------------------------------------------------------------------------
def test_source_parallax_quality():
    """synthetic.stereo_pair(480, 270, 0); depth: the ground-truth disparity carried into the left view (forward warp, nearest wins,
    gaps take the smaller neighbour); frame: the left view; error: mean absolute BGR error of the rendered right eye against the true one.

    Measured with these references: today's defaults 39.0, source parallax 4.44 (ratio 0.11); in the holes (6.8 % of the frame)
    background extension 35.4, the stored 2:1 squeezed right eye 4.89 (ratio 0.14)."""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline._native import stereo_gains
    from video_3d_pipeline.convert import fill_map_q16, source_parallax
    W, H = 480, 270
    L, Rt = syn.stereo_pair(W, H, 0)
    dR = syn.gt_disparity(W, H)
    dL = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in np.argsort(dR[y], kind="stable"):             # ascending: the nearest (largest) is written last and wins
            t = int(round(x + float(dR[y, x])))
            if 0 <= t < W:
                dL[y, t] = max(dL[y, t], dR[y, x])
        idx = np.flatnonzero(dL[y] > 0)
        for x in np.flatnonzero(dL[y] == 0):
            a, b = idx[idx < x], idx[idx > x]
            dL[y, x] = min(([dL[y, a[-1]]] if len(a) else []) + ([dL[y, b[0]]] if len(b) else []))

    def err(E, mask=None):
        e = np.abs(E.astype(int) - Rt.astype(int)).mean(axis=2)
        return float(e[mask].mean() if mask is not None else e.mean())

    # the parent: per-frame min-max depth, 48 px, 0.5, 0.5, through the existing reference
    Dn = np.rint((dL - dL.min()) / (dL.max() - dL.min()) * 65535).astype(np.uint16)
    parent = err(R.render(L, Dn, *R.stereo_gains())[:, W:])
    # part 1: metric depth (the range (0, 64)) and the source's parallax, the matcher's eye as wide as the frame
    D = np.rint(dL / 64 * 65535).astype(np.uint16)
    p = source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": W}, W)
    gains = stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    ER = R.render(L, D, *gains)[:, W:]
    hole = ~X.hit_mask(D, gains[1], gains[2])
    share = float(hole.mean())
    print(f"hole share {share:.4f}; all pixels: parent {parent:.2f}, source parallax {err(ER):.2f} (ratio {err(ER) / parent:.3f})")
    assert 0.02 <= share <= 0.15
    assert err(ER) <= 0.25 * parent
    # part 2: the holes from the stored (2:1 squeezed) right eye
    sbs = syn.sbs_frame(W, H, 0)
    q = fill_map_q16(None, (W // 2, H), (W, H))
    assert q == (32768, -16384, 65536, 0)
    EF = X.eyes(L, D, *gains, False, sbs, 2, *q)[1]
    assert np.array_equal(EF[~hole], ER[~hole])
    print(f"holes: background {err(ER, hole):.2f}, source fill {err(EF, hole):.2f} (ratio {err(EF, hole) / err(ER, hole):.3f}); "
          f"all pixels with the fill {err(EF):.2f}")
    assert err(EF, hole) <= 0.33 * err(ER, hole)
