"""Host side of the robust depth range (--range-percentile) on CPU: option parsing, the streaming driver, both CLIs and block
sharding with oracle-backed stand-ins whose new backend methods come from tests/range_ref.py, and the quality of the result on
the temporally coherent synthetic clip through the oracle matcher."""
import json
import os

import numpy as np
import pytest

import range_ref as RR
import temporal_ref as TR
from oracle import oracle as O
from test_host import OracleStereoBackend, OracleUpscaleBackend
from test_pipeline_host import OraclePipelineBackend
from test_temporal_host import (NF, ForbiddenPipelineBackend, ForbiddenStereoBackend, TemporalPipelineBackend, TemporalStereoBackend,
                                _depth_cli, _pipeline, _pngs, clips)  # noqa: F401  (clips: the module's fixture)

Q = 9000          # on the 192x48 clip the 90th percentile lies well inside the scene: the files differ from the max's


class _RangeMethods:
    """what HipStereoBackend adds or widens for the option, NumPy"""

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill, range_quantile=10000):
        return RR.stabilize(depth, gray, radius, tau, cut_threshold, int(fill), t0, n, q=range_quantile)

    def depth_to_u16_robust(self, depth, range_quantile):
        return RR.to_u16(np.asarray(depth, np.float32), range_quantile)


class RangeStereoBackend(_RangeMethods, TemporalStereoBackend):
    pass


class RangePipelineBackend(_RangeMethods, TemporalPipelineBackend):
    pass


class _NoRobust:
    """option off: the new method must not be called, and temporal_stabilize keeps its eight positional arguments (the
    stand-ins of test_temporal_host.py take no more: a ninth is a TypeError)"""

    def depth_to_u16_robust(self, *a, **k):
        raise AssertionError("depth_to_u16_robust called with the option off")


class OffStereoR0(_NoRobust, ForbiddenStereoBackend):
    pass


class OffPipelineR0(_NoRobust, ForbiddenPipelineBackend):
    pass


class OffStereoR2(_NoRobust, TemporalStereoBackend):
    pass


class OffPipelineR2(_NoRobust, TemporalPipelineBackend):
    pass


def _maps(d, n=NF):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), f"depth_{i:06d}.png")) for i in range(n)])


def _oracle_clip(sbs):
    from video_3d_pipeline.utils import iter_frames
    frames = list(iter_frames(sbs))
    return OracleStereoBackend().sbs_to_disparity(frames, True), np.stack([O.sbs_to_gray(f, True)[0] for f in frames])


# ---------------------------------------------------------------- the option itself

def test_check_range_percentile():
    from video_3d_pipeline.temporal import check_range_percentile
    assert check_range_percentile(100) == 10000 and check_range_percentile(100.0) == 10000
    assert check_range_percentile(98) == 9800 and check_range_percentile(99.9) == 9990 and check_range_percentile(99.99) == 9999
    assert check_range_percentile(50) == 5000 and check_range_percentile(50.01) == 5001 and check_range_percentile(97.5) == 9750
    for bad in (49.99, 100.01, 0, -1, 98.123, 99.999, float("nan"), float("inf"), True, "98", None):
        with pytest.raises(ValueError):
            check_range_percentile(bad)


def test_suffix_manifest_and_constructors_keep_their_old_forms():
    from video_3d_pipeline.temporal import BlockStabilizer, TemporalStabilizer, cache_suffix, manifest_entry
    assert cache_suffix(0, 12, 20, True) == "" and cache_suffix(0, 12, 20, True, 10000) == ""
    assert cache_suffix(0, 12, 20, True, 9800) == "_rangeq9800"
    assert cache_suffix(2, 12, 20, True, 10000) == cache_suffix(2, 12, 20, True)
    assert cache_suffix(2, 12, 20, True, 9800) == cache_suffix(2, 12, 20, True) + "_rangeq9800"
    assert manifest_entry(2, 12, 20, True) == manifest_entry(2, 12, 20, True, 10000) == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True}
    assert manifest_entry(2, 12, 20, True, 9800)["range_quantile"] == 9800
    be = RangeStereoBackend()
    assert TemporalStabilizer(be, 2).range_quantile == 10000 and TemporalStabilizer(be, 2, 12, 20, True, 9800).range_quantile == 9800
    assert BlockStabilizer(be, (2, 12, 20, True), 0, 3, 0).stab.range_quantile == 10000
    assert BlockStabilizer(be, (2, 12, 20, True), 0, 3, 0, 9800).stab.range_quantile == 9800
    for bad in (4999, 10001, 98.5, True):
        with pytest.raises(ValueError):
            TemporalStabilizer(be, 2, range_quantile=bad)


def test_command_lines_reach_the_constructors(clips):
    from video_3d_pipeline import depth as depth_mod, pipeline as pipe_mod
    sbs, v4k = clips
    for mod, name, argv in ((depth_mod, "HybridStereoDepthExtractor", [sbs]), (pipe_mod, "SbsTo4kDepthPipeline", [sbs, v4k])):
        seen = {}
        orig = getattr(mod, name)

        class Spy(orig):
            def __init__(self, **kw):
                seen.update(kw)
                raise RuntimeError("stop here")

        setattr(mod, name, Spy)
        try:
            assert mod.main(argv + ["--range-percentile", "98", "--temporal-radius", "2"]) == 1
            assert (seen["range_percentile"], seen["temporal_radius"]) == (98.0, 2)
            seen.clear()
            assert mod.main(argv) == 1
            assert seen["range_percentile"] == 100.0
        finally:
            setattr(mod, name, orig)
    with pytest.raises(ValueError):
        depth_mod.HybridStereoDepthExtractor(work_dir="unused", backend=OracleStereoBackend(), range_percentile=98.123)


# ---------------------------------------------------------------- the streaming driver

class _NumpyBackend:
    temporal_concat = TemporalStereoBackend.temporal_concat
    temporal_stabilize = _RangeMethods.temporal_stabilize


@pytest.mark.parametrize("T", [1, 7, 11])
def test_streaming_equals_the_whole_clip_call(T):
    from video_3d_pipeline.temporal import TemporalStabilizer
    rng = np.random.default_rng(T)
    depth = (rng.integers(0, 1024, (T, 6, 9)) / 16.0).astype(np.float32)
    base = rng.integers(0, 256, (6, 9))
    gray = np.clip(base[None] + rng.integers(-15, 16, (T, 6, 9)), 0, 255).astype(np.uint8)
    if T > 4:
        gray[4:] = 255 - gray[4:]
    for R in (1, 2, 8):
        want = RR.stabilize(depth, gray, R, q=Q)
        assert (want != TR.stabilize(depth, gray, R)).any()
        for step in (1, 2, 3, 5):
            st = TemporalStabilizer(_NumpyBackend(), R, range_quantile=Q)
            parts = []
            for i in range(0, T, step):
                out = st.push(depth[i:i + step].copy(), gray[i:i + step].copy())
                parts += [] if out is None else [out]
            out = st.finish()
            parts += [] if out is None else [out]
            assert np.array_equal(np.concatenate(parts), want), (R, step)


# ---------------------------------------------------------------- option off: nothing changes

def test_option_off_changes_nothing(tmp_path, clips):
    """the parent's stand-ins and default arguments against stand-ins that forbid the new method and refuse a ninth argument,
    with the option spelt out as 100: same directory names, same files byte for byte, at radius 0 and radius 2"""
    sbs, v4k = clips
    for R, plain_be, plain_pbe, off_be, off_pbe in ((0, OracleStereoBackend, OraclePipelineBackend, OffStereoR0, OffPipelineR0),
                                                    (2, TemporalStereoBackend, TemporalPipelineBackend, OffStereoR2, OffPipelineR2)):
        _, plain_dir = _depth_cli(tmp_path, sbs, f"plain{R}", plain_be(), temporal_radius=R)
        _, off_dir = _depth_cli(tmp_path, sbs, f"off{R}", off_be(), temporal_radius=R, range_percentile=100.0)
        assert off_dir.name == plain_dir.name and sorted(os.listdir(off_dir)) == sorted(os.listdir(plain_dir))
        assert _pngs(off_dir) == _pngs(plain_dir) and len(_pngs(off_dir)) == NF
        if R:
            assert (off_dir / "temporal.json").read_bytes() == (plain_dir / "temporal.json").read_bytes()
            assert "range_quantile" not in json.loads((off_dir / "temporal.json").read_text())
        else:
            assert not (off_dir / "temporal.json").exists()
        _, plain = _pipeline(tmp_path, sbs, v4k, f"plain{R}", plain_pbe(), run_kw=dict(keep_depth_maps=True), temporal_radius=R)
        pipe, off = _pipeline(tmp_path, sbs, v4k, f"off{R}", off_pbe(), run_kw=dict(keep_depth_maps=True), temporal_radius=R,
                              range_percentile=100)
        assert _pngs(off["frames_dir"]) == _pngs(plain["frames_dir"]) and len(_pngs(off["frames_dir"])) == NF
        assert {k: v for k, v in off.items() if k != "frames_dir"} == {k: v for k, v in plain.items() if k != "frames_dir"}
        assert ("temporal" in off) == bool(R)
        cache = pipe.extractor.get_cache_path(sbs, 0, NF)
        assert cache.name == plain_dir.name and _pngs(cache) == _pngs(plain_dir)
    # and the files are what the contract without the option says
    depth, gray = _oracle_clip(sbs)
    assert np.array_equal(_maps(off_dir), TR.stabilize(depth, gray, 2))


# ---------------------------------------------------------------- option on

@pytest.mark.parametrize("R", [0, 2])
def test_depth_cli_and_one_pass_pipeline_write_the_same_files(tmp_path, clips, R):
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    sbs, v4k = clips
    _, off_dir = _depth_cli(tmp_path, sbs, "off", TemporalStereoBackend(), temporal_radius=R)
    ex, ddir = _depth_cli(tmp_path, sbs, "on", RangeStereoBackend(), temporal_radius=R, range_percentile=Q / 100)
    _, other = _depth_cli(tmp_path, sbs, "on2", RangeStereoBackend(), temporal_radius=R, range_percentile=98)
    assert len({off_dir.name, ddir.name, other.name}) == 3                          # the quantile is part of the cache key
    entry = {"radius": R, "tau": 12, "cut_threshold": 20, "fill": True, "range_quantile": Q}
    assert json.loads((ddir / "temporal.json").read_text()) == entry
    depth, gray = _oracle_clip(sbs)
    want = RR.stabilize(depth, gray, R, q=Q) if R else RR.to_u16(depth, Q)
    got = _maps(ddir)
    assert np.array_equal(got, want) and (got != _maps(off_dir)).any()
    assert ex.last_decoded_frames == NF
    # depth CLI + upscale CLI == one pass
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    out = up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / "cli.json"))
    want4k = _pngs(json.loads(open(out).read())["frames_dir"])
    pipe, man = _pipeline(tmp_path, sbs, v4k, "on", RangePipelineBackend(), run_kw=dict(keep_depth_maps=True), temporal_radius=R,
                          range_percentile=Q / 100)
    assert len(want4k) == NF and _pngs(man["frames_dir"]) == want4k
    assert man["count"] == NF and man["temporal"] == entry
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)
    assert json.loads((cache / "temporal.json").read_text()) == entry
    # start_frame / max_frames with the option on
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    ex2 = HybridStereoDepthExtractor(work_dir=str(tmp_path / "sub"), cache_dir=str(tmp_path / "sub"), batch_size=2, stereo_only=True,
                                     backend=RangeStereoBackend(), temporal_radius=R, range_percentile=Q / 100)
    sub = ex2.process_video_sbs(sbs, start_frame=1, max_frames=3)
    assert np.array_equal(_maps(sub, 3), RR.stabilize(depth[1:4], gray[1:4], R, q=Q) if R else RR.to_u16(depth[1:4], Q))


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_write_what_one_process_writes(tmp_path, clips, monkeypatch, world):
    """ranks simulated one after the other: the histogram is per frame, so the halo of R frames is still enough (radius 2), and
    round-robin frames need nothing from each other (radius 0)"""
    from video_3d_pipeline import sharding
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs, v4k = clips
    for n_frames, R in ((NF, 2), (3, 2), (NF, 0)):
        kw = dict(batch_size=2, stereo_only=True, temporal_radius=R, range_percentile=Q / 100)
        tag = f"{n_frames}_{R}"
        one = HybridStereoDepthExtractor(work_dir=str(tmp_path / f"o{tag}"), cache_dir=str(tmp_path / f"o{tag}"), backend=RangeStereoBackend(), **kw)
        want_dir = one.process_video_sbs(sbs, max_frames=n_frames)
        pone = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"po{tag}"), guide_batch=2, backend=RangePipelineBackend(), **kw)
        want4k = json.loads(open(pone.run(sbs, v4k, output_path=str(tmp_path / f"po{tag}.json"), max_frames=n_frames)).read())
        with monkeypatch.context() as mp:
            mp.setattr(sharding, "_initialized", lambda: True)
            mp.setattr(sharding, "barrier", lambda: None)
            mp.setattr(sharding, "total", lambda v: n_frames)
            mp.setenv("WORLD_SIZE", str(world))
            for rank in reversed(range(world)):
                mp.setenv("RANK", str(rank))
                ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / f"w{tag}"), cache_dir=str(tmp_path / f"w{tag}"),
                                                backend=RangeStereoBackend(), **kw)
                got_dir = ex.process_video_sbs(sbs, max_frames=n_frames, force_reprocess=True)
                pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pw{tag}"), guide_batch=2, backend=RangePipelineBackend(), **kw)
                out4k = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pw{tag}.json"), max_frames=n_frames, force_reprocess=True)
        got4k = json.loads(open(out4k).read())
        assert len(_pngs(want_dir)) == n_frames and _pngs(got_dir) == _pngs(want_dir), (world, n_frames, R)
        assert json.loads((got_dir / "temporal.json").read_text())["range_quantile"] == Q
        assert got4k["count"] == n_frames and got4k["temporal"]["range_quantile"] == Q
        assert _pngs(got4k["frames_dir"]) == _pngs(want4k["frames_dir"]), (world, n_frames, R)


# ---------------------------------------------------------------- quality on the temporally coherent clip

def test_robust_range_quality_on_the_synthetic_clip():
    """320x120, 9 frames, the clip, static mask and flicker() of test_temporal_host.py's quality test, oracle matcher, q = 9800.
    The yardstick is the maximum range computed here by the contract without the option (TR.minmax):
      static-region flicker of the u16 samples below half of the maximum range's, per frame (R = 0) and at R = 2, tau = 12;
      every frame's white point at or above 40.0, the moving object's ground truth: the object is not clipped.
    Half is a wide margin for another noise seed, not a tuned bound: measured 1044.7 -> 87.0 (R = 0) and 940.7 -> 28.8 (R = 2),
    ratios 0.083 and 0.031, with every frame's white point exactly 40.0."""
    from video_3d_pipeline import synthetic as syn
    W, H, T, R, q = 320, 120, 9, 2, 9800
    L, Rt, gt = syn.temporal_clip(W, H, T)
    depth = np.stack([O.disp_to_depth(O.sgbm_compute(l, r)) for l, r in zip(L, Rt)])
    assert not TR.cuts(L, 20).any()

    boxes = [syn.temporal_object_box(W, H, t) for t in range(T)]
    static = np.ones((H, W), bool)
    static[:, :64 + 8] = False
    x0, x1 = min(b[0] for b in boxes), max(b[2] for b in boxes)
    static[max(boxes[0][1] - 6, 0):boxes[0][3] + 6, max(x0 - 46, 0):x1 + 6] = False
    both = static[None] & (depth[1:] > 0) & (depth[:-1] > 0)
    assert both.mean() > 0.3

    def flicker(a):
        a = a.astype(np.int64)
        return float(np.abs(a[1:] - a[:-1])[both].mean())

    max0 = flicker(TR.to_u16_range(depth, TR.minmax(depth)))                       # the parent's per-frame path
    assert np.array_equal(TR.to_u16_range(depth, TR.minmax(depth)), np.stack([O.depth_to_u16(d) for d in depth]))
    rob0 = flicker(RR.to_u16(depth, q))
    max2 = flicker(TR.stabilize(depth, L, R))                                      # the parent's stabilised path
    rob2 = flicker(RR.stabilize(depth, L, R, q=q))
    his = RR.robust_minmax(depth, q)[:, 1]
    print(f"u16 flicker, maximum -> 98th percentile: R = 0 {max0:.1f} -> {rob0:.1f} levels; R = 2 {max2:.1f} -> {rob2:.1f} levels; "
          f"white points {his.tolist()}; maxima {TR.minmax(depth)[:, 1].tolist()}")
    assert rob0 < 0.5 * max0 and rob2 < 0.5 * max2
    assert (his >= np.float32(40.0)).all()
    assert gt.max() == 40.0
    for t in range(T):
        n_valid, k, _ = RR.select(RR.histogram(depth[t]), q)
        assert RR.above(depth[t], his[t]) <= n_valid - k
