"""Host side of the temporal stabilisation on CPU: the streaming driver, both CLIs with oracle-backed stand-ins whose new
backend methods come from tests/temporal_ref.py, block sharding, and the quality of the result on the temporally coherent
synthetic clip through the oracle matcher."""
import json
import os

import numpy as np
import pytest

import temporal_ref as TR
from oracle import oracle as O
from test_host import OracleStereoBackend, OracleUpscaleBackend
from test_pipeline_host import OraclePipelineBackend

SW, SH, NF = 192, 48, 7


class _TemporalMethods:
    """the new backend methods, NumPy: what HipStereoBackend adds for the stage"""

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None):
        self._lg = np.stack([O.sbs_to_gray(f, unsqueeze)[0] for f in frames])
        return super().sbs_to_disparity(frames, unsqueeze, mono_provider)

    def left_gray(self, n):
        return self._lg[:n]

    def temporal_concat(self, held, new):
        return np.array(new) if held is None else np.concatenate([held, new])

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill):
        return TR.stabilize(depth, gray, radius, tau, cut_threshold, int(fill), t0, n)

    def to_host_u16(self, u16):
        return np.array(u16, np.uint16)


class TemporalStereoBackend(_TemporalMethods, OracleStereoBackend):
    pass


class TemporalPipelineBackend(_TemporalMethods, OraclePipelineBackend):
    pass


class _Forbidden:
    """radius 0 must not touch the stage"""

    def left_gray(self, n):
        raise AssertionError("left_gray called with the stage off")

    def temporal_concat(self, held, new):
        raise AssertionError("temporal_concat called with the stage off")

    def temporal_stabilize(self, *a):
        raise AssertionError("temporal_stabilize called with the stage off")


class ForbiddenStereoBackend(_Forbidden, OracleStereoBackend):
    pass


class ForbiddenPipelineBackend(_Forbidden, OraclePipelineBackend):
    pass


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("tclips")
    np.save(d / "sbs.npy", syn.temporal_sbs_clip(SW, SH, NF, cut_at=4, speed=4))
    rng = np.random.default_rng(5)
    np.save(d / "v4k.npy", rng.integers(0, 256, (NF, 2 * SH, 2 * SW, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


# ---------------------------------------------------------------- the streaming driver

class _NumpyBackend:
    temporal_concat = _TemporalMethods.temporal_concat
    temporal_stabilize = _TemporalMethods.temporal_stabilize


@pytest.mark.parametrize("T", [1, 7, 11])
def test_streaming_equals_the_whole_clip_call(T):
    from video_3d_pipeline.temporal import TemporalStabilizer
    rng = np.random.default_rng(T)
    depth = (rng.integers(0, 1024, (T, 6, 9)) / 16.0).astype(np.float32)
    base = rng.integers(0, 256, (6, 9))
    gray = np.clip(base[None] + rng.integers(-15, 16, (T, 6, 9)), 0, 255).astype(np.uint8)
    if T > 4:
        gray[4:] = 255 - gray[4:]                            # a scene cut inside the clip
    for R in (1, 2, 8):                                      # 8: larger than the 1- and 7-frame clips
        want = TR.stabilize(depth, gray, R)
        for step in (1, 2, 3, 5):
            st = TemporalStabilizer(_NumpyBackend(), R)
            parts, lag = [], []
            for i in range(0, T, step):
                d, g = depth[i:i + step].copy(), gray[i:i + step].copy()
                out = st.push(d, g)
                d[:] = -1                                    # the driver keeps copies, not the pass's buffers
                g[:] = 0
                parts += [] if out is None else [out]
                lag.append(st.pending())
            assert all(p <= R for p in lag[:-1]) or T <= R
            out = st.finish()
            parts += [] if out is None else [out]
            assert np.array_equal(np.concatenate(parts), want), (R, step)
            assert st.pending() == 0
            with pytest.raises(RuntimeError):
                st.push(depth[:1], gray[:1])


def test_parameter_checks():
    from video_3d_pipeline.temporal import TemporalStabilizer, cache_suffix, check_parameters
    assert check_parameters(0) == (0, 12, 20, True)
    for bad in (dict(radius=9), dict(radius=-1), dict(radius=1, tau=0), dict(radius=1, tau=256), dict(radius=1, cut_threshold=257),
                dict(radius=1.5), dict(radius=True)):
        with pytest.raises(ValueError):
            check_parameters(**bad)
    with pytest.raises(ValueError):
        TemporalStabilizer(_NumpyBackend(), 0)
    assert cache_suffix(0, 12, 20, True) == "" and cache_suffix(2, 12, 20, True) != cache_suffix(2, 12, 20, False)


def test_temporal_block_partitions_the_clip():
    from video_3d_pipeline.sharding import temporal_block
    for n in (0, 1, 2, 5, 7, 34, 100):
        for world in (1, 2, 3, 8):
            for R in (1, 2, 8):
                owned = []
                for rank in range(world):
                    first, count, hb, ha = temporal_block(n, rank, world, R)
                    owned += list(range(first, first + count))
                    assert 0 <= first - hb and first + count + ha <= n and count <= -(-n // world)
                    if count:
                        assert hb == min(R, first) and ha == min(R, n - first - count)
                    else:
                        assert (hb, ha) == (0, 0)
                assert owned == list(range(n)), (n, world, R)
    assert temporal_block(7, 1, 2, 2) == (4, 3, 2, 0)
    with pytest.raises(ValueError):
        temporal_block(7, 2, 2, 1)


# ---------------------------------------------------------------- the CLIs

def _depth_cli(tmp_path, sbs, tag, backend, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=3, stereo_only=True, backend=backend, **kw)
    return ex, ex.process_video_sbs(sbs)


def _pipeline(tmp_path, sbs, v4k, tag, backend, run_kw=None, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=3, stereo_only=True, guide_batch=2, backend=backend, **kw)
    out = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **(run_kw or {}))
    return pipe, json.loads(open(out).read())


def test_radius_zero_changes_nothing(tmp_path, clips):
    sbs, v4k = clips
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", OracleStereoBackend())
    ex, zero_dir = _depth_cli(tmp_path, sbs, "zero", ForbiddenStereoBackend(), temporal_radius=0, temporal_tau=30, temporal_cut=5,
                              temporal_fill=False)
    assert zero_dir.name == plain_dir.name                             # the reference's md5 key, unchanged
    assert sorted(os.listdir(zero_dir)) == sorted(os.listdir(plain_dir)) == [f"depth_{i:06d}.png" for i in range(NF)]
    assert _pngs(zero_dir) == _pngs(plain_dir)
    _, plain = _pipeline(tmp_path, sbs, v4k, "plain", OraclePipelineBackend(), run_kw=dict(keep_depth_maps=True))
    pipe, zero = _pipeline(tmp_path, sbs, v4k, "zero", ForbiddenPipelineBackend(), run_kw=dict(keep_depth_maps=True), temporal_radius=0)
    assert _pngs(zero["frames_dir"]) == _pngs(plain["frames_dir"]) and len(_pngs(zero["frames_dir"])) == NF
    assert {k: v for k, v in zero.items() if k != "frames_dir"} == {k: v for k, v in plain.items() if k != "frames_dir"}
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == plain_dir.name and _pngs(cache) == _pngs(plain_dir) and not (cache / "temporal.json").exists()


def test_depth_cli_with_a_radius(tmp_path, clips):
    from video_3d_pipeline import depth as depth_mod
    from video_3d_pipeline.utils import iter_frames, read_png16
    sbs, _ = clips
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", OracleStereoBackend())
    ex, ddir = _depth_cli(tmp_path, sbs, "r2", TemporalStereoBackend(), temporal_radius=2)
    assert ddir.name != plain_dir.name and ddir.name != _depth_cli(tmp_path, sbs, "r1", TemporalStereoBackend(), temporal_radius=1)[1].name
    assert json.loads((ddir / "temporal.json").read_text()) == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True}
    frames = list(iter_frames(sbs))
    depth = OracleStereoBackend().sbs_to_disparity(frames, True)
    gray = np.stack([O.sbs_to_gray(f, True)[0] for f in frames])
    want = TR.stabilize(depth, gray, 2)
    assert TR.cuts(gray, 20)[4] == 1 and TR.cuts(gray, 20).sum() == 1
    got = np.stack([read_png16(ddir / f"depth_{i:06d}.png") for i in range(NF)])
    assert np.array_equal(got, want)
    assert (got != np.stack([read_png16(plain_dir / f"depth_{i:06d}.png") for i in range(NF)])).any()
    assert ex.last_decoded_frames == NF
    # start_frame / max_frames: frames outside the processed range do not exist for the window
    ex2 = depth_mod.HybridStereoDepthExtractor(work_dir=str(tmp_path / "sub"), cache_dir=str(tmp_path / "sub"), batch_size=2,
                                               stereo_only=True, backend=TemporalStereoBackend(), temporal_radius=2)
    sub = ex2.process_video_sbs(sbs, start_frame=1, max_frames=3)
    got = np.stack([read_png16(sub / f"depth_{i:06d}.png") for i in range(3)])
    assert np.array_equal(got, TR.stabilize(depth[1:4], gray[1:4], 2))
    # the command line reaches the same constructor arguments
    seen = {}

    class Spy(depth_mod.HybridStereoDepthExtractor):
        def __init__(self, **kw):
            seen.update(kw)
            raise RuntimeError("stop here")

    orig = depth_mod.HybridStereoDepthExtractor
    depth_mod.HybridStereoDepthExtractor = Spy
    try:
        assert depth_mod.main([sbs, "--temporal-radius", "3", "--temporal-tau", "9", "--temporal-cut", "30", "--no-temporal-fill"]) == 1
    finally:
        depth_mod.HybridStereoDepthExtractor = orig
    assert (seen["temporal_radius"], seen["temporal_tau"], seen["temporal_cut"], seen["temporal_fill"]) == (3, 9, 30, False)


def test_two_cli_route_and_one_pass_pipeline_write_the_same_4k_files(tmp_path, clips):
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    sbs, v4k = clips
    _, ddir = _depth_cli(tmp_path, sbs, "r2", TemporalStereoBackend(), temporal_radius=2)
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    out = up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / "cli.json"))
    want = _pngs(json.loads(open(out).read())["frames_dir"])
    pipe, man = _pipeline(tmp_path, sbs, v4k, "r2", TemporalPipelineBackend(), run_kw=dict(keep_depth_maps=True), temporal_radius=2)
    assert len(want) == NF and _pngs(man["frames_dir"]) == want
    assert man["count"] == NF and man["temporal"] == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True}
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)
    assert json.loads((cache / "temporal.json").read_text())["radius"] == 2
    _, other = _pipeline(tmp_path, sbs, v4k, "r2nofill", TemporalPipelineBackend(), temporal_radius=2, temporal_fill=False)
    assert _pngs(other["frames_dir"]) != want


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_write_what_one_process_writes(tmp_path, clips, monkeypatch, world):
    """ranks simulated one after the other in this process: contiguous blocks plus halos give the single-process files, also
    for a clip shorter than world * radius"""
    from video_3d_pipeline import sharding
    sbs, v4k = clips
    for n_frames, R in ((NF, 2), (3, 2)):
        from video_3d_pipeline.depth import HybridStereoDepthExtractor
        from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
        one = HybridStereoDepthExtractor(work_dir=str(tmp_path / f"o{n_frames}"), cache_dir=str(tmp_path / f"o{n_frames}"), batch_size=2,
                                         stereo_only=True, backend=TemporalStereoBackend(), temporal_radius=R)
        want_dir = one.process_video_sbs(sbs, max_frames=n_frames)
        pone = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"po{n_frames}"), batch_size=2, stereo_only=True, guide_batch=2,
                                    backend=TemporalPipelineBackend(), temporal_radius=R)
        want4k = json.loads(open(pone.run(sbs, v4k, output_path=str(tmp_path / f"po{n_frames}.json"), max_frames=n_frames)).read())
        with monkeypatch.context() as mp:
            mp.setattr(sharding, "_initialized", lambda: True)
            mp.setattr(sharding, "barrier", lambda: None)
            mp.setattr(sharding, "total", lambda v: n_frames)
            mp.setenv("WORLD_SIZE", str(world))
            decoded = []
            for rank in reversed(range(world)):
                mp.setenv("RANK", str(rank))
                ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / f"w{n_frames}"), cache_dir=str(tmp_path / f"w{n_frames}"),
                                                batch_size=2, stereo_only=True, backend=TemporalStereoBackend(), temporal_radius=R)
                got_dir = ex.process_video_sbs(sbs, max_frames=n_frames, force_reprocess=True)
                decoded.append(ex.last_decoded_frames)
                pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pw{n_frames}"), batch_size=2, stereo_only=True, guide_batch=2,
                                            backend=TemporalPipelineBackend(), temporal_radius=R)
                out4k = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pw{n_frames}.json"), max_frames=n_frames, force_reprocess=True)
        got4k = json.loads(open(out4k).read())                       # rank 0, which ran last, wrote the manifest
        blocks = [sharding.temporal_block(n_frames, r, world, R) for r in reversed(range(world))]
        assert decoded == [c + a + b if c else 0 for (_, c, a, b) in blocks]
        assert len(_pngs(want_dir)) == n_frames and _pngs(got_dir) == _pngs(want_dir), (world, n_frames)
        assert got4k["count"] == n_frames and _pngs(got4k["frames_dir"]) == _pngs(want4k["frames_dir"]), (world, n_frames)


# ---------------------------------------------------------------- quality on the temporally coherent clip

def test_stabilisation_quality_on_the_synthetic_clip():
    """320x120, 9 frames, static textured background, sigma-3 noise per frame and eye, a rectangle at d = 40 moving 6 px per
    frame, oracle matcher; R = 2, tau = 12.  The per-frame path is the yardstick:
      static-region flicker of the disparity and of the u16 samples strictly below the per-frame path's;
      the moving object's mean error against ground truth at most 5 % above the per-frame path's;
      the share of invalid pixels does not rise."""
    from video_3d_pipeline import synthetic as syn
    W, H, T, R = 320, 120, 9, 2
    L, Rt, gt = syn.temporal_clip(W, H, T)
    depth = np.stack([O.disp_to_depth(O.sgbm_compute(l, r)) for l, r in zip(L, Rt)])
    cut = TR.cuts(L, 20)
    assert not cut.any()
    stab = TR.filter_clip(depth, L, R, 12, cut, 1)
    u_frame = np.stack([O.depth_to_u16(d) for d in depth]).astype(np.int64)
    u_stab = TR.stabilize(depth, L, R).astype(np.int64)

    boxes = [syn.temporal_object_box(W, H, t) for t in range(T)]
    static = np.ones((H, W), bool)
    static[:, :64 + 8] = False                                            # the matcher's blind band
    x0, x1 = min(b[0] for b in boxes), max(b[2] for b in boxes)
    static[max(boxes[0][1] - 6, 0):boxes[0][3] + 6, max(x0 - 46, 0):x1 + 6] = False   # swept by the object or occluded by it
    both = static[None] & (depth[1:] > 0) & (depth[:-1] > 0)              # pixels the per-frame path has in both frames
    assert both.mean() > 0.3

    def flicker(a):
        return float(np.abs(a[1:] - a[:-1])[both].mean())

    f_frame, f_stab = flicker(depth), flicker(stab)
    fu_frame, fu_stab = flicker(u_frame), flicker(u_stab)
    obj = np.zeros((T, H, W), bool)
    for t, (bx0, by0, bx1, by1) in enumerate(boxes):
        obj[t, by0 + 2:by1 - 2, bx0 + 2:bx1 - 2] = True
    obj &= depth > 0
    e_frame, e_stab = float(np.abs(depth - gt)[obj].mean()), float(np.abs(stab - gt)[obj].mean())
    inv_frame, inv_stab = float((depth <= 0).mean()), float((stab <= 0).mean())
    print(f"disparity flicker {f_frame:.4f} -> {f_stab:.4f} px/frame; u16 flicker {fu_frame:.1f} -> {fu_stab:.1f} levels; "
          f"object error {e_frame:.3f} -> {e_stab:.3f} px; invalid {inv_frame:.4f} -> {inv_stab:.4f}")
    assert f_stab < f_frame and fu_stab < fu_frame
    assert e_stab <= 1.05 * e_frame
    assert inv_stab <= inv_frame


def test_scene_change_is_detected_at_the_default_threshold():
    from video_3d_pipeline import synthetic as syn
    L, _, _ = syn.temporal_clip(320, 120, 9, cut_at=5)
    sad = np.abs(L[1:].astype(np.int64) - L[:-1]).reshape(8, -1).mean(axis=1)
    print("mean absolute luma difference per pair:", np.round(sad, 1))
    assert list(TR.cuts(L, 20)) == [0, 0, 0, 0, 0, 1, 0, 0, 0]
