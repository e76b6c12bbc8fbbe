"""Host side of --fill-holes on CPU: with the flag off the backend sees exactly the calls it saw before (the stand-ins of the
existing host tests take no new keyword and no new method: either would be a TypeError / AttributeError here), the cache key,
the manifest and the directory are unchanged; with it on the stage runs once per device pass on the int16 disparity before the
depth conversion, the key gains `_fill1`, the manifest `"fill_holes": true` and the directory `fill.json`."""
import hashlib
import json
import os

import numpy as np
import pytest

import fill_ref as FR
import range_ref as RR
from oracle import oracle as O
from test_host import OracleStereoBackend, OracleUpscaleBackend
from test_pipeline_host import OraclePipelineBackend
from test_range_host import RangePipelineBackend, RangeStereoBackend
from test_temporal_host import NF, _depth_cli, _pipeline, _pngs, clips  # noqa: F401  (clips: the module's fixture)


class _FillMethods:
    """what HipStereoBackend widens for the flag, NumPy: the oracle disparity, filled by the reference before /16 or the blend"""

    def _disp(self, left, right, fill_holes):
        d = O.sgbm_compute(left, right)
        return FR.fill_frame(d) if fill_holes else d

    def pairs_to_disparity(self, pairs, monos=None, fill_holes=False):
        self.__dict__.setdefault("calls", []).append(("pairs", len(pairs), monos is not None, fill_holes))
        disps = [self._disp(O.bgr_to_gray(l), O.bgr_to_gray(r), fill_holes) for l, r in pairs]
        if monos is None:
            return [O.disp_to_depth(d) for d in disps]
        return [O.mono_blend(d, np.asarray(m, np.float32)) for d, m in zip(disps, monos)]

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None, fill_holes=False):
        self.__dict__.setdefault("calls", []).append(("sbs", len(frames), mono_provider is not None, fill_holes))
        self._lg = np.stack([O.sbs_to_gray(f, unsqueeze)[0] for f in frames])
        out = []
        for f in frames:
            d = self._disp(*O.sbs_to_gray(f, unsqueeze), fill_holes)
            if mono_provider is None:
                out.append(O.disp_to_depth(d))
            else:
                left_rgb = O.split_sbs(f, unsqueeze)[0][..., ::-1]
                out.append(O.mono_blend(d, np.asarray(mono_provider([left_rgb])[0], np.float32)))
        return np.stack(out)


class FillStereoBackend(_FillMethods, RangeStereoBackend):
    pass


class FillPipelineBackend(_FillMethods, RangePipelineBackend):
    pass


def _maps(d, n=NF):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), f"depth_{i:06d}.png")) for i in range(n)])


def _oracle_clip(sbs, fill):
    """(depth f32 [n,H,W], left gray [n,H,W]) of the clip through the oracle matcher, the disparity filled by the reference"""
    from video_3d_pipeline.utils import iter_frames
    depth, gray = [], []
    for f in iter_frames(sbs):
        l, r = O.sbs_to_gray(f, True)
        d = O.sgbm_compute(l, r)
        depth.append(O.disp_to_depth(FR.fill_frame(d) if fill else d))
        gray.append(l)
    return np.stack(depth), np.stack(gray)


# ---------------------------------------------------------------- the option itself

def test_suffix_options_and_constructor_check():
    import argparse
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.temporal import add_fill_arguments, fill_options, fill_suffix
    assert fill_suffix(False) == "" and fill_suffix(True) == "_fill1"
    p = argparse.ArgumentParser()
    add_fill_arguments(p)
    assert fill_options(p.parse_args([])) == {"fill_holes": False}
    assert fill_options(p.parse_args(["--fill-holes"])) == {"fill_holes": True}
    for bad in (1, "yes", None):
        with pytest.raises(ValueError):
            HybridStereoDepthExtractor(work_dir="unused", backend=OracleStereoBackend(), fill_holes=bad)


def test_cache_key(tmp_path):
    """off: the reference's key, byte for byte; on: `_fill1` after the temporal and range suffixes"""
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.temporal import cache_suffix

    def name(**kw):
        ex = HybridStereoDepthExtractor(work_dir=str(tmp_path), cache_dir=str(tmp_path), backend=OracleStereoBackend(), **kw)
        return ex.get_cache_path("clip.npy", 3, 40).name

    def md5(suffix):
        return "depth_" + hashlib.md5(f"clip.npy_3_40_Intel/dpt-large_True{suffix}".encode()).hexdigest()[:16]

    assert name() == name(fill_holes=False) == md5("")                                      # the reference-compatible key
    assert name(fill_holes=True) == md5("_fill1")
    both = cache_suffix(2, 12, 20, True, 9800)
    assert name(temporal_radius=2, range_percentile=98) == name(temporal_radius=2, range_percentile=98, fill_holes=False) == md5(both)
    assert name(temporal_radius=2, range_percentile=98, fill_holes=True) == md5(both + "_fill1")


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
            assert mod.main(argv + ["--fill-holes", "--temporal-radius", "1", "--range-percentile", "99"]) == 1
            assert (seen["fill_holes"], seen["temporal_radius"], seen["range_percentile"]) == (True, 1, 99.0)
            seen.clear()
            assert mod.main(argv) == 1
            assert seen["fill_holes"] is False
        finally:
            setattr(mod, name, orig)
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    assert SbsTo4kDepthPipeline(work_dir="unused", backend=FillPipelineBackend(), fill_holes=True).extractor.fill_holes is True
    assert SbsTo4kDepthPipeline(work_dir="unused", backend=OraclePipelineBackend()).extractor.fill_holes is False


# ---------------------------------------------------------------- flag off: nothing changes

def test_flag_off_changes_nothing(tmp_path, clips):
    """the parent's stand-ins (no `fill_holes` keyword anywhere: passing one raises) with the flag spelt out as False against
    the default construction: same directory names, same files byte for byte, no manifest key, no side file"""
    sbs, v4k = clips
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", OracleStereoBackend())
    _, off_dir = _depth_cli(tmp_path, sbs, "off", OracleStereoBackend(), fill_holes=False)
    assert off_dir.name == plain_dir.name
    assert sorted(os.listdir(off_dir)) == sorted(os.listdir(plain_dir)) == [f"depth_{i:06d}.png" for i in range(NF)]
    assert _pngs(off_dir) == _pngs(plain_dir)
    depth, _ = _oracle_clip(sbs, False)
    assert np.array_equal(_maps(off_dir), np.stack([O.depth_to_u16(d) for d in depth]))
    _, plain = _pipeline(tmp_path, sbs, v4k, "plain", OraclePipelineBackend(), run_kw=dict(keep_depth_maps=True))
    pipe, off = _pipeline(tmp_path, sbs, v4k, "off", OraclePipelineBackend(), run_kw=dict(keep_depth_maps=True), fill_holes=False)
    assert "fill_holes" not in off and set(off) == set(plain)
    assert _pngs(off["frames_dir"]) == _pngs(plain["frames_dir"]) and len(_pngs(off["frames_dir"])) == NF
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == plain_dir.name and _pngs(cache) == _pngs(plain_dir) and not (cache / "fill.json").exists()
    # with the other two options on and this one off: their stand-ins, which know no `fill_holes` either
    _, r_plain = _depth_cli(tmp_path, sbs, "rplain", RangeStereoBackend(), temporal_radius=1, range_percentile=99)
    _, r_off = _depth_cli(tmp_path, sbs, "roff", RangeStereoBackend(), temporal_radius=1, range_percentile=99, fill_holes=False)
    assert r_off.name == r_plain.name and sorted(os.listdir(r_off)) == sorted(os.listdir(r_plain)) and _pngs(r_off) == _pngs(r_plain)
    assert not (r_off / "fill.json").exists()


def test_flag_off_process_frame_batch_is_todays_call():
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    pairs = [O.split_sbs(syn.sbs_frame(192, 48, i), True) for i in range(2)]
    ex = HybridStereoDepthExtractor(work_dir="unused", stereo_only=True, backend=OracleStereoBackend(), fill_holes=False)
    maps = ex.process_frame_batch(pairs)
    want = OracleStereoBackend().pairs_to_disparity(pairs)
    assert all(np.array_equal(a, b) for a, b in zip(maps, want))


# ---------------------------------------------------------------- flag on

def test_depth_cli_fills_before_the_depth_conversion(tmp_path, clips):
    sbs, _ = clips
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", OracleStereoBackend())
    be = FillStereoBackend()
    ex, ddir = _depth_cli(tmp_path, sbs, "on", be, fill_holes=True)
    assert ddir.name != plain_dir.name
    assert json.loads((ddir / "fill.json").read_text()) == {"fill_holes": True} and not (ddir / "temporal.json").exists()
    # once per device pass (batch_size 3 over 7 frames), always with the flag, nothing else new
    assert be.calls == [("sbs", 3, False, True), ("sbs", 3, False, True), ("sbs", 1, False, True)]
    depth, _ = _oracle_clip(sbs, True)
    got = _maps(ddir)
    assert np.array_equal(got, np.stack([O.depth_to_u16(d) for d in depth]))
    assert (got != _maps(plain_dir)).any()
    holes = (_oracle_clip(sbs, False)[0] == 0).sum()           # invalid pixels (and the few valid zeros) of the unfilled clip
    assert holes > 64 * 48 * NF and (depth == 0).sum() < holes // 100


def test_one_pass_pipeline_writes_the_depth_clis_files(tmp_path, clips):
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    sbs, v4k = clips
    _, ddir = _depth_cli(tmp_path, sbs, "on", FillStereoBackend(), fill_holes=True)
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    out = up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / "cli.json"))
    want4k = _pngs(json.loads(open(out).read())["frames_dir"])
    be = FillPipelineBackend()
    pipe, man = _pipeline(tmp_path, sbs, v4k, "on", be, run_kw=dict(keep_depth_maps=True), fill_holes=True)
    assert man["fill_holes"] is True and "temporal" not in man and man["count"] == NF
    assert len(want4k) == NF and _pngs(man["frames_dir"]) == want4k
    assert [c[3] for c in be.calls] == [True] * 3
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)
    assert json.loads((cache / "fill.json").read_text()) == {"fill_holes": True}
    # without --keep-depth-maps no depth directory is written, so no side file either
    pipe2, man2 = _pipeline(tmp_path, sbs, v4k, "on2", FillPipelineBackend(), fill_holes=True)
    assert man2["fill_holes"] is True and _pngs(man2["frames_dir"]) == want4k
    assert not (pipe2.extractor.get_cache_path(sbs, 0, NF) / "fill.json").exists()


def test_flag_combines_with_the_temporal_stage_and_the_robust_range(tmp_path, clips):
    sbs, v4k = clips
    ex, ddir = _depth_cli(tmp_path, sbs, "all", FillStereoBackend(), fill_holes=True, temporal_radius=1, range_percentile=99)
    _, nofill = _depth_cli(tmp_path, sbs, "nofill", RangeStereoBackend(), temporal_radius=1, range_percentile=99)
    assert ddir.name != nofill.name
    entry = {"radius": 1, "tau": 12, "cut_threshold": 20, "fill": True, "range_quantile": 9900}
    assert json.loads((ddir / "temporal.json").read_text()) == entry == json.loads((nofill / "temporal.json").read_text())
    assert json.loads((ddir / "fill.json").read_text()) == {"fill_holes": True}
    depth, gray = _oracle_clip(sbs, True)
    assert np.array_equal(_maps(ddir), RR.stabilize(depth, gray, 1, q=9900))
    pipe, man = _pipeline(tmp_path, sbs, v4k, "all", FillPipelineBackend(), run_kw=dict(keep_depth_maps=True), fill_holes=True,
                          temporal_radius=1, range_percentile=99)
    assert man["fill_holes"] is True and man["temporal"] == entry
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)


def test_process_frame_batch_honours_the_flag():
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    pairs = [O.split_sbs(syn.sbs_frame(192, 48, i), True) for i in range(2)]
    be = FillStereoBackend()
    ex = HybridStereoDepthExtractor(work_dir="unused", stereo_only=True, backend=be, fill_holes=True)
    maps = ex.process_frame_batch(pairs)
    assert be.calls == [("pairs", 2, False, True)]
    for (l, r), m in zip(pairs, maps):
        d = O.sgbm_compute(O.bgr_to_gray(l), O.bgr_to_gray(r))
        assert (d < 0).any() and (FR.fill_frame(d) >= 0).all() and np.array_equal(m, O.disp_to_depth(FR.fill_frame(d)))
    # with neural guidance the maps are blended into the FILLED disparity
    mono = lambda lefts: [np.full((6, 8), 2.0, np.float32) + np.arange(8, dtype=np.float32) for _ in lefts]
    be = FillStereoBackend()
    ex = HybridStereoDepthExtractor(work_dir="unused", backend=be, mono_provider=mono, fill_holes=True)
    maps = ex.process_frame_batch(pairs)
    assert be.calls == [("pairs", 2, True, True)]
    d = O.sgbm_compute(O.bgr_to_gray(pairs[0][0]), O.bgr_to_gray(pairs[0][1]))
    assert np.array_equal(maps[0], O.mono_blend(FR.fill_frame(d), mono([None])[0]))


# ---------------------------------------------------------------- HipStereoBackend: where the stage sits

class _FakeLib:
    def v3d_fill_holes_ws_bytes(self, n, H):
        return (n * H + 15) // 16 * 16


class _FakeNative:
    """records the order of the native calls of one pass; tensors are CPU tensors"""

    def __init__(self, timeouts=0):
        self.log, self.timeouts = [], timeouts
        outer = self

        class StereoSGBM:
            def __init__(self, W, H, n, device=None, **params):
                pass

            def compute(self, lg, rg, out=None):
                outer.log.append("compute")
                out.fill_(-16)
                return out

            def sync_errors(self):
                outer.timeouts, n = max(outer.timeouts - 1, 0), outer.timeouts
                return n

            def set_lockstep(self, enable):
                outer.log.append("lockstep-off")

            def close(self):
                pass

        self.StereoSGBM = StereoSGBM

    def lib(self):
        return _FakeLib()

    def sbs_to_gray_batch(self, dev, unsqueeze, out):
        self.log.append("gray")

    def fill_holes_disp16_batch(self, disp, out=None, ws=None):
        assert out is disp and ws.numel() >= 16 and ws.numel() >= disp.shape[0] * disp.shape[1]
        self.log.append("fill")
        return disp

    def disp_to_depth(self, disp, out=None):
        self.log.append("depth")
        return out

    def mono_blend(self, disp, mono, ws, wm, out):
        self.log.append("blend")

    def split_sbs(self, frame, unsqueeze):
        import torch
        return torch.zeros((4, 8, 3), dtype=torch.uint8), None


def _hip_backend(native):
    import torch
    from video_3d_pipeline.depth import HipStereoBackend

    class Backend(HipStereoBackend):
        def __init__(self):
            self.torch, self.native, self.device = torch, native, torch.device("cpu")
            self.sgbm_params, self._matcher, self._geom = {}, None, None

        def _staging(self, key, shape, dtype, pinned):                    # no pinned memory on a CPU-only box
            return super()._staging(key, shape, dtype, False)

    return Backend()


def test_hip_backend_runs_the_stage_after_the_matcher_and_before_the_depth(capsys):
    frames = [np.zeros((4, 16, 3), np.uint8)] * 2
    nat = _FakeNative()
    _hip_backend(nat).sbs_to_disparity(frames, True)
    assert nat.log == ["gray", "compute", "depth"]                         # flag off: today's sequence
    nat = _FakeNative()
    be = _hip_backend(nat)
    be.sbs_to_disparity(frames, True, fill_holes=True)
    be.sbs_to_disparity(frames, True, fill_holes=True)
    assert nat.log == ["gray", "compute", "fill", "depth"] * 2             # once per pass
    assert be._bufs["fill_ws"].numel() == 16
    nat = _FakeNative(timeouts=1)                                          # the lock-step recompute comes first
    _hip_backend(nat).sbs_to_disparity(frames, True, fill_holes=True)
    assert nat.log == ["gray", "compute", "lockstep-off", "compute", "fill", "depth"]
    nat = _FakeNative()                                                    # the hybrid blend reads the filled disparity
    import torch
    _hip_backend(nat).sbs_to_disparity(frames, True, lambda lefts: [torch.ones((2, 2)) for _ in lefts], fill_holes=True)
    assert nat.log == ["gray", "compute", "fill", "blend"]
    capsys.readouterr()
