"""--input-layout tb on the host, without a GPU: the flag on the three CLIs, the keyword that only a top-bottom run hands to the
backend, the cache key, the eye size, the refusals, the manifest and the side file.  Stand-in backends take the place of the HIP
ones as in tests/test_host.py; the ones of the SBS runs here are the existing stand-ins, which do not know the keyword."""
import argparse
import hashlib
import json

import numpy as np
import pytest

import tb_ref
from oracle import oracle as O
from test_host import OracleStereoBackend
from test_pipeline_host import OraclePipelineBackend

SW, SH = 192, 48


class RecordingStereoBackend(OracleStereoBackend):
    """the depth stand-in that knows top-bottom frames (through tests/tb_ref.py) and records the keywords of every call"""

    def __init__(self):
        self.calls = []

    def split_sbs(self, f, unsqueeze, **kw):
        self.calls.append(("split_sbs", kw))
        return tb_ref.split(f, unsqueeze) if kw.get("input_layout") == "tb" else super().split_sbs(f, unsqueeze)

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None, **kw):
        self.calls.append(("sbs_to_disparity", kw))
        if kw.get("input_layout") != "tb":
            return super().sbs_to_disparity(frames, unsqueeze, mono_provider)
        return np.stack([O.disp_to_depth(O.sgbm_compute(*tb_ref.to_gray(f, unsqueeze))) for f in frames])


class RecordingPipelineBackend(OraclePipelineBackend, RecordingStereoBackend):
    def __init__(self):
        OraclePipelineBackend.__init__(self)
        RecordingStereoBackend.__init__(self)


@pytest.fixture()
def clips(tmp_path):
    from video_3d_pipeline import synthetic as syn
    np.save(tmp_path / "sbs.npy", np.stack([syn.sbs_frame(SW, SH, i) for i in range(3)]))
    np.save(tmp_path / "tb.npy", np.stack([syn.tb_frame(SW, SH, i) for i in range(3)]))
    np.save(tmp_path / "v4k.npy", np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(3)]))
    return str(tmp_path / "sbs.npy"), str(tmp_path / "tb.npy"), str(tmp_path / "v4k.npy")


def _extractor(tmp_path, tag, backend, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp_path / f"d_{tag}")
    return HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True, backend=backend, **kw)


def test_tb_frame_is_the_counterpart_of_sbs_frame():
    from video_3d_pipeline import synthetic as syn
    left, right = syn.stereo_pair(SW, SH, 1)
    tb = syn.tb_frame(SW, SH, 1)
    assert tb.shape == (SH, SW, 3) and tb.dtype == np.uint8 and tb.flags.c_contiguous
    mean = lambda a: ((a[0::2].astype(np.uint16) + a[1::2] + 1) >> 1).astype(np.uint8)
    assert np.array_equal(tb[:SH // 2], mean(left)) and np.array_equal(tb[SH // 2:], mean(right))      # the left eye on top


def test_the_flag_parses_on_the_three_clis(tmp_path, capsys):
    from video_3d_pipeline import depth, framematch, pipeline
    for add in (lambda p: depth.add_depth_arguments(p, "force"), framematch.add_refine_arguments):
        p = argparse.ArgumentParser()
        add(p)
        assert p.parse_args([]).input_layout == "sbs" and p.parse_args(["--input-layout", "tb"]).input_layout == "tb"
        with pytest.raises(SystemExit):
            p.parse_args(["--input-layout", "frame-sequential"])
    p = argparse.ArgumentParser()
    depth.add_depth_arguments(p, "force")
    assert "input_layout" not in depth.depth_options(p.parse_args([]))                  # an SBS run constructs everything as before
    assert depth.depth_options(p.parse_args(["--input-layout", "tb"]))["input_layout"] == "tb"
    p = argparse.ArgumentParser()
    framematch.add_refine_arguments(p)
    assert "input_layout" not in framematch.refine_options(p.parse_args([]))
    assert framematch.refine_options(p.parse_args(["--input-layout", "tb"]))["input_layout"] == "tb"
    # the CLIs themselves know it: argparse gets past the flag and fails on the clip (depth, pipeline) or runs (align, below)
    assert depth.main([str(tmp_path / "no.npy"), "--input-layout", "tb", "--stereo-only", "--device", "cpu", "--work-dir", str(tmp_path / "w")]) == 1
    assert pipeline.main([str(tmp_path / "no.npy"), str(tmp_path / "no4k.npy"), "--input-layout", "tb", "--stereo-only", "--device", "cpu",
                          "--work-dir", str(tmp_path / "w")]) == 1
    assert "unrecognized" not in capsys.readouterr().err
    with pytest.raises(ValueError, match="input_layout"):
        depth.HybridStereoDepthExtractor(work_dir=str(tmp_path / "w"), cache_dir=str(tmp_path / "w"), backend=OracleStereoBackend(), input_layout="ou")


@pytest.mark.parametrize("unsqueeze", [True, False])
def test_eye_size(unsqueeze):
    from video_3d_pipeline.depth import sbs_eye_size
    info = {"width": 1920, "height": 1080}
    assert sbs_eye_size(info, unsqueeze) == ((1920, 1080) if unsqueeze else (960, 1080))
    assert sbs_eye_size(info, unsqueeze, "sbs") == sbs_eye_size(info, unsqueeze)
    assert sbs_eye_size(info, unsqueeze, input_layout="tb") == ((1920, 1080) if unsqueeze else (1920, 540))


def test_cache_key(tmp_path):
    """an SBS run's directory is the one the key formula has always given; a top-bottom run's is another"""
    sbs = _extractor(tmp_path, "k", OracleStereoBackend())
    tb = _extractor(tmp_path, "k", OracleStereoBackend(), input_layout="tb")
    key = "movie.mp4_3_17_Intel/dpt-large_True"
    assert sbs.get_cache_path("movie.mp4", 3, 17).name == f"depth_{hashlib.md5(key.encode()).hexdigest()[:16]}"
    assert tb.get_cache_path("movie.mp4", 3, 17).name == f"depth_{hashlib.md5((key + '_tb').encode()).hexdigest()[:16]}"
    filled = _extractor(tmp_path, "k", OracleStereoBackend(), input_layout="tb", fill_holes=True, min_disparity=-16)
    from video_3d_pipeline.depth import min_disparity_suffix
    from video_3d_pipeline.temporal import fill_suffix
    suffixes = fill_suffix(True) + min_disparity_suffix(-16) + "_tb"                  # the layout comes last
    assert filled.get_cache_path("movie.mp4", 3, 17).name == f"depth_{hashlib.md5((key + suffixes).encode()).hexdigest()[:16]}"


def test_an_sbs_run_hands_the_backend_no_keyword_and_a_tb_run_does(tmp_path, clips):
    from video_3d_pipeline.utils import read_png16
    sbs, tb, _ = clips
    plain = OracleStereoBackend()                                    # does not accept the keyword: an SBS run must not pass it
    out_plain = _extractor(tmp_path, "plain", plain).process_video_sbs(sbs)
    rec = RecordingStereoBackend()
    ex = _extractor(tmp_path, "sbs", rec)
    out_sbs = ex.process_video_sbs(sbs)
    ex.split_sbs_frame(np.load(sbs)[0])
    assert rec.calls and all(kw == {} for _, kw in rec.calls)
    assert out_sbs.name == out_plain.name and sorted(p.name for p in out_sbs.iterdir()) == [f"depth_{i:06d}.png" for i in range(3)]
    assert ex.manifest_extra() == {} and ex.eye_size({"width": SW, "height": SH}) == (SW, SH)

    rec = RecordingStereoBackend()
    ex = _extractor(tmp_path, "tb", rec, input_layout="tb")
    out_tb = ex.process_video_sbs(tb)
    assert [c for c in rec.calls if c[0] == "sbs_to_disparity"] and all(kw == {"input_layout": "tb"} for _, kw in rec.calls)
    assert out_tb.name != out_sbs.name
    assert sorted(p.name for p in out_tb.iterdir()) == [f"depth_{i:06d}.png" for i in range(3)] + ["input_layout.json"]
    assert json.loads((out_tb / "input_layout.json").read_text()) == {"input_layout": "tb"}
    assert ex.manifest_extra() == {"input_layout": "tb"}
    frames = np.load(tb)
    want = O.depth_to_u16(O.disp_to_depth(O.sgbm_compute(*tb_ref.to_gray(frames[1], True))))
    assert np.array_equal(read_png16(out_tb / "depth_000001.png"), want) and want.shape == (SH, SW)
    L, R = ex.split_sbs_frame(frames[0])
    assert L.shape == (SH, SW, 3) and np.array_equal(R, tb_ref.split(frames[0], True)[1]) and rec.calls[-1] == ("split_sbs", {"input_layout": "tb"})
    assert ex.split_sbs_frame(frames[0], unsqueeze=False)[0].shape == (SH // 2, SW, 3)


def test_an_odd_height_is_refused_for_tb_only(tmp_path):
    tb = _extractor(tmp_path, "odd", RecordingStereoBackend(), input_layout="tb")
    with pytest.raises(ValueError, match="top-bottom frame height must be even"):
        tb.split_sbs_frame(np.zeros((7, 8, 3), np.uint8))
    assert tb.split_sbs_frame(np.zeros((8, 7, 3), np.uint8))[0].shape == (8, 7, 3)      # an odd width is fine top-bottom
    np.save(tmp_path / "odd.npy", np.zeros((2, 7, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="top-bottom frame height must be even"):
        tb.process_video_sbs(str(tmp_path / "odd.npy"))
    sbs = _extractor(tmp_path, "odd_sbs", RecordingStereoBackend())
    with pytest.raises(ValueError, match="SBS frame width must be even"):
        sbs.split_sbs_frame(np.zeros((8, 7, 3), np.uint8))


def test_pipeline_manifest_carries_the_layout_only_for_tb(tmp_path, clips):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs, tb, v4k = clips
    mans = {}
    for tag, clip, kw in (("sbs", sbs, {}), ("tb", tb, {"input_layout": "tb"})):
        be = RecordingPipelineBackend() if kw else OraclePipelineBackend()
        pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"p_{tag}"), batch_size=2, stereo_only=True, backend=be, **kw)
        out = pipe.run(clip, v4k, output_path=str(tmp_path / f"{tag}.json"))
        mans[tag] = json.loads(open(out).read())
        if kw:
            assert all(k == kw for name, k in be.calls if name == "sbs_to_disparity") and be.calls
    assert "input_layout" not in mans["sbs"] and mans["tb"]["input_layout"] == "tb"
    assert mans["tb"]["count"] == mans["sbs"]["count"] == 3


def test_upscale_cli_carries_the_side_file_into_its_manifest(tmp_path):
    from video_3d_pipeline.upscale import input_layout_entry
    assert input_layout_entry(tmp_path) == {}
    (tmp_path / "input_layout.json").write_text(json.dumps({"input_layout": "tb"}))
    assert input_layout_entry(tmp_path) == {"input_layout": "tb"}
    (tmp_path / "input_layout.json").write_text("not json")
    assert input_layout_entry(tmp_path) == {}


def _block_file(tmp_path, name, **over):
    block = dict(status="registered", map=[1.0, 0.0, 0.875, 0.0625], eye_size=[SW, SH], guide_size=[2 * SW, 2 * SH], unsqueeze=True)
    block.update(over)
    f = tmp_path / name
    f.write_text(json.dumps({"time_offset_seconds": 0.0, "guide_start_frame": 0, "spatial": block}))
    return str(f)


def test_resolve_refuses_a_layout_mismatch(tmp_path):
    from video_3d_pipeline import register as R
    sizes = dict(eye_size=(SW, SH), guide_size=(2 * SW, 2 * SH), unsqueeze=True)
    sbs_block, tb_block = _block_file(tmp_path, "s.json"), _block_file(tmp_path, "t.json", input_layout="tb")
    assert R.resolve(sbs_block, **sizes)["map"] == R.resolve(tb_block, input_layout="tb", **sizes)["map"] == (1.0, 0.0, 0.875, 0.0625)
    with pytest.raises(ValueError, match="estimated with input_layout=tb, this run has input_layout=sbs"):
        R.resolve(tb_block, **sizes)
    with pytest.raises(ValueError, match="estimated with input_layout=sbs, this run has input_layout=tb"):
        R.resolve(sbs_block, input_layout="tb", **sizes)
    # a caller that does not split the clip itself (the upscale CLI: sizes from the depth maps) compares nothing
    assert R.resolve(tb_block, eye_size=(SW, SH))["map"] == (1.0, 0.0, 0.875, 0.0625)
    assert R.resolve(tb_block, no_spatial=True, **sizes) is None


class TbAlignBackend:
    """the stand-in of the align CLI's refinement and registration for top-bottom clips whose left eye is the top half"""

    def __init__(self):
        import framematch_ref as FR
        import register_ref as RR
        self.FR, self.RR, self.calls = FR, RR, []

    def _left(self, frames, unsqueeze, kw):
        assert not unsqueeze and kw == {"input_layout": "tb"}
        return np.stack([f[:f.shape[0] // 2, :, 0] for f in frames])

    def sbs_left_signatures(self, frames, unsqueeze, **kw):
        self.calls.append("signatures")
        return self.FR.signature(self._left(frames, unsqueeze, kw))

    def sbs_left_profiles(self, frames, unsqueeze, **kw):
        self.calls.append("profiles")
        return self.RR.profiles(self._left(frames, unsqueeze, kw))

    def guide_signatures(self, frames, height, width):
        return self.FR.signature(np.stack([f[..., 0] for f in frames]))

    def guide_profiles(self, frames, height, width):
        return self.RR.profiles(np.stack([f[..., 0] for f in frames]))

    def signature_scores(self, a, b):
        return self.FR.scores(a, b)

    def read_scores(self, handle):
        return handle

    def match_scores(self, prof_a, prof_b, cand, bins):
        return self.RR.match_scores(prof_a, prof_b, cand, bins)


def test_align_cli_reads_the_top_eye_and_records_the_layout(tmp_path):
    import framematch_ref as FR
    from video_3d_pipeline import align, register as R
    left, guide = FR.match_clips(128, 72, 24, speed=6, delay=3)
    np.save(tmp_path / "tb.npy", np.repeat(np.concatenate([left, left], axis=1)[..., None], 3, axis=3))     # full top-bottom: 128 x 144
    np.save(tmp_path / "g.npy", np.repeat(guide[..., None], 3, axis=3))
    be = TbAlignBackend()
    rc = align.main([str(tmp_path / "tb.npy"), str(tmp_path / "g.npy"), "--work-dir", str(tmp_path / "w"), "--video-only", "--no-unsqueeze",
                     "--refine-window", "12", "--refine-min-score", "0.5", "--refine-min-margin", "0.01", "--register-spatial",
                     "--input-layout", "tb"], backend=be)
    data = json.loads((tmp_path / "w" / "alignment_data.json").read_text())
    assert rc == 0 and "signatures" in be.calls and "profiles" in be.calls
    assert data["guide_start_frame"] == 3 and data["visual_parameters"]["input_layout"] == "tb"
    assert data["spatial"]["input_layout"] == "tb" and data["spatial"]["eye_size"] == [128, 72]
    if data["spatial"]["status"] == "registered" and tuple(data["spatial"]["map"]) != R.IDENTITY:
        with pytest.raises(ValueError, match="input_layout=tb"):
            R.resolve(str(tmp_path / "w" / "alignment_data.json"), unsqueeze=False)


def test_convert_refuses_source_fill_from_a_tb_source(tmp_path, capsys):
    from test_source_parallax_host import SourceRenderBackend
    from video_3d_pipeline import convert
    from video_3d_pipeline.utils import write_png16
    W, H = 64, 32
    np.save(tmp_path / "v4k.npy", np.zeros((2, H, W, 3), np.uint8))
    np.save(tmp_path / "tb.npy", np.zeros((2, H // 2, W // 2, 3), np.uint8))
    frames = tmp_path / "d_frames"
    frames.mkdir()
    for i in range(2):
        write_png16(frames / f"depth4k_{i:06d}.png", np.full((H, W), 1000 * i, np.uint16))
    block = {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": W // 2}

    def run(name, extra, *flags):
        (tmp_path / name).write_text(json.dumps({"format": "png16-sequence", "frames_dir": str(frames), "count": 2, "depth_range": block, **extra}))
        be = SourceRenderBackend()
        rc = convert.main([str(tmp_path / "v4k.npy"), str(tmp_path / name), "--output", str(tmp_path / (name + ".out.json")),
                           "--parallax", "source", *flags], backend=be)
        return rc, be.calls, capsys.readouterr().out
    rc, calls, out = run("tb.json", {"input_layout": "tb"}, "--fill-from-source", str(tmp_path / "tb.npy"))
    assert rc == 1 and not calls and "--fill-from-source cannot read a top-bottom source" in out and "rows, not columns" in out
    rc, calls, _ = run("tb_plain.json", {"input_layout": "tb"})              # --parallax source alone needs only the manifest
    assert rc == 0 and calls == [None]
    rc, calls, _ = run("sbs.json", {}, "--fill-from-source", str(tmp_path / "tb.npy"))
    assert rc == 0 and len(calls) == 1 and calls[0] is not None              # the same request with an SBS run's manifest goes through
