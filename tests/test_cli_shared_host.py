"""The three pieces the CLIs and the one-pass pipeline share, on the CPU with the stand-in backends of the other host tests:
convert.StereoPlan through both of its routes (the convert CLI, the pipeline's --stereo-output), --guide-start-frame |
--alignment-file of the three parsers (align.add_guide_arguments / resolve_guide_start), and utils.finish_sequence under
encode_depth4k and finish_stereo_output."""
import json
import re

import numpy as np
import pytest

import register_ref as RR
from test_convert_host import H4, W4, RefRenderBackend, RefStereoPipelineBackend, _pngs
from test_pipeline_host import SH, SW
from test_source_parallax_host import SourceRenderBackend, _PackPipelineBackend

N_FRAMES = 3
SPATIAL_MAP = "1,0,0.875,0.0625"


class WarpPackPipelineBackend(_PackPipelineBackend):
    """the metric pipeline stand-in whose render_stereo knows every layout, plus the warp of --spatial-map"""

    def warp_u16(self, u16, q, size):
        return RR.warp(np.asarray(u16).view(np.uint16), *q, 0, *size)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    tmp = tmp_path_factory.mktemp("shared")
    np.save(tmp / "sbs.npy", np.stack([syn.sbs_frame(SW, SH, i) for i in range(N_FRAMES)]))
    np.save(tmp / "v4k.npy", np.random.default_rng(7).integers(0, 256, (N_FRAMES + 1, H4, W4, 3), dtype=np.uint8))
    return tmp, str(tmp / "sbs.npy"), str(tmp / "v4k.npy")


# ------------------------------------------------------------------------------------------------------------------------
# the plan, both routes
# ------------------------------------------------------------------------------------------------------------------------
SETTINGS = {
    # tag: (stereo flags of both CLIs, depth flags of the pipeline, pipeline stand-in, convert stand-in)
    "default": ([], [], RefStereoPipelineBackend, RefRenderBackend),          # stand-ins that take no optional keyword at all
    "half-tb-subpixel": (["--layout", "half-tb", "--subpixel"], [], WarpPackPipelineBackend, SourceRenderBackend),
    "source": (["--parallax", "source", "--parallax-gain", "1.5"], ["--depth-range", "metric", "--spatial-map", SPATIAL_MAP],
               WarpPackPipelineBackend, SourceRenderBackend),
}


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_plan_gives_both_routes_the_same_manifest(clips, tag, monkeypatch, capsys):
    from video_3d_pipeline import convert, pipeline
    tmp, sbs, v4k = clips
    flags, depth_flags, pipe_backend, render_backend = SETTINGS[tag]
    monkeypatch.setattr(pipeline, "HipPipelineBackend", lambda device: pipe_backend())
    depth_out, got_path, want_path = tmp / f"depth_{tag}.json", tmp / f"pipe3d_{tag}.json", tmp / f"cli3d_{tag}.json"
    assert pipeline.main([sbs, v4k, "--output", str(depth_out), "--stereo-output", str(got_path), "--work-dir", str(tmp / f"w_{tag}"),
                          "--stereo-only", "--batch-size", "2", "--guide-start-frame", "1"] + flags + depth_flags) == 0
    pipe_said = capsys.readouterr().out
    assert convert.main([v4k, str(depth_out), "--output", str(want_path), "--guide-start-frame", "1"] + flags,
                        backend=render_backend()) == 0
    cli_said = capsys.readouterr().out
    got, want = json.loads(got_path.read_text()), json.loads(want_path.read_text())
    assert list(got) == list(want)                                     # the same keys in the same order
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    assert got["frames_dir"] != want["frames_dir"] and got["count"] == N_FRAMES
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"]) and len(_pngs(got["frames_dir"])) == N_FRAMES + 1     # + info.json
    lines = [re.findall(r"^Source parallax: .*$", said, re.M) for said in (pipe_said, cli_said)]
    assert lines[0] == lines[1] and len(lines[0]) == (1 if tag == "source" else 0)
    if tag == "default":
        assert list(got) == ["format", "frames_dir", "pattern", "count", "width", "height", "fps", "layout", "max_shift", "convergence",
                             "eye_split", "gain_left", "gain_right", "conv", "note"]
    if tag == "half-tb-subpixel":
        assert list(got)[-2:] == ["note", "subpixel"] and (got["layout"], got["width"], got["height"]) == ("half-tb", W4, H4)
    if tag == "source":
        assert list(got)[-4:] == ["note", "parallax", "parallax_scale", "parallax_gain"]
        assert got["parallax_scale"] == W4 / SW and got["parallax_gain"] == 1.5 and got["eye_split"] == 0     # Ax = 1: the map's x scale
        assert lines[0][0].startswith(f"Source parallax: {W4 / SW:g} 4K px per matcher px x gain 1.5 -> gains (0, ")


def test_plan_is_what_the_converter_holds():
    from video_3d_pipeline.convert import DepthTo3DConverter, StereoPlan, stereo_settings
    conv = DepthTo3DConverter(max_shift=20, eye_split=0.25, layout="half-sbs", subpixel=True, backend=RefRenderBackend())
    plan = conv.plan
    assert isinstance(plan, StereoPlan) and conv.params is plan.params and conv.gains == plan.gains
    assert (conv.layout_code, conv.gains) == stereo_settings(20, 0.5, 0.25, "half-sbs") and plan.render_kwargs() == {"subpixel": True}
    assert (conv.subpixel, conv.parallax, conv.parallax_gain, conv.spatial_map) == (True, "invented", 1.0, None)
    assert StereoPlan().render_kwargs() == {} and StereoPlan().source_kwargs(None, (W4, H4)) == {}
    plan.check_frame(W4, H4)
    assert plan.size == (W4, H4)
    for layout, size, text in (("half-sbs", (W4 + 1, H4), "half SBS needs an even frame width"),
                               ("half-tb", (W4, H4 + 1), "half top-bottom needs an even frame height")):
        with pytest.raises(ValueError, match=text):
            StereoPlan(layout=layout).check_frame(*size)
    for bad in (dict(layout="anaglyph"), dict(subpixel="yes"), dict(parallax="film"), dict(parallax="source", parallax_gain=-2),
                dict(max_shift=-1), dict(fill_from_source="s.npy")):
        with pytest.raises(ValueError):
            StereoPlan(**bad)
    src = StereoPlan(parallax="source", parallax_gain=2.0)
    assert src.gains is None
    block = {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": SW}
    assert src.resolve_source(block, W4, (0.5, 0.25, 1.0, 0.0)) == src.gains and src.spatial_map == (0.5, 0.25, 1.0, 0.0)
    assert (src.params["parallax_scale"], src.params["parallax_gain"], src.params["eye_split"]) == (2 * W4 / SW, 2.0, 0.0)


# ------------------------------------------------------------------------------------------------------------------------
# --guide-start-frame | --alignment-file
# ------------------------------------------------------------------------------------------------------------------------
def _stubbed_mains(monkeypatch, tmp_path):
    """the three mains with their drivers replaced: -> {name: (run(*flags) -> return code, what the driver was called with)}"""
    from video_3d_pipeline import convert, pipeline, upscale
    seen = {"upscale": {}, "pipeline": {}, "convert": {}}

    def stub(name):
        class Stub:
            def __init__(self, **kw):
                pass

            def _call(self, *a, **kw):
                seen[name].update(kw)
                return "out.json"
            process_depth_upscaling = run = process_conversion = _call
        return Stub
    monkeypatch.setattr(upscale, "SimpleDepthUpscaler", stub("upscale"))
    monkeypatch.setattr(pipeline, "SbsTo4kDepthPipeline", stub("pipeline"))
    monkeypatch.setattr(convert, "DepthTo3DConverter", stub("convert"))
    np.savez(tmp_path / "k4.npz", frames=np.zeros((3, 8, 16, 3), np.uint8), fps=25.0)
    k4 = str(tmp_path / "k4.npz")
    return {"upscale": lambda *flags: upscale.main([str(tmp_path), k4, *flags]),
            "pipeline": lambda *flags: pipeline.main(["sbs.npy", k4, *flags]),
            "convert": lambda *flags: convert.main([k4, str(tmp_path), *flags])}, seen


def test_the_three_parsers_share_the_guide_offset(tmp_path, monkeypatch, capsys):
    mains, seen = _stubbed_mains(monkeypatch, tmp_path)
    good, negative, absent = tmp_path / "al.json", tmp_path / "neg.json", tmp_path / "absent.json"
    good.write_text(json.dumps({"video1_path": "s", "video2_path": "k", "time_offset_seconds": 1.23, "video1_fps": 24.0}))
    negative.write_text(json.dumps({"video1_path": "s", "video2_path": "k", "time_offset_seconds": -0.5, "video1_fps": 24.0}))
    said = {}
    for name, run in mains.items():
        with pytest.raises(SystemExit) as e:                           # both flags: argparse's own refusal
            run("--guide-start-frame", "3", "--alignment-file", str(good))
        assert e.value.code == 2 and not seen[name], name
        capsys.readouterr()
        assert run("--alignment-file", str(good)) == 0 and seen[name]["guide_start_frame"] == 31, name      # round(1.23 s * 25 fps)
        assert f"Alignment file {good}: --guide-start-frame 31\n" in capsys.readouterr().out
        assert run("--guide-start-frame", "7") == 0 and seen[name]["guide_start_frame"] == 7
        assert run() == 0 and seen[name]["guide_start_frame"] == 0
        seen[name].clear()
        capsys.readouterr()
        errors = []
        for f in (absent, negative):
            assert run("--alignment-file", str(f)) == 1 and not seen[name], (name, f)
            out = capsys.readouterr().out
            assert out.startswith("Error: ") and out.count("\n") == 1, out
            errors.append(out)
        assert "--start-frame 12 " in errors[1]                       # round(0.5 s * 24 fps on the SBS side)
        said[name] = errors
    assert said["upscale"] == said["pipeline"] == said["convert"]


# ------------------------------------------------------------------------------------------------------------------------
# the finisher
# ------------------------------------------------------------------------------------------------------------------------
def _finishers(tmp_path):
    """the two builders of a manifest over one frames directory: -> {pattern: (call(output path), the manifest it builds)}"""
    from video_3d_pipeline.convert import finish_stereo_output
    from video_3d_pipeline.upscale import encode_depth4k
    d = tmp_path / "x_frames"
    params = dict(max_shift=48.0, convergence=0.5, eye_split=0.5, layout="full-sbs", subpixel=True)
    depth = {"format": "png16-sequence", "frames_dir": str(d), "pattern": "depth4k_%06d.png", "count": 3, "width": 8, "height": 4,
             "fps": 25.0, "guided_radius": 8, "guided_eps": 0.001, "fill_holes": True,
             "note": "no ffmpeg binary on this host: 4K depth frames kept as 16-bit PNGs"}
    stereo = {"format": "png8-rgb-sequence", "frames_dir": str(d), "pattern": "frame_%06d.png", "count": 3, "width": 16, "height": 4,
              "fps": 25.0, "layout": "full-sbs", "max_shift": 48.0, "convergence": 0.5, "eye_split": 0.5, "gain_left": 6144,
              "gain_right": -6144, "conv": 32768, "note": "no ffmpeg binary on this host: side-by-side frames kept as 8-bit RGB PNGs",
              "subpixel": True}
    return d, {"depth4k_%06d.png": (lambda out: encode_depth4k(d, out, 3, 8, 4, 25.0, 8, 1e-3, {"fill_holes": True}), depth),
               "frame_%06d.png": (lambda out: finish_stereo_output(d, out, 3, 16, 4, 25.0, params, (6144, -6144, 32768)), stereo)}


def test_finish_sequence_writes_the_manifest_without_a_binary(tmp_path, monkeypatch):
    from video_3d_pipeline import utils
    monkeypatch.setattr(utils.shutil, "which", lambda name: None)
    monkeypatch.setattr(utils.subprocess, "run", lambda *a, **k: pytest.fail("no binary, no command"))
    given = {"zeta": 1, "alpha": [1.5, "two"], "note": "kept in the caller's order", "fps": 23.976}
    for name in ("m.json", "m.mp4"):                                   # an .mp4 path without a binary holds the manifest too
        utils.finish_sequence(tmp_path / "m_frames", "frame_%06d.png", tmp_path / name, 23.976, given)
        assert (tmp_path / name).read_bytes() == json.dumps(given, indent=1).encode()
    # the builders pass their complete dict: `note` is the depth manifest's last key, and precedes the stereo manifest's optional ones
    _, finishers = _finishers(tmp_path)
    for pattern, (call, manifest) in finishers.items():
        call(tmp_path / "b.mp4")
        assert (tmp_path / "b.mp4").read_bytes() == json.dumps(manifest, indent=1).encode(), pattern


def test_finish_sequence_runs_the_one_ffmpeg_command(tmp_path, monkeypatch, capsys):
    from video_3d_pipeline import utils
    calls = []

    class Result:
        returncode, stderr = 0, b"x264 [error]: boom\n"

    def run(cmd, **kw):
        calls.append((cmd, kw))
        return Result
    monkeypatch.setattr(utils.shutil, "which", lambda name: "/opt/bin/ffmpeg" if name == "ffmpeg" else None)
    monkeypatch.setattr(utils.subprocess, "run", run)
    d, finishers = _finishers(tmp_path)
    out = tmp_path / "x.mp4"
    for pattern, (call, _) in finishers.items():
        call(out)
        assert calls.pop() == (["/opt/bin/ffmpeg", "-y", "-v", "error", "-r", "25.0", "-f", "image2", "-i", str(d / pattern),
                                "-vcodec", "libx264", "-pix_fmt", "yuv420p", "-crf", "18", "-preset", "medium", "-r", "25.0", str(out)],
                               {"capture_output": True}), pattern
        assert not out.exists()                                        # the command writes the file, nothing else does
        call(tmp_path / "x.json")                                      # not an .mp4: the manifest, binary or not
        assert not calls and json.loads((tmp_path / "x.json").read_text())["pattern"] == pattern
    Result.returncode = 3
    for pattern, (call, _) in finishers.items():
        with pytest.raises(RuntimeError, match="FFmpeg processing failed: rc=3"):
            call(out)
        assert "FFmpeg error:\nx264 [error]: boom\n" in capsys.readouterr().out, pattern
