"""Host logic of --subpixel (video_3d_pipeline.convert and the pipeline's --stereo-output) on the CPU.  Stand-in backends over the
NumPy contracts take the place of the HIP ones: with the flag off they are the stand-ins of tests/test_convert_host.py, which do
not know the `subpixel` argument, and must see exactly the calls and write exactly the manifest of before; with it on, the frames
are those of tests/stereo_sub_ref.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stereo_ref as R
import stereo_sub_ref as S
from conftest import ROOT
from test_convert_host import RefRenderBackend, RefStereoPipelineBackend, _pngs, _read_clip, inputs, sbs_clips  # noqa: F401


class SubRenderBackend(RefRenderBackend):
    """knows the flag; records what it was called with"""

    def __init__(self):
        super().__init__()
        self.flags = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False):
        self.flags.append(subpixel)
        self.batches.append(len(frames))
        ref = S if subpixel else R
        return np.stack([ref.render(f, d, gain_left, gain_right, conv, layout) for f, d in zip(frames, depths)])


class SubStereoPipelineBackend(RefStereoPipelineBackend):
    def render_stereo(self, u16_4k, gains, layout, subpixel=False):
        ref = S if subpixel else R
        return [None if f is None else ref.render(f, q, *gains, layout) for f, q in zip(self.staged, u16_4k)]


def _run(args, backend):
    from video_3d_pipeline import convert
    return convert.main([str(a) for a in args], backend=backend)


def test_flag_off_calls_the_old_backend_and_writes_the_old_manifest(inputs):
    """RefRenderBackend.render_batch has no `subpixel` parameter: any new argument would be a TypeError"""
    tmp, frames, depths = inputs
    out = tmp / "off.json"
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", out], RefRenderBackend()) == 0
    man = json.loads(out.read_text())
    assert sorted(man) == sorted(["format", "frames_dir", "pattern", "count", "width", "height", "fps", "layout", "max_shift",
                                  "convergence", "eye_split", "gain_left", "gain_right", "conv", "note"])
    got = _read_clip(man["frames_dir"])
    for i in range(5):
        assert np.array_equal(got[i], R.render(frames[i], depths[i], *R.stereo_gains())), i
    be = SubRenderBackend()
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "off2.json"], be) == 0 and be.flags == [False, False]
    assert _pngs(json.loads((tmp / "off2.json").read_text())["frames_dir"]) == _pngs(man["frames_dir"])


@pytest.mark.parametrize("layout", ["full-sbs", "half-sbs"])
def test_flag_on_cli_frames_equal_the_subpixel_reference(inputs, layout):
    tmp, frames, depths = inputs
    out = tmp / "on.json"
    be = SubRenderBackend()
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", out, "--subpixel", "--layout", layout, "--max-shift", "30"], be) == 0
    assert be.flags == [True, True] and be.batches == [4, 1]
    man = json.loads(out.read_text())
    assert man["subpixel"] is True and man["layout"] == layout
    got = _read_clip(man["frames_dir"])
    lay = S.FULL_SBS if layout == "full-sbs" else S.HALF_SBS
    gains = S.stereo_gains(30.0)
    differs = 0
    for i in range(5):
        assert np.array_equal(got[i], S.render(frames[i], depths[i], *gains, lay)), i
        differs += not np.array_equal(got[i], R.render(frames[i], depths[i], *gains, lay))
    assert differs                                                              # the flag changes the picture
    # a backend that predates the flag refuses it instead of rendering whole pixels quietly
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "old.json", "--subpixel"], RefRenderBackend()) == 1


def test_converter_class_and_default_output_name(inputs, monkeypatch):
    from video_3d_pipeline.convert import DepthTo3DConverter, stereo_settings
    tmp, frames, depths = inputs
    conv = DepthTo3DConverter(max_shift=20, eye_split=0.25, backend=SubRenderBackend(), subpixel=True)
    assert conv.subpixel and conv.params["subpixel"] is True
    assert np.array_equal(conv.render_frame(frames[0], depths[0]), S.render(frames[0], depths[0], *S.stereo_gains(20, 0.5, 0.25)))
    off = DepthTo3DConverter(max_shift=20, eye_split=0.25, backend=RefRenderBackend())
    assert not off.subpixel and "subpixel" not in off.params
    assert np.array_equal(off.render_frame(frames[0], depths[0]), R.render(frames[0], depths[0], *R.stereo_gains(20, 0.5, 0.25)))
    with pytest.raises(ValueError, match="subpixel"):
        stereo_settings(subpixel="yes")
    monkeypatch.chdir(tmp)                                                      # the default name lands in the working directory
    on_path = conv.process_conversion(str(tmp / "v4k.npy"), str(tmp / "depth_4k_frames"), max_frames=2)
    off_path = off.process_conversion(str(tmp / "v4k.npy"), str(tmp / "depth_4k_frames"), max_frames=2)
    assert on_path == "3d_full-sbs_subpx_depth_4k_frames.mp4" and off_path == "3d_full-sbs_depth_4k_frames.mp4"


def _pipeline(tmp, sbs, v4k, tag, backend, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp / f"w_{tag}"), batch_size=2, stereo_only=True, guide_batch=3, backend=backend)
    return json.loads(open(pipe.run(sbs, v4k, output_path=str(tmp / f"depth_{tag}.json"), **kw)).read())


def test_pipeline_stereo_output_with_and_without_the_flag(sbs_clips):
    tmp, sbs, v4k, _ = sbs_clips
    opts = dict(max_shift=25.0, convergence=0.4, eye_split=0.7, layout="full-sbs")
    # off, through the stand-in that does not know the flag (subpixel=False given explicitly is "off" too)
    _pipeline(tmp, sbs, v4k, "off", RefStereoPipelineBackend(), guide_start_frame=1, stereo_output=str(tmp / "off3d.json"),
              stereo_options=dict(opts, subpixel=False))
    off = json.loads((tmp / "off3d.json").read_text())
    assert "subpixel" not in off
    _pipeline(tmp, sbs, v4k, "on", SubStereoPipelineBackend(), guide_start_frame=1, stereo_output=str(tmp / "on3d.json"),
              stereo_options=dict(opts, subpixel=True))
    on = json.loads((tmp / "on3d.json").read_text())
    assert on["subpixel"] is True and {k: v for k, v in on.items() if k not in ("subpixel", "frames_dir")} == \
        {k: v for k, v in off.items() if k != "frames_dir"}
    assert _pngs(on["frames_dir"]) != _pngs(off["frames_dir"])
    # the pipeline and the convert CLI write the same files
    rc = _run([v4k, tmp / "depth_on.json", "--output", tmp / "cli3d.json", "--guide-start-frame", "1", "--subpixel",
               "--max-shift", "25", "--convergence", "0.4", "--eye-split", "0.7"], SubRenderBackend())
    assert rc == 0
    want = json.loads((tmp / "cli3d.json").read_text())
    assert _pngs(on["frames_dir"]) == _pngs(want["frames_dir"]) and len(_pngs(on["frames_dir"])) == 6
    assert {k: v for k, v in on.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}


def test_both_clis_and_the_rate_tool_take_the_flag():
    from video_3d_pipeline import convert
    import argparse
    for mod in ("video_3d_pipeline.convert", "video_3d_pipeline.pipeline"):
        res = subprocess.run([sys.executable, "-m", mod, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0 and "--subpixel" in res.stdout, mod
    p = argparse.ArgumentParser()
    convert.add_stereo_arguments(p)
    assert "subpixel" not in convert.stereo_options(p.parse_args([]))
    assert convert.stereo_options(p.parse_args(["--subpixel"]))["subpixel"] is True
    assert "--subpixel" in open(os.path.join(ROOT, "tools", "convert_rate.py")).read()


def test_binding_lists_the_entry():
    from video_3d_pipeline import _native
    import inspect
    assert "v3d_render_stereo_subpixel_batch" in _native.EXPORTS
    assert inspect.signature(_native.render_stereo_batch).parameters["subpixel"].default is False
    assert hasattr(_native.lib(), "v3d_render_stereo_subpixel_batch")
    header = open(os.path.join(ROOT, "include", "v3d_hip.h")).read()
    assert "#define V3D_STEREO_TEAR16 32" in header and S.TEAR16 == 32
