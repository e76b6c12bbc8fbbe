"""Host logic of the top-bottom, row-interleaved and anaglyph layouts (video_3d_pipeline.convert and the pipeline's
--stereo-output) on the CPU.  Stand-in backends over the NumPy contract (tests/stereo_pack_ref.py) take the place of the HIP
ones; they have the signatures of the stand-ins in tests/test_convert_sub_host.py, so nothing but the layout code tells a call
for a new layout from an old one."""
import json
import subprocess
import sys

import numpy as np
import pytest

import stereo_pack_ref as P
from conftest import ROOT
from test_convert_host import H4, W4, RefStereoPipelineBackend, _pngs, _read_clip, inputs, sbs_clips  # noqa: F401

NEW = {P.NAMES[c]: c for c in (P.FULL_TB, P.HALF_TB, P.ROWS, P.ANAGLYPH_COLOUR, P.ANAGLYPH_DUBOIS)}


class PackRenderBackend:
    """test-only stand-in for convert.HipRenderBackend over the packing contract; records what it was called with"""

    def __init__(self):
        self.calls = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False):
        assert capacity is None or len(frames) <= capacity
        self.calls.append((len(frames), layout, subpixel))
        return np.stack([P.render(f, d, gain_left, gain_right, conv, layout, subpixel) for f, d in zip(frames, depths)])


class PackStereoPipelineBackend(RefStereoPipelineBackend):
    def render_stereo(self, u16_4k, gains, layout, subpixel=False):
        return [None if f is None else P.render(f, q, *gains, layout, subpixel) for f, q in zip(self.staged, u16_4k)]


def _run(args, backend):
    from video_3d_pipeline import convert
    return convert.main([str(a) for a in args], backend=backend)


def test_layout_table_and_output_size():
    from video_3d_pipeline import _native, convert
    assert convert.LAYOUTS == {name: code for code, name in P.NAMES.items()}
    for code in P.PACKINGS:
        assert _native.stereo_output_size(code, 38, 10) == P.output_size(code, 38, 10) == convert.output_size(code, 38, 10)
    assert _native.stereo_output_size(_native.STEREO_PACK_FULL_TB, 7, 3) == (7, 6)
    assert (_native.STEREO_PACK_FULL_SBS, _native.STEREO_PACK_HALF_SBS) == (_native.STEREO_FULL_SBS, _native.STEREO_HALF_SBS)
    for bad in ((7, 4, 4), (-1, 4, 4), (P.HALF_SBS, 5, 4), (P.HALF_TB, 4, 5)):
        with pytest.raises(ValueError):
            _native.stereo_output_size(*bad)
    for name in ("top-bottom", "anaglyph"):                                     # the generic names stay refused
        with pytest.raises(ValueError):
            convert.stereo_settings(layout=name)
    assert "v3d_render_stereo_packed_batch" in _native.EXPORTS and hasattr(_native.lib(), "v3d_render_stereo_packed_batch")


@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("layout", list(NEW))
def test_cli_frames_equal_the_restatement(inputs, layout, subpixel):
    from video_3d_pipeline.utils import get_video_info
    tmp, frames, depths = inputs
    out = tmp / "packed.json"
    be = PackRenderBackend()
    rc = _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", out, "--layout", layout, "--max-shift", "30",
               "--eye-split", "0.3"] + (["--subpixel"] if subpixel else []), be)
    assert rc == 0 and be.calls == [(4, NEW[layout], subpixel), (1, NEW[layout], subpixel)]
    man = json.loads(out.read_text())
    gains = P.R.stereo_gains(30.0, 0.5, 0.3)
    got = _read_clip(man["frames_dir"])
    assert len(got) == 5
    for i in range(5):
        assert np.array_equal(got[i], P.render(frames[i], depths[i], *gains, NEW[layout], subpixel)), i
    ow, oh = P.output_size(NEW[layout], W4, H4)
    assert (man["count"], man["width"], man["height"], man["layout"]) == (5, ow, oh, layout)
    assert man.get("subpixel", False) is subpixel
    assert sorted(k for k in man if k != "subpixel") == sorted(
        ["format", "frames_dir", "pattern", "count", "width", "height", "fps", "layout", "max_shift", "convergence", "eye_split",
         "gain_left", "gain_right", "conv", "note"])
    info = get_video_info(man["frames_dir"])
    assert (info["width"], info["height"], info["frames"]) == (ow, oh, 5)
    assert got[0].shape == (oh, ow, 3)


def test_half_tb_on_an_odd_height_exits_1_with_a_message(tmp_path, capsys):
    from video_3d_pipeline.utils import write_png16
    H, W = 5, 8
    np.save(tmp_path / "odd.npy", np.zeros((2, H, W, 3), np.uint8))
    (tmp_path / "d_frames").mkdir()
    for i in range(2):
        write_png16(tmp_path / "d_frames" / f"depth4k_{i:06d}.png", np.zeros((H, W), np.uint16))
    be = PackRenderBackend()
    assert _run([tmp_path / "odd.npy", tmp_path / "d_frames", "--output", tmp_path / "o.json", "--layout", "half-tb"], be) == 1
    assert "half top-bottom needs an even frame height" in capsys.readouterr().out and not be.calls
    assert not (tmp_path / "o.json").exists()
    assert _run([tmp_path / "odd.npy", tmp_path / "d_frames", "--output", tmp_path / "o.json", "--layout", "interlaced"], be) == 0


def test_default_output_name_and_render_frame(inputs, monkeypatch):
    from video_3d_pipeline.convert import DepthTo3DConverter
    tmp, frames, depths = inputs
    conv = DepthTo3DConverter(max_shift=20, layout="full-tb", backend=PackRenderBackend())
    got = conv.render_frame(frames[0], depths[0])
    assert got.shape == (2 * H4, W4, 3) and np.array_equal(got, P.render(frames[0], depths[0], *P.R.stereo_gains(20), P.FULL_TB))
    monkeypatch.chdir(tmp)
    assert conv.process_conversion(str(tmp / "v4k.npy"), str(tmp / "depth_4k_frames"), max_frames=1) == "3d_full-tb_depth_4k_frames.mp4"


def _pipeline(tmp, sbs, v4k, tag, backend, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp / f"w_{tag}"), batch_size=2, stereo_only=True, guide_batch=3, backend=backend)
    return json.loads(open(pipe.run(sbs, v4k, output_path=str(tmp / f"depth_{tag}.json"), **kw)).read())


@pytest.mark.parametrize("layout,subpixel", [("half-tb", True), ("anaglyph-dubois", False)])
def test_pipeline_stereo_output_equals_the_convert_cli(sbs_clips, layout, subpixel):
    tmp, sbs, v4k, _ = sbs_clips
    opts = dict(max_shift=25.0, convergence=0.4, eye_split=0.7, layout=layout, subpixel=subpixel)
    _pipeline(tmp, sbs, v4k, "p", PackStereoPipelineBackend(), guide_start_frame=1, stereo_output=str(tmp / "p3d.json"),
              stereo_options=opts)
    got = json.loads((tmp / "p3d.json").read_text())
    rc = _run([v4k, tmp / "depth_p.json", "--output", tmp / "cli3d.json", "--guide-start-frame", "1", "--layout", layout,
               "--max-shift", "25", "--convergence", "0.4", "--eye-split", "0.7"] + (["--subpixel"] if subpixel else []),
              PackRenderBackend())
    assert rc == 0
    want = json.loads((tmp / "cli3d.json").read_text())
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"]) and len(_pngs(got["frames_dir"])) == 6
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    assert (got["layout"], got["width"], got["height"]) == (layout, W4, H4)


def test_pipeline_without_stereo_output_calls_nothing_new(sbs_clips):
    class Strict(PackStereoPipelineBackend):
        def render_stereo(self, *a, **kw):
            raise AssertionError("render_stereo without --stereo-output")
    tmp, sbs, v4k, _ = sbs_clips
    assert _pipeline(tmp, sbs, v4k, "plain", Strict(), guide_start_frame=1)["count"] == 5


def test_both_clis_list_the_layouts():
    for mod in ("video_3d_pipeline.convert", "video_3d_pipeline.pipeline"):
        res = subprocess.run([sys.executable, "-m", mod, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, mod
        for name in NEW:
            assert name in res.stdout, (mod, name)
