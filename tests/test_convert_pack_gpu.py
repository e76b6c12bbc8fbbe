"""The top-bottom and anaglyph layouts end to end on the MI355X (real HIP backends): the convert CLI on a small synthetic clip for
full-tb (an output taller than its input) and anaglyph-dubois, with zlib and with --png-encoder gpu, decoding to the frames of the
NumPy contract (tests/stereo_pack_ref.py); and the one-pass pipeline's --stereo-output --layout half-tb --subpixel, which writes
the files the convert CLI writes from the pipeline's depth output."""
import json
import os

import numpy as np
import pytest

import stereo_pack_ref as P
from test_convert_sub_gpu import N_FRAMES, OPTS, SH, SW, _decoded, _pngs, clip  # noqa: F401  (the clip of the sub-pixel tests)

pytestmark = pytest.mark.gpu

LAYOUTS = {"full-tb": P.FULL_TB, "anaglyph-dubois": P.ANAGLYPH_DUBOIS}


@pytest.mark.parametrize("encoder", ["zlib", "gpu"])
@pytest.mark.parametrize("layout,subpixel", [("full-tb", False), ("anaglyph-dubois", True)])
def test_convert_cli_equals_the_restatement(native, clip, tmp_path, layout, subpixel, encoder):
    from video_3d_pipeline import convert
    tmp, frames, depths, gains, _ = clip
    out = tmp_path / "o.json"
    rc = convert.main([str(tmp / "v4k.npy"), str(tmp / "d_frames"), "--output", str(out), "--layout", layout, *OPTS,
                       "--png-encoder", encoder] + (["--subpixel"] if subpixel else []))
    assert rc == 0
    man = json.loads(out.read_text())
    ow, oh = P.output_size(LAYOUTS[layout], 2 * SW, 2 * SH)
    assert (man["layout"], man["width"], man["height"], man["count"]) == (layout, ow, oh, N_FRAMES)
    assert (man["gain_left"], man["gain_right"], man["conv"]) == gains
    got = _decoded(man["frames_dir"])
    assert len(got) == N_FRAMES
    for i in range(N_FRAMES):
        assert got[i].shape == (oh, ow, 3)
        assert np.array_equal(got[i], P.render(frames[i], depths[i], *gains, LAYOUTS[layout], subpixel)), i


def test_pipeline_stereo_output_half_tb_subpixel_equals_the_convert_cli(native, tmp_path):
    from video_3d_pipeline import convert, pipeline, synthetic as syn
    from video_3d_pipeline.utils import read_png16
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(N_FRAMES)])
    v4k = np.random.default_rng(9).integers(0, 256, (N_FRAMES, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)
    sbs_p, v4k_p, depth_out, st = str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), str(tmp_path / "depth.json"), str(tmp_path / "st3d.json")
    rc = pipeline.main([sbs_p, v4k_p, "--work-dir", str(tmp_path / "w"), "--output", depth_out, "--stereo-only", "--stereo-output", st,
                        "--layout", "half-tb", *OPTS, "--subpixel"])
    assert rc == 0
    rc = convert.main([v4k_p, depth_out, "--output", str(tmp_path / "cli3d.json"), "--layout", "half-tb", *OPTS, "--subpixel"])
    assert rc == 0
    got, want = json.loads(open(st).read()), json.loads((tmp_path / "cli3d.json").read_text())
    assert got["layout"] == "half-tb" and got["subpixel"] is True and got["count"] == want["count"] == N_FRAMES
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"])
    ddir = json.loads(open(depth_out).read())["frames_dir"]
    gains = P.R.stereo_gains(40, 0.45, 0.3)
    frames = _decoded(got["frames_dir"])
    for i in range(N_FRAMES):
        d = read_png16(os.path.join(ddir, f"depth4k_{i:06d}.png"))
        assert np.array_equal(frames[i], P.render(v4k[i], d, *gains, P.HALF_TB, True)), i
