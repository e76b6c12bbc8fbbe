"""--subpixel end to end on the MI355X (real HIP backends): DepthTo3DConverter, the convert CLI and the one-pass pipeline's
--stereo-output --subpixel on a small synthetic clip, with zlib and with --png-encoder gpu.  The written PNGs decode to the frames of
the NumPy contract (tests/stereo_sub_ref.py), and the pipeline and the convert CLI write the same files."""
import json
import os

import numpy as np
import pytest

import stereo_ref as R
import stereo_sub_ref as S

pytestmark = pytest.mark.gpu

SW, SH = 128, 32                      # SBS frame; the "4K" frame is 2SW x 2SH = 256 x 64
N_FRAMES = 5


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _decoded(d):
    from video_3d_pipeline.utils import iter_frames
    return list(iter_frames(d))


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """the 4K clip, its depth maps (ramps, a block at another depth, one noise frame) and the reference's frames, rendered once"""
    from video_3d_pipeline.utils import write_png16
    tmp = tmp_path_factory.mktemp("subclip")
    rng = np.random.default_rng(11)
    W, H = 2 * SW, 2 * SH
    frames = rng.integers(0, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)
    np.save(tmp / "v4k.npy", frames)
    ddir = tmp / "d_frames"
    ddir.mkdir()
    x = np.arange(W)[None, :]
    depths = []
    for i in range(N_FRAMES):
        d = np.clip(rng.integers(0, 65536) + x * int(rng.integers(-200, 200)) + rng.integers(-900, 900, (H, 1)), 0, 65535)
        d[:, 80:120] = rng.integers(0, 65536)
        if i == N_FRAMES - 1:
            d = rng.integers(0, 65536, (H, W))
        depths.append(d.astype(np.uint16))
        write_png16(ddir / f"depth4k_{i:06d}.png", depths[-1])
    gains = S.stereo_gains(40, 0.45, 0.3)
    want = {lay: [S.render(frames[i], depths[i], *gains, lay) for i in range(N_FRAMES)] for lay in (S.FULL_SBS, S.HALF_SBS)}
    return tmp, frames, depths, gains, want


OPTS = ["--max-shift", "40", "--convergence", "0.45", "--eye-split", "0.3"]


@pytest.mark.parametrize("encoder", ["zlib", "gpu"])
@pytest.mark.parametrize("layout", ["full-sbs", "half-sbs"])
def test_convert_cli_subpixel_equals_the_reference(native, clip, tmp_path, layout, encoder):
    from video_3d_pipeline import convert
    tmp, frames, depths, gains, want = clip
    lay = S.FULL_SBS if layout == "full-sbs" else S.HALF_SBS
    out = tmp_path / "o.json"
    rc = convert.main([str(tmp / "v4k.npy"), str(tmp / "d_frames"), "--output", str(out), "--layout", layout, *OPTS, "--subpixel",
                       "--png-encoder", encoder])
    assert rc == 0
    man = json.loads(out.read_text())
    assert man["subpixel"] is True and man["count"] == N_FRAMES and (man["gain_left"], man["gain_right"], man["conv"]) == gains
    got = _decoded(man["frames_dir"])
    assert len(got) == N_FRAMES
    for i in range(N_FRAMES):
        assert np.array_equal(got[i], want[lay][i]), i
    assert not np.array_equal(got[0], R.render(frames[0], depths[0], *gains, lay))        # not the whole-pixel picture


def test_converter_class_flag_on_and_off(native, clip):
    from video_3d_pipeline import convert
    _, frames, depths, gains, want = clip
    on = convert.DepthTo3DConverter(max_shift=40, convergence=0.45, eye_split=0.3, subpixel=True)
    assert np.array_equal(on.render_frame(frames[1], depths[1]), want[S.FULL_SBS][1])
    off = convert.DepthTo3DConverter(max_shift=40, convergence=0.45, eye_split=0.3)
    assert np.array_equal(off.render_frame(frames[1], depths[1]), R.render(frames[1], depths[1], *gains))


@pytest.mark.parametrize("encoder", ["zlib", "gpu"])
def test_pipeline_stereo_output_subpixel_equals_the_convert_cli(native, tmp_path, encoder):
    from video_3d_pipeline import convert, pipeline, synthetic as syn
    from video_3d_pipeline.utils import read_png16
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(N_FRAMES)])
    v4k = np.random.default_rng(9).integers(0, 256, (N_FRAMES, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)
    sbs_p, v4k_p, depth_out, st = str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), str(tmp_path / "depth.json"), str(tmp_path / "st3d.json")
    rc = pipeline.main([sbs_p, v4k_p, "--work-dir", str(tmp_path / "w"), "--output", depth_out, "--stereo-only", "--stereo-output", st,
                        "--layout", "half-sbs", *OPTS, "--subpixel", "--png-encoder", encoder])
    assert rc == 0
    rc = convert.main([v4k_p, depth_out, "--output", str(tmp_path / "cli3d.json"), "--layout", "half-sbs", *OPTS, "--subpixel",
                       "--png-encoder", encoder])
    assert rc == 0
    got, want = json.loads(open(st).read()), json.loads((tmp_path / "cli3d.json").read_text())
    assert got["subpixel"] is True and got["count"] == want["count"] == N_FRAMES
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"])
    # ... and they decode to the reference's rendering of the pipeline's own depth maps
    ddir = json.loads(open(depth_out).read())["frames_dir"]
    gains = S.stereo_gains(40, 0.45, 0.3)
    frames = _decoded(got["frames_dir"])
    for i in range(N_FRAMES):
        d = read_png16(os.path.join(ddir, f"depth4k_{i:06d}.png"))
        assert np.array_equal(frames[i], S.render(v4k[i], d, *gains, S.HALF_SBS)), i
