"""Source-faithful 3D through the real HIP backends on a small synthetic clip: 480 x 270 eyes stored side by side at full width
(--no-unsqueeze: the matcher's eye is the stored eye) and a 960 x 540 BGR "4K" release, the left view enlarged 2x.  The one-pass
pipeline with --depth-range metric --fill-holes --stereo-output --parallax source writes the files of the three CLIs; with
--fill-from-source the convert CLI's right eye is held to the clip's true right eye; without the new flags nothing changes."""
import hashlib
import json
import os

import numpy as np
import pytest

import stereo_ref as R

pytestmark = pytest.mark.gpu

EW, EH, NF = 480, 270, 2
FLAGS = ("--depth-range", "metric", "--fill-holes")


def _zoom2(a):
    from scipy.ndimage import zoom
    return np.clip(np.rint(zoom(a.astype(np.float32), (2, 2, 1), order=1, mode="nearest", grid_mode=True)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("srcclips")
    pairs = [syn.stereo_pair(EW, EH, i) for i in range(NF)]
    np.save(d / "sbs.npy", np.stack([np.hstack(p) for p in pairs]))
    np.save(d / "v4k.npy", np.stack([_zoom2(p[0]) for p in pairs]))
    return str(d / "sbs.npy"), str(d / "v4k.npy"), [_zoom2(p[1]) for p in pairs]


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


def _depth_dir(work):
    dirs = [d for d in sorted(os.listdir(work)) if d.startswith("depth_") and os.path.isdir(os.path.join(work, d))]
    assert len(dirs) == 1, dirs
    return os.path.join(work, dirs[0])


def _three_clis(tmp, tag, sbs, v4k, depth_flags=(), convert_flags=()):
    """depth CLI, upscale CLI, convert CLI -> (depth dir, 4K depth manifest, stereo manifest)"""
    from video_3d_pipeline import convert, depth
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    work = str(tmp / f"cli_{tag}")
    assert depth.main([sbs, "--work-dir", work, "--stereo-only", "--no-unsqueeze", *depth_flags]) == 0
    up = SimpleDepthUpscaler().process_depth_upscaling(_depth_dir(work), v4k, output_path=str(tmp / f"up_{tag}.json"))
    assert convert.main([v4k, up, "--output", str(tmp / f"3d_{tag}.json"), *convert_flags]) == 0
    return _depth_dir(work), json.loads(open(up).read()), json.loads(open(tmp / f"3d_{tag}.json").read())


def _right_eye_error(man, truth):
    from video_3d_pipeline.utils import iter_frames
    frames = list(iter_frames(man["frames_dir"]))
    assert len(frames) == NF and frames[0].shape == (2 * EH, 4 * EW, 3)
    return float(np.mean([np.abs(f[:, 2 * EW:].astype(int) - t.astype(int)).mean() for f, t in zip(frames, truth)]))


def test_pipeline_writes_the_files_of_the_three_clis(native, tmp_path, clips):
    from video_3d_pipeline import pipeline
    sbs, v4k, _ = clips
    ddir, up, st = _three_clis(tmp_path, "m", sbs, v4k, FLAGS, ("--parallax", "source"))
    block = {"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": EW}
    assert json.loads(open(os.path.join(ddir, "depth_range.json")).read()) == block == up["depth_range"]
    key = f"{sbs}_0_{NF}_Intel/dpt-large_False_fill1_metric"
    assert os.path.basename(ddir) == "depth_" + hashlib.md5(key.encode()).hexdigest()[:16]
    work, out = str(tmp_path / "pipe"), str(tmp_path / "pipe.json")
    assert pipeline.main([sbs, v4k, "--work-dir", work, "--output", out, "--stereo-only", "--no-unsqueeze", "--keep-depth-maps", *FLAGS,
                          "--stereo-output", str(tmp_path / "pipe3d.json"), "--parallax", "source"]) == 0
    man, pst = json.loads(open(out).read()), json.loads(open(tmp_path / "pipe3d.json").read())
    assert os.path.basename(_depth_dir(work)) == os.path.basename(ddir) and _pngs(_depth_dir(work)) == _pngs(ddir)
    assert json.loads(open(os.path.join(_depth_dir(work), "depth_range.json")).read()) == block == man["depth_range"]
    assert _pngs(man["frames_dir"]) == _pngs(up["frames_dir"]) and len(_pngs(man["frames_dir"])) == NF
    assert _pngs(pst["frames_dir"]) == _pngs(st["frames_dir"]) and len(_pngs(st["frames_dir"])) == NF
    assert {k: v for k, v in pst.items() if k != "frames_dir"} == {k: v for k, v in st.items() if k != "frames_dir"}
    assert (st["parallax"], st["parallax_scale"], st["parallax_gain"], st["eye_split"], st["convergence"]) == ("source", 2.0, 1.0, 0, 0)
    assert (st["gain_left"], st["gain_right"], st["conv"]) == (0, -32769, 0)
    # the samples are metric: the stereo frames are the contract's render of the 4K frame and the 4K depth with those gains
    from video_3d_pipeline.utils import iter_frames, read_png16
    got, frames = list(iter_frames(st["frames_dir"])), list(iter_frames(v4k))
    d0 = read_png16(os.path.join(up["frames_dir"], "depth4k_000000.png"))
    assert np.array_equal(got[0], R.render(frames[0], d0, 0, -32769, 0))


def test_fill_from_source_halves_the_right_eyes_error(native, tmp_path, clips):
    """the right eye against the clip's true right eye (enlarged 2x), mean absolute BGR error over the clip, driven by the matcher's
    own disparity.  Measured on one MI355X: today's defaults 37.51, --parallax source with --fill-from-source 5.30 (ratio 0.141)."""
    sbs, v4k, truth = clips
    _, _, parent = _three_clis(tmp_path, "parent", sbs, v4k)
    _, _, src = _three_clis(tmp_path, "src", sbs, v4k, FLAGS, ("--parallax", "source", "--fill-from-source", sbs))
    assert src["fill_from_source"] == sbs and src["source_start_frame"] == 0 and "fill_from_source" not in parent
    e_parent, e_src = _right_eye_error(parent, truth), _right_eye_error(src, truth)
    print(f"right eye vs truth: today's defaults {e_parent:.2f}, source parallax + source fill {e_src:.2f} (ratio {e_src / e_parent:.3f})")
    assert e_src <= 0.5 * e_parent


def test_without_the_flags_nothing_changes(native, tmp_path, clips):
    sbs, v4k, _ = clips
    ddir, up, st = _three_clis(tmp_path, "off", sbs, v4k)
    key = f"{sbs}_0_{NF}_Intel/dpt-large_False"
    assert os.path.basename(ddir) == "depth_" + hashlib.md5(key.encode()).hexdigest()[:16]          # the reference's key
    assert sorted(os.listdir(ddir)) == [f"depth_{i:06d}.png" for i in range(NF)]
    assert sorted(up) == sorted(["format", "frames_dir", "pattern", "count", "width", "height", "fps", "guided_radius", "guided_eps", "note"])
    assert sorted(st) == sorted(["format", "frames_dir", "pattern", "count", "width", "height", "fps", "layout", "max_shift", "convergence",
                                 "eye_split", "gain_left", "gain_right", "conv", "note"])
    assert (st["max_shift"], st["convergence"], st["eye_split"]) == (48.0, 0.5, 0.5)
    from video_3d_pipeline.utils import iter_frames, read_png16
    got, frames = list(iter_frames(st["frames_dir"])), list(iter_frames(v4k))
    for i in range(NF):                                        # the parent's bytes: the contract's render at the default gains
        d = read_png16(os.path.join(up["frames_dir"], f"depth4k_{i:06d}.png"))
        assert np.array_equal(got[i], R.render(frames[i], d, *R.stereo_gains())), i
