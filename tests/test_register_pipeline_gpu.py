"""Spatial registration end to end through the real HIP backends on small .npy clips: a 256 x 144 left eye with letterbox bars and
a 512 x 288 guide that shows the picture alone.  `align --register-spatial` recovers the map; the upscale CLI and the one-pass
pipeline, given that alignment file, write the composition of the stages -- the binding's guided filter on the restatement's warp
(tests/register_ref.py) of the very low-res u16 planes -- bit for bit; --no-spatial writes what a file without the block gives."""
import json
import os

import numpy as np
import pytest

import register_ref as RR

pytestmark = pytest.mark.gpu

EYE, GUIDE, NF = (256, 144), (512, 288), 3
LETTERBOX = (1.0, 0.0, 0.875, 0.0625)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("rclips")
    pairs = [syn.registered_pair(EYE, GUIDE, LETTERBOX, i, bars=True) for i in range(NF)]
    eye, guide = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    # the right eye: the left one at disparity 8 (left half of the picture) and 20 (right half), so that the matcher has depth to find
    right = np.where((np.arange(EYE[0]) < EYE[0] // 2)[None, None, :], np.roll(eye, -8, axis=2), np.roll(eye, -20, axis=2))
    np.save(d / "sbs.npy", np.repeat(np.concatenate([eye, right], axis=2)[..., None], 3, axis=3))
    np.save(d / "v4k.npy", np.repeat(guide[..., None], 3, axis=3))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


@pytest.fixture(scope="module")
def aligned(clips, tmp_path_factory):
    """the align CLI's file with the block, and the same file without it"""
    from video_3d_pipeline import align
    w = tmp_path_factory.mktemp("align")
    assert align.main([*clips, "--work-dir", str(w), "--video-only", "--no-unsqueeze", "--refine-window", "2", "--refine-probes", "1",
                       "--register-spatial"]) == 0
    data = json.loads((w / "alignment_data.json").read_text())
    plain = {k: v for k, v in data.items() if k != "spatial"}
    (w / "plain.json").write_text(json.dumps(plain))
    return str(w / "alignment_data.json"), str(w / "plain.json"), data


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


def _planes(d, pattern, n=NF):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), pattern % i)) for i in range(n)])


def _depth_dir(work):
    dirs = [d for d in sorted(os.listdir(work)) if d.startswith("depth_") and os.path.isdir(os.path.join(work, d))]
    assert len(dirs) == 1, dirs
    return os.path.join(work, dirs[0])


def _pipeline_cli(tmp_path, tag, clips, *flags):
    from video_3d_pipeline import pipeline as pipe_mod
    work, out = str(tmp_path / f"pipe_{tag}"), str(tmp_path / f"pipe_{tag}.json")
    assert pipe_mod.main([*clips, "--work-dir", work, "--output", out, "--stereo-only", "--no-unsqueeze", "--keep-depth-maps", *flags]) == 0
    return _depth_dir(work), json.loads(open(out).read())


def _upscale_cli(tmp_path, tag, ddir, v4k, *flags):
    from video_3d_pipeline import upscale as up_mod
    out = str(tmp_path / f"up_{tag}.json")
    assert up_mod.main([ddir, v4k, "--output", out, *flags]) == 0
    return json.loads(open(out).read())


def test_align_recovers_the_letterbox(aligned):
    """within 1.0 source pixel at both ends of both axes, as tests/test_register_host.py asks of the restatement"""
    sp = aligned[2]["spatial"]
    ex, bx, ey, by = sp["map"]
    Ax, Bx, Ay, By = LETTERBOX
    r = max(abs(bx - Bx) * EYE[0], abs(ex + bx - Ax - Bx) * EYE[0], abs(by - By) * EYE[1], abs(ey + by - Ay - By) * EYE[1])
    print(f"device estimate: {sp['status']} map {sp['map']} scores {sp['score']} residual {r:.3f} px")
    assert sp["status"] == "registered" and aligned[2]["guide_start_frame"] == 0
    assert (sp["eye_size"], sp["guide_size"], sp["unsqueeze"]) == (list(EYE), list(GUIDE), False)
    assert r <= 1.0


def test_clis_write_the_composition_of_the_stages(native, tmp_path, clips, aligned):
    from video_3d_pipeline import register as R
    from video_3d_pipeline.upscale import GUIDED_EPS, GUIDED_RADIUS
    f, plain_file, data = aligned
    ddir, man = _pipeline_cli(tmp_path, "map", clips, "--alignment-file", f)
    assert man["spatial_map"] == data["spatial"]["map"] and man["spatial_map_source"] == f
    lo = _planes(ddir, "depth_%06d.png")
    assert lo.shape == (NF, EYE[1], EYE[0]) and lo.dtype == np.uint16 and (lo > 0).mean() > 0.2
    w = R.warp_q16(data["spatial"]["map"], EYE, GUIDE)
    assert w["size"] == EYE
    warped = RR.warp(lo, *w["q"], 0, *w["size"])
    assert not np.array_equal(warped, lo)
    luma = native.bgr_to_gray(native.to_device(np.load(clips[1])))
    want = native.guided_upscale_u16_batch(native.to_device(warped.view(np.int16)), luma, GUIDED_RADIUS, GUIDED_EPS).cpu().numpy().view(np.uint16)
    got = _planes(man["frames_dir"], "depth4k_%06d.png")
    assert np.array_equal(got, want), f"pipeline: {int((got != want).sum())} samples differ"
    up = _upscale_cli(tmp_path, "map", ddir, clips[1], "--alignment-file", f)
    assert up["spatial_map"] == data["spatial"]["map"]
    got = _planes(up["frames_dir"], "depth4k_%06d.png")
    assert np.array_equal(got, want), f"upscale: {int((got != want).sum())} samples differ"
    # --no-spatial: the files of a run whose alignment file has no block, and no trace in the manifest
    d0, man0 = _pipeline_cli(tmp_path, "plain", clips, "--alignment-file", plain_file)
    d1, man1 = _pipeline_cli(tmp_path, "off", clips, "--alignment-file", f, "--no-spatial")
    assert _pngs(man0["frames_dir"]) == _pngs(man1["frames_dir"]) and _pngs(d0) == _pngs(d1) == _pngs(ddir)
    assert "spatial_map" not in man0 and "spatial_map" not in man1
    assert not np.array_equal(_planes(man0["frames_dir"], "depth4k_%06d.png"), want)
    up0 = _upscale_cli(tmp_path, "plain", ddir, clips[1], "--alignment-file", plain_file)
    up1 = _upscale_cli(tmp_path, "off", ddir, clips[1], "--alignment-file", f, "--no-spatial")
    assert _pngs(up0["frames_dir"]) == _pngs(up1["frames_dir"]) == _pngs(man0["frames_dir"]) and "spatial_map" not in up1
