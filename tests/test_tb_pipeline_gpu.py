"""--input-layout tb on the MI355X, from the packed frame to the files: the backend's disparity against the oracle's matcher on the
grays of tests/tb_ref.py, the depth CLI's PNGs, the left-eye signatures and profiles, the one-pass pipeline against depth CLI +
upscale CLI, and one check against ground truth that the eyes are neither swapped nor cut at the wrong row."""
import json
import os

import numpy as np
import pytest

import tb_ref

pytestmark = pytest.mark.gpu
W, H, N = 320, 180, 3


@pytest.fixture(scope="module")
def frames():
    from video_3d_pipeline import synthetic as syn
    return [syn.tb_frame(W, H, i) for i in range(N)]


@pytest.fixture(scope="module")
def want_disp(frames):
    """the oracle's disparity x16 of the reference grays, computed once"""
    from oracle import oracle as O
    return [O.sgbm_compute(*tb_ref.to_gray(f, True)) for f in frames]


@pytest.fixture(scope="module")
def clips(tmp_path_factory, frames):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("tb_clips")
    np.save(d / "tb.npy", np.stack(frames))
    np.save(d / "v4k.npy", np.stack([np.repeat(syn.guide_frame(W, H, i)[..., None], 3, axis=2) for i in range(N)]))
    return str(d / "tb.npy"), str(d / "v4k.npy")


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


def test_disparity_equals_the_oracle_on_the_reference_grays(native, frames, want_disp):
    from video_3d_pipeline.depth import HipStereoBackend
    be = HipStereoBackend("cuda")
    got = be.sbs_to_disparity(frames, True, input_layout="tb").cpu().numpy()
    assert got.shape == (N, H, W) and got.dtype == np.float32
    for i, d in enumerate(want_disp):
        assert np.array_equal(got[i], np.maximum(d.astype(np.float32) / np.float32(16), np.float32(0))), i
        assert np.array_equal(be.left_gray(N)[i].cpu().numpy(), tb_ref.to_gray(frames[i], True)[0])
    squeezed = be.sbs_to_disparity(frames[:1], False, input_layout="tb")
    assert tuple(squeezed.shape) == (1, H // 2, W)
    with pytest.raises(ValueError, match="top-bottom frame height must be even"):
        be.sbs_to_disparity([np.zeros((7, 128, 3), np.uint8)], True, input_layout="tb")
    be.close_matcher()


def test_depth_cli_writes_the_reference_pngs(native, oracle, tmp_path, clips, want_disp, capsys):
    """the PNGs of save_depth_map's arithmetic (per-frame min-max -> uint16) for the oracle's disparities"""
    from video_3d_pipeline import depth
    from video_3d_pipeline.utils import read_png16
    rc = depth.main([clips[0], "--work-dir", str(tmp_path / "cli"), "--stereo-only", "--input-layout", "tb"])
    assert rc == 0 and "Success" in capsys.readouterr().out
    dirs = [d for d in os.listdir(tmp_path / "cli") if d.startswith("depth_")]
    assert len(dirs) == 1
    out = tmp_path / "cli" / dirs[0]
    assert sorted(os.listdir(out)) == [f"depth_{i:06d}.png" for i in range(N)] + ["input_layout.json"]
    for i, d in enumerate(want_disp):
        assert np.array_equal(read_png16(out / f"depth_{i:06d}.png"), oracle.depth_to_u16(oracle.disp_to_depth(d))), i


def test_left_eye_signatures_and_profiles(native, frames):
    """the top-bottom calls equal the same device entries on the left eye handed over as a plane"""
    from video_3d_pipeline.depth import HipStereoBackend
    be = HipStereoBackend("cuda")
    for unsqueeze in (True, False):
        left = native.to_device(np.stack([tb_ref.to_gray(f, unsqueeze)[0] for f in frames]))
        sig = be.sbs_left_signatures(frames, unsqueeze, input_layout="tb")
        assert np.array_equal(sig.cpu().numpy(), native.frame_signature_batch(left).cpu().numpy())
        col, row = be.sbs_left_profiles(frames, unsqueeze, input_layout="tb")
        want_col, want_row = native.plane_profiles_batch(left)
        assert np.array_equal(col.cpu().numpy(), want_col.cpu().numpy()) and np.array_equal(row.cpu().numpy(), want_row.cpu().numpy())


def test_pipeline_equals_depth_cli_plus_upscale_cli(native, tmp_path, clips):
    from video_3d_pipeline import depth, pipeline, upscale
    tb, v4k = clips
    assert depth.main([tb, "--work-dir", str(tmp_path / "d"), "--stereo-only", "--input-layout", "tb"]) == 0
    ddir = tmp_path / "d" / [d for d in os.listdir(tmp_path / "d") if d.startswith("depth_")][0]
    assert upscale.main([str(ddir), v4k, "--output", str(tmp_path / "two.json")]) == 0
    assert pipeline.main([tb, v4k, "--work-dir", str(tmp_path / "p"), "--stereo-only", "--input-layout", "tb", "--output", str(tmp_path / "one.json")]) == 0
    two, one = json.loads((tmp_path / "two.json").read_text()), json.loads((tmp_path / "one.json").read_text())
    want, got = _pngs(two["frames_dir"]), _pngs(one["frames_dir"])
    assert len(want) == N and got == want
    assert one["input_layout"] == "tb" and two["input_layout"] == "tb" and (one["width"], one["height"]) == (2 * W, 2 * H)


def test_the_eyes_are_neither_swapped_nor_mis_seamed(native):
    """640 x 360: the mean |d - d*| over the valid pixels right of column 64 through the top-bottom path is at most 1.1 x the
    figure of sbs_frame of the same scene through the existing path (the CPU oracle gives 1.336 / 1.352 = 0.988: a top-bottom eye
    keeps its horizontal resolution); swapped eyes leave almost nothing valid"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HipStereoBackend
    Wb, Hb = 640, 360
    gt = syn.gt_disparity(Wb, Hb)
    be = HipStereoBackend("cuda")

    def error(depth):
        d = depth.cpu().numpy()[0][:, 64:]
        valid = d > 0
        return float(np.abs(d - gt[:, 64:])[valid].mean()), float(valid.mean())
    err_tb, valid_tb = error(be.sbs_to_disparity([syn.tb_frame(Wb, Hb, 0)], True, input_layout="tb"))
    err_sbs, valid_sbs = error(be.sbs_to_disparity([syn.sbs_frame(Wb, Hb, 0)], True))
    be.close_matcher()
    print(f"mean |d - d*|: top-bottom {err_tb:.4f} ({valid_tb:.4f} valid), side-by-side {err_sbs:.4f} ({valid_sbs:.4f} valid), "
          f"ratio {err_tb / err_sbs:.4f}")
    assert valid_tb > 0.5 and err_tb <= 1.1 * err_sbs               # the oracle leaves 0.96 valid; anything above half is no swap
