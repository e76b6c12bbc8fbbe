"""--fill-holes through the real HIP backends on a small synthetic clip: the depth CLI's PNGs are the reference fill of the
oracle disparity followed by the oracle's normalisation, the one-pass pipeline writes the same PNGs, the flag combines with the
temporal stage and the robust range, and without it every output is what the oracle chain of the existing tests gives."""
import json
import os

import numpy as np
import pytest

import fill_ref as FR
import range_ref as RR

pytestmark = pytest.mark.gpu

SW, SH, NF = 192, 64, 3


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("fclips")
    np.save(d / "sbs.npy", syn.temporal_sbs_clip(SW, SH, NF, speed=4))
    rng = np.random.default_rng(9)
    np.save(d / "v4k.npy", rng.integers(0, 256, (NF, 2 * SH, 2 * SW, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


@pytest.fixture(scope="module")
def chain(clips, oracle):
    """the oracle's side of the clip, computed once: int16 disparity and left gray per frame"""
    from video_3d_pipeline.utils import iter_frames
    disp, gray = [], []
    for f in iter_frames(clips[0]):
        l, r = oracle.sbs_to_gray(f, True)
        disp.append(oracle.sgbm_compute(l, r))
        gray.append(l)
    disp = np.stack(disp)
    assert (disp < 0).mean() > 0.3                       # 64 of 192 columns at least
    return disp, np.stack(gray)


def _depth_dir(work):
    dirs = [d for d in sorted(os.listdir(work)) if d.startswith("depth_") and os.path.isdir(os.path.join(work, d))]
    assert len(dirs) == 1, dirs
    return os.path.join(work, dirs[0])


def _maps(d):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), f"depth_{i:06d}.png")) for i in range(NF)])


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if f.endswith(".png")}


def _depth_cli(tmp_path, tag, sbs, *flags):
    from video_3d_pipeline import depth as depth_mod
    work = str(tmp_path / f"cli_{tag}")
    assert depth_mod.main([sbs, "--work-dir", work, "--stereo-only", *flags]) == 0
    return _depth_dir(work)


def _pipeline_cli(tmp_path, tag, sbs, v4k, *flags):
    from video_3d_pipeline import pipeline as pipe_mod
    work, out = str(tmp_path / f"pipe_{tag}"), str(tmp_path / f"pipe_{tag}.json")
    assert pipe_mod.main([sbs, v4k, "--work-dir", work, "--output", out, "--stereo-only", "--keep-depth-maps", *flags]) == 0
    return _depth_dir(work), json.loads(open(out).read())


def test_depth_cli_and_pipeline_with_the_flag(native, oracle, tmp_path, clips, chain):
    sbs, v4k = clips
    disp, _ = chain
    ddir = _depth_cli(tmp_path, "on", sbs, "--fill-holes")
    want = np.stack([oracle.depth_to_u16(oracle.disp_to_depth(FR.fill_frame(d))) for d in disp])
    got = _maps(ddir)
    assert np.array_equal(got, want)
    assert json.loads(open(os.path.join(ddir, "fill.json")).read()) == {"fill_holes": True}
    assert sorted(os.listdir(ddir)) == [f"depth_{i:06d}.png" for i in range(NF)] + ["fill.json"]
    pdir, man = _pipeline_cli(tmp_path, "on", sbs, v4k, "--fill-holes")
    assert os.path.basename(pdir) == os.path.basename(ddir) and _pngs(pdir) == _pngs(ddir)
    assert man["fill_holes"] is True and man["count"] == NF and "temporal" not in man
    assert json.loads(open(os.path.join(pdir, "fill.json")).read()) == {"fill_holes": True}
    # the 4K maps are the upscale CLI's on those depth maps
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    out = SimpleDepthUpscaler().process_depth_upscaling(ddir, v4k, output_path=str(tmp_path / "up.json"))
    assert _pngs(man["frames_dir"]) == _pngs(json.loads(open(out).read())["frames_dir"])


def test_flag_combines_with_the_temporal_stage_and_the_robust_range(native, oracle, tmp_path, clips, chain):
    sbs, v4k = clips
    disp, gray = chain
    flags = ("--fill-holes", "--temporal-radius", "1", "--range-percentile", "99")
    ddir = _depth_cli(tmp_path, "all", sbs, *flags)
    depth = np.stack([oracle.disp_to_depth(FR.fill_frame(d)) for d in disp])
    assert np.array_equal(_maps(ddir), RR.stabilize(depth, gray, 1, q=9900))
    assert json.loads(open(os.path.join(ddir, "temporal.json")).read())["range_quantile"] == 9900
    assert json.loads(open(os.path.join(ddir, "fill.json")).read()) == {"fill_holes": True}
    pdir, man = _pipeline_cli(tmp_path, "all", sbs, v4k, *flags)
    assert os.path.basename(pdir) == os.path.basename(ddir) and _pngs(pdir) == _pngs(ddir)
    assert man["fill_holes"] is True and man["temporal"]["radius"] == 1


def test_without_the_flag_nothing_changes(native, oracle, tmp_path, clips, chain):
    sbs, v4k = clips
    disp, _ = chain
    ddir = _depth_cli(tmp_path, "off", sbs)
    want = np.stack([oracle.depth_to_u16(oracle.disp_to_depth(d)) for d in disp])
    assert np.array_equal(_maps(ddir), want)
    assert sorted(os.listdir(ddir)) == [f"depth_{i:06d}.png" for i in range(NF)]
    key = f"{sbs}_0_{NF}_Intel/dpt-large_True"
    import hashlib
    assert os.path.basename(ddir) == "depth_" + hashlib.md5(key.encode()).hexdigest()[:16]          # the reference's key
    pdir, man = _pipeline_cli(tmp_path, "off", sbs, v4k)
    assert os.path.basename(pdir) == os.path.basename(ddir) and _pngs(pdir) == _pngs(ddir)
    assert "fill_holes" not in man and not os.path.exists(os.path.join(pdir, "fill.json"))
    from video_3d_pipeline.utils import iter_frames, read_png16
    guides = list(iter_frames(v4k))                      # the 4K samples: the oracle's filter on the unfilled maps, to one level
    for f in range(NF):
        q = oracle.guided_upscale(want[f].astype(np.float32), oracle.bgr_to_gray(guides[f]), 8, 1e-3)
        got = read_png16(os.path.join(man["frames_dir"], f"depth4k_{f:06d}.png"))
        assert np.abs(got.astype(np.float64) - np.clip(np.rint(q), 0, 65535)).max() <= 1, f


def test_backend_surfaces_with_the_flag(native, oracle, clips, chain):
    """HipStereoBackend directly: the device pass, the NumPy surface (pairs_to_disparity) and the hybrid blend read the filled
    disparity; without the keyword they return today's values"""
    from video_3d_pipeline.depth import HipStereoBackend
    from video_3d_pipeline.utils import iter_frames
    disp, _ = chain
    frames = list(iter_frames(clips[0]))
    be = HipStereoBackend()
    filled = np.stack([FR.fill_frame(d) for d in disp])
    assert np.array_equal(be.sbs_to_disparity(frames, True, fill_holes=True).cpu().numpy(), np.stack([oracle.disp_to_depth(d) for d in filled]))
    assert np.array_equal(be.sbs_to_disparity(frames, True).cpu().numpy(), np.stack([oracle.disp_to_depth(d) for d in disp]))
    pairs = [oracle.split_sbs(f, True) for f in frames[:2]]
    dp = [oracle.sgbm_compute(oracle.bgr_to_gray(l), oracle.bgr_to_gray(r)) for l, r in pairs]
    got = be.pairs_to_disparity(pairs, fill_holes=True)
    assert all(np.array_equal(g, oracle.disp_to_depth(FR.fill_frame(d))) for g, d in zip(got, dp))
    got = be.pairs_to_disparity(pairs)
    assert all(np.array_equal(g, oracle.disp_to_depth(d)) for g, d in zip(got, dp))
    monos = [np.random.default_rng(i).random((16, 24)).astype(np.float32) * 5 + 1 for i in range(2)]
    got = be.pairs_to_disparity(pairs, monos, fill_holes=True)
    assert all(np.array_equal(g, oracle.mono_blend(FR.fill_frame(d), m)) for g, d, m in zip(got, dp, monos))
