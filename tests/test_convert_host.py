"""Host logic of the DIBR step (video_3d_pipeline.convert, the declared `video-3d-convert`) and of the pipeline's
--stereo-output on CPU.  A stand-in backend over the NumPy contract (tests/stereo_ref.py) takes the place of the HIP one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import stereo_ref as R
from conftest import ROOT
from test_pipeline_host import OraclePipelineBackend, SW, SH

W4, H4 = 2 * SW, 2 * SH                # the "4K" frame of the pipeline tests: 384 x 96


class RefRenderBackend:
    """test-only stand-in for convert.HipRenderBackend; records the batch sizes"""

    def __init__(self):
        self.batches = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None):
        assert capacity is None or len(frames) <= capacity
        self.batches.append(len(frames))
        return np.stack([R.render(f, d, gain_left, gain_right, conv, layout) for f, d in zip(frames, depths)])


class RefStereoPipelineBackend(OraclePipelineBackend):
    """the pipeline stand-in plus render_stereo over the frames guide_luma last staged (as the HIP backend keeps them)"""

    def guide_luma(self, frames, height, width, capacity):
        self.staged = list(frames)
        return super().guide_luma(frames, height, width, capacity)

    def render_stereo(self, u16_4k, gains, layout):
        return [None if f is None else R.render(f, q, *gains, layout) for f, q in zip(self.staged, u16_4k)]


def _clip4k(n, W=W4, H=H4, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def _depths(n, W=W4, H=H4, seed=1):
    rng = np.random.default_rng(seed)
    x = np.arange(W)[None, :]
    out = []
    for i in range(n):
        d = rng.integers(0, 65536) + x * int(rng.integers(-150, 150)) + rng.integers(-2000, 2000, (H, 1))
        d[:, W // 3:W // 2] = rng.integers(0, 65536)                 # a block at another depth: occlusions, disocclusions
        out.append(np.clip(d, 0, 65535).astype(np.uint16))
    return out


@pytest.fixture()
def inputs(tmp_path):
    from video_3d_pipeline.utils import write_png16
    frames = _clip4k(6)
    np.save(tmp_path / "v4k.npy", frames)
    np.save(tmp_path / "v4k_short.npy", frames[:3])
    ddir = tmp_path / "depth_4k_frames"
    ddir.mkdir()
    depths = _depths(5)
    for i, d in enumerate(depths):
        write_png16(ddir / f"depth4k_{i:06d}.png", d)
    return tmp_path, frames, depths


def _read_clip(path):
    from video_3d_pipeline.utils import iter_frames
    return list(iter_frames(str(path)))


def _run(args, backend=None):
    from video_3d_pipeline import convert
    return convert.main([str(a) for a in args], backend=backend if backend is not None else RefRenderBackend())


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("layout, opts", [(R.FULL_SBS, []), (R.HALF_SBS, ["--max-shift", "30", "--convergence", "0.2",
                                                                            "--eye-split", "0"])])
def test_cli_frames_equal_the_reference(inputs, layout, opts):
    from video_3d_pipeline.utils import get_video_info
    tmp, frames, depths = inputs
    out = tmp / "sbs3d.json"
    be = RefRenderBackend()
    rc = _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", out, "--layout", ["full-sbs", "half-sbs"][layout]] + opts, be)
    assert rc == 0
    man = json.loads(out.read_text())
    gains = R.stereo_gains(*(map(float, opts[1::2]) if opts else ()))
    got = _read_clip(man["frames_dir"])
    assert len(got) == 5 and be.batches == [4, 1]
    for i in range(5):
        assert np.array_equal(got[i], R.render(frames[i], depths[i], *gains, layout)), i
    ow = 2 * W4 if layout == R.FULL_SBS else W4
    assert (man["count"], man["width"], man["height"], man["pattern"]) == (5, ow, H4, "frame_%06d.png")
    assert (man["gain_left"], man["gain_right"], man["conv"]) == gains
    assert man["layout"] == ["full-sbs", "half-sbs"][layout] and man["format"] == "png8-rgb-sequence"
    info = get_video_info(man["frames_dir"])
    assert (info["width"], info["height"], info["frames"], info["fps"]) == (ow, H4, 5, 23.976)
    if layout == R.HALF_SBS:
        assert np.array_equal(got[0][:, :W4 // 2], ((frames[0][:, 0::2].astype(int) + frames[0][:, 1::2] + 1) >> 1))


def test_three_depth_input_forms(inputs, capsys):
    tmp, _, _ = inputs
    want = None
    (tmp / "depth_4k.json").write_text(json.dumps({"format": "png16-sequence", "frames_dir": str(tmp / "depth_4k_frames"),
                                                   "pattern": "depth4k_%06d.png", "count": 4}))
    (tmp / "manifest.mp4").write_text((tmp / "depth_4k.json").read_text())      # a manifest at an .mp4 path (no ffmpeg)
    (tmp / "depth_4k.mp4").write_bytes(b"\x00\x00\x00\x18ftypmp42")              # a real video next to its _frames dir
    for k, (src, count) in enumerate(((tmp / "depth_4k_frames", 5), (tmp / "depth_4k.json", 4), (tmp / "manifest.mp4", 4),
                                      (tmp / "depth_4k.mp4", 5))):
        out = tmp / f"o{k}.json"
        assert _run([tmp / "v4k.npy", src, "--output", out]) == 0, src
        got = _pngs(json.loads(out.read_text())["frames_dir"])
        assert len(got) == count + 1                                              # + info.json
        want = want or got
        assert all(got[f] == want[f] for f in got), src
    assert _run([tmp / "v4k.npy", tmp / "nothing_here", "--output", tmp / "x.json"]) == 1
    assert "Error: No depth maps found in" in capsys.readouterr().out
    (tmp / "empty").mkdir()
    assert _run([tmp / "v4k.npy", tmp / "empty", "--output", tmp / "x.json"]) == 1
    assert "No depth maps found" in capsys.readouterr().out


def test_guide_start_frame_and_alignment_file(inputs):
    tmp, frames, depths = inputs
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "g1.json", "--guide-start-frame", "1"]) == 0
    got = _read_clip(json.loads((tmp / "g1.json").read_text())["frames_dir"])
    assert len(got) == 5
    for i in range(5):                                                           # depth i pairs with 4K frame 1 + i
        assert np.array_equal(got[i], R.render(frames[1 + i], depths[i], *R.stereo_gains())), i
    (tmp / "align.json").write_text(json.dumps({"time_offset_seconds": 1 / 23.976, "video1_path": "a", "video2_path": "b"}))
    assert _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "al.json", "--alignment-file", tmp / "align.json"]) == 0
    assert _pngs(json.loads((tmp / "al.json").read_text())["frames_dir"]) == _pngs(json.loads((tmp / "g1.json").read_text())["frames_dir"])
    with pytest.raises(SystemExit) as e:
        _run([tmp / "v4k.npy", tmp / "depth_4k_frames", "--guide-start-frame", "1", "--alignment-file", tmp / "align.json"])
    assert e.value.code == 2


def test_existing_output_is_skipped_unless_forced(inputs):
    tmp, _, _ = inputs
    be = RefRenderBackend()
    args = [tmp / "v4k.npy", tmp / "depth_4k_frames", "--output", tmp / "o.json", "--max-frames", "2"]
    assert _run(args, be) == 0 and be.batches == [2]
    assert _run(args, be) == 0 and be.batches == [2]
    assert _run(args + ["--force"], be) == 0 and be.batches == [2, 2]


def test_error_exits(inputs, capsys):
    from video_3d_pipeline.utils import write_png16
    tmp, _, _ = inputs
    bad = tmp / "bad_frames"
    bad.mkdir()
    write_png16(bad / "depth4k_000000.png", np.zeros((H4, W4 - 2), np.uint16))
    cases = [([tmp / "v4k.npy", tmp / "nope"], "No depth maps found"),
             ([tmp / "nope.npy", tmp / "depth_4k_frames"], "Could not read video info"),
             ([tmp / "v4k.npy", bad], "depth map depth4k_000000.png is"),
             ([tmp / "v4k.npy", tmp / "depth_4k_frames", "--max-shift", "-1"], "max_shift"),
             ([tmp / "v4k.npy", tmp / "depth_4k_frames", "--max-shift", "nan"], "max_shift"),
             ([tmp / "v4k.npy", tmp / "depth_4k_frames", "--max-shift", "70000"], "max_shift"),
             ([tmp / "v4k.npy", tmp / "depth_4k_frames", "--convergence", "1.5"], "convergence"),
             ([tmp / "v4k.npy", tmp / "depth_4k_frames", "--eye-split", "-0.1"], "eye_split")]
    for args, msg in cases:
        assert _run(args + ["--output", tmp / "e.json"]) == 1, args
        out = capsys.readouterr().out
        assert "Error:" in out and msg in out, (args, out)
    from video_3d_pipeline import convert
    assert convert.main([str(tmp / "v4k.npy"), str(tmp / "depth_4k_frames"), "--output", str(tmp / "c.json"), "--device", "cpu"]) == 1
    assert "only has the MI355X (HIP) path" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        convert.main(["--layout", "top-bottom", "a", "b"])


def test_short_4k_clip_stops_the_render(inputs, capsys):
    tmp, frames, depths = inputs
    assert _run([tmp / "v4k_short.npy", tmp / "depth_4k_frames", "--output", tmp / "s.json"]) == 0
    assert "4K video ended after 3" in capsys.readouterr().out
    man = json.loads((tmp / "s.json").read_text())
    got = _read_clip(man["frames_dir"])
    assert man["count"] == 3 and len(got) == 3
    assert np.array_equal(got[2], R.render(frames[2], depths[2], *R.stereo_gains()))


def test_stereo_gains_rounding():
    from video_3d_pipeline._native import stereo_gains
    assert stereo_gains() == (6144, -6144, 32768)                       # 48 px split evenly around the middle depth
    assert stereo_gains(3 / 256, 0.5, 0.5) == (2, -2, 32768)            # 1.5 -> 2: half up, both signs
    assert stereo_gains(48, 0.0, 0.0) == (0, -12288, 0)                # eye_split 0: the left eye is the frame itself
    assert stereo_gains(48, 1.0, 1.0) == (12288, 0, 65535)
    assert stereo_gains(0, 0.5, 0.5) == (0, 0, 32768)
    assert stereo_gains(65535.99, 0.5, 1.0)[0] == (1 << 24) - 3         # the largest shift stays below 2^24
    rng = np.random.default_rng(0)
    for _ in range(200):
        args = (float(rng.uniform(0, 600)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)))
        assert stereo_gains(*args) == R.stereo_gains(*args)
    for bad in [(-1, 0.5, 0.5), (float("nan"), 0.5, 0.5), (float("inf"), 0.5, 0.5), (65536, 0.5, 0.5), (48, 1.01, 0.5),
                (48, -0.01, 0.5), (48, 0.5, 1.5), (48, 0.5, float("nan")), (True, 0.5, 0.5), ("48", 0.5, 0.5)]:
        with pytest.raises(ValueError):
            stereo_gains(*bad)
    from video_3d_pipeline.convert import DepthTo3DConverter
    with pytest.raises(ValueError, match="layout"):
        DepthTo3DConverter(layout="anaglyph", backend=RefRenderBackend())


def test_rgb_png_round_trip_through_pillow(tmp_path):
    import io
    from PIL import Image
    from video_3d_pipeline.utils import PngWriterPool, encode_png8
    rng = np.random.default_rng(4)
    for (h, w) in ((1, 1), (3, 7), (17, 64), (96, 768)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        with Image.open(io.BytesIO(encode_png8(a))) as im:
            assert im.mode == "RGB" and im.size == (w, h) and np.array_equal(np.asarray(im), a)
        with Image.open(io.BytesIO(encode_png8(a, bgr=True))) as im:
            assert np.array_equal(np.asarray(im), a[..., ::-1])
    with pytest.raises(ValueError):
        encode_png8(np.zeros((4, 4), np.uint8))
    from video_3d_pipeline.convert import png_rgb_from_bgr
    imgs = [rng.integers(0, 256, (9, 13, 3), dtype=np.uint8) for _ in range(6)]
    with PngWriterPool(workers=3, max_pending=2) as pool:
        for i, a in enumerate(imgs):
            pool.submit(tmp_path / f"frame_{i:06d}.png", a, encode=png_rgb_from_bgr)
    got = _read_clip(tmp_path)                                            # iter_frames gives BGR back
    assert len(got) == 6 and all(np.array_equal(g, a) for g, a in zip(got, imgs))


def test_render_frame_numpy_surface():
    from video_3d_pipeline.convert import DepthTo3DConverter
    F, D = _clip4k(1)[0], _depths(1)[0]
    conv = DepthTo3DConverter(max_shift=20, eye_split=0.25, layout="half-sbs", backend=RefRenderBackend())
    assert np.array_equal(conv.render_frame(F, D), R.render(F, D, *R.stereo_gains(20, 0.5, 0.25), R.HALF_SBS))
    with pytest.raises(ValueError):
        conv.render_frame(F, D[:, 1:])


# ---------------------------------------------------------------- the pipeline's --stereo-output

@pytest.fixture()
def sbs_clips(tmp_path):
    from video_3d_pipeline import synthetic as syn
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(5)])
    rng = np.random.default_rng(7)
    guides = rng.integers(0, 256, (6, H4, W4, 3), dtype=np.uint8)       # colour 4K frames: the stereo frames' source
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", guides)
    np.save(tmp_path / "v4k_short.npy", guides[:4])
    return tmp_path, str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), str(tmp_path / "v4k_short.npy")


def _pipeline(tmp, sbs, v4k, tag, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp / f"w_{tag}"), batch_size=2, stereo_only=True, guide_batch=3,
                                backend=RefStereoPipelineBackend())
    out = pipe.run(sbs, v4k, output_path=str(tmp / f"depth_{tag}.json"), **kw)
    return json.loads(open(out).read())


@pytest.mark.parametrize("layout", ["full-sbs", "half-sbs"])
def test_pipeline_stereo_output_equals_the_convert_cli(sbs_clips, layout):
    tmp, sbs, v4k, _ = sbs_clips
    plain = _pipeline(tmp, sbs, v4k, "plain", guide_start_frame=1)
    opts = dict(max_shift=25.0, convergence=0.4, eye_split=0.7, layout=layout)
    man = _pipeline(tmp, sbs, v4k, "st", guide_start_frame=1, stereo_output=str(tmp / "st3d.json"), stereo_options=opts)
    assert _pngs(man["frames_dir"]) == _pngs(plain["frames_dir"])          # the depth files do not change
    assert sorted(os.listdir(man["frames_dir"])) == [f"depth4k_{i:06d}.png" for i in range(5)]
    rc = _run([v4k, tmp / "depth_st.json", "--output", tmp / "cli3d.json", "--guide-start-frame", "1", "--layout", layout,
               "--max-shift", "25", "--convergence", "0.4", "--eye-split", "0.7"])
    assert rc == 0
    want = json.loads((tmp / "cli3d.json").read_text())
    got = json.loads((tmp / "st3d.json").read_text())
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"]) and len(_pngs(got["frames_dir"])) == 6
    assert {k: v for k, v in got.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}


def test_pipeline_without_a_4k_frame_writes_no_stereo_frame(sbs_clips):
    tmp, sbs, _, short = sbs_clips
    _pipeline(tmp, sbs, short, "short", stereo_output=str(tmp / "short3d.json"))
    got = json.loads((tmp / "short3d.json").read_text())
    assert got["count"] == 4 and sorted(os.listdir(got["frames_dir"])) == [f"frame_{i:06d}.png" for i in range(4)] + ["info.json"]


def test_pipeline_cli_takes_the_stereo_flags():
    from video_3d_pipeline import pipeline
    res = subprocess.run([sys.executable, "-m", "video_3d_pipeline.pipeline", "--help"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0 and "--stereo-output" in res.stdout and "--eye-split" in res.stdout and "--layout" in res.stdout
    assert pipeline.main(["a.npy", "b.npy", "--stereo-output", "x.json", "--max-shift", "-3", "--device", "cpu"]) == 1


def test_convert_is_exported_and_runs_as_module():
    import video_3d_pipeline as v
    from video_3d_pipeline.convert import DepthTo3DConverter
    assert v.DepthTo3DConverter is DepthTo3DConverter
    res = subprocess.run([sys.executable, "-m", "video_3d_pipeline.convert", "--help"], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0
    for flag in ("--layout", "--max-shift", "--convergence", "--eye-split", "--max-frames", "--force", "--guide-start-frame",
                 "--alignment-file", "--output"):
        assert flag in res.stdout, flag


# ---------------------------------------------------------------- torchrun: frame i -> rank i mod world

def _convert_worker(rank, world, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for p in (ROOT, os.path.join(ROOT, "video-3d-pipeline_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from video_3d_pipeline import sharding
    from video_3d_pipeline.convert import DepthTo3DConverter
    from test_convert_host import RefRenderBackend
    sharding.init_process_group("gloo")
    conv = DepthTo3DConverter(layout="half-sbs", backend=RefRenderBackend(), batch_size=2)
    conv.process_conversion(os.path.join(tmp, "v4k.npy"), os.path.join(tmp, "depth_4k_frames"), os.path.join(tmp, "w2.json"),
                            guide_start_frame=1)
    assert conv.last_rendered_frames == len(range(rank, 5, world))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_world2_gloo_equals_one_process(inputs):
    from video_3d_pipeline.convert import DepthTo3DConverter
    tmp, _, _ = inputs
    DepthTo3DConverter(layout="half-sbs", backend=RefRenderBackend()).process_conversion(
        str(tmp / "v4k.npy"), str(tmp / "depth_4k_frames"), str(tmp / "w1.json"), guide_start_frame=1)
    port = 29600 + (os.getpid() % 2000)
    mp.spawn(_convert_worker, args=(2, port, str(tmp)), nprocs=2, join=True)
    one, two = json.loads((tmp / "w1.json").read_text()), json.loads((tmp / "w2.json").read_text())
    assert _pngs(two["frames_dir"]) == _pngs(one["frames_dir"]) and two["count"] == one["count"] == 5
