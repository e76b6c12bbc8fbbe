"""Host logic of the one-pass SBS -> 4K depth pipeline (video_3d_pipeline.pipeline) on CPU.  Oracle-backed stand-ins take the
place of the HIP backends, as in test_host.py: the pipeline's files must equal, byte for byte, what the depth CLI followed by
the upscale CLI write with the same stand-ins."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from test_host import OracleStereoBackend, OracleUpscaleBackend

SW, SH = 192, 48                      # SBS frame; the unsqueezed depth is SW x SH, the "4K" frame 2SW x 2SH


class OraclePipelineBackend(OracleStereoBackend):
    """test-only stand-in for pipeline.HipPipelineBackend; records the guided batch sizes"""

    def __init__(self):
        self.guided_batches = []

    def guide_luma(self, frames, height, width, capacity):
        assert len(frames) <= capacity
        return np.stack([np.full((height, width), 128, np.uint8) if f is None else (f if f.ndim == 2 else O.bgr_to_gray(f))
                         for f in frames])

    def guided_upscale_u16(self, u16, luma, r, eps):
        self.guided_batches.append(len(u16))
        return np.stack([np.clip(np.rint(O.guided_upscale(d.astype(np.float32), g, r, eps).astype(np.float32)), 0, 65535)
                         .astype(np.uint16) for d, g in zip(u16, luma)])


@pytest.fixture()
def clips(tmp_path):
    from video_3d_pipeline import synthetic as syn
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(5)])
    guides = np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(6)])
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", guides)
    np.save(tmp_path / "v4k_short.npy", guides[:4])
    return str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), str(tmp_path / "v4k_short.npy")


def _two_clis(tmp_path, sbs, v4k, tag, start_frame=0, max_frames=None, guide_start_frame=0):
    """depth CLI + upscale CLI with oracle backends -> (upscaler, {name: bytes} of the 4K PNGs, depth cache dir)"""
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True, backend=OracleStereoBackend())
    ddir = ex.process_video_sbs(sbs, start_frame=start_frame, max_frames=max_frames)
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    out = up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / f"cli_{tag}.json"), guide_start_frame=guide_start_frame)
    return up, _pngs(json.loads(open(out).read())["frames_dir"]), ddir


def _pipeline(tmp_path, sbs, v4k, tag, batch_size=2, guide_batch=8, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=batch_size, stereo_only=True,
                                guide_batch=guide_batch, backend=OraclePipelineBackend())
    out = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **kw)
    man = json.loads(open(out).read())
    return pipe, man, _pngs(man["frames_dir"])


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_pipeline_files_equal_the_two_clis(tmp_path, clips):
    """5 frames in passes of 2 (a clip length that is not a multiple of the pass), guided batches of 8, 1 and 3"""
    sbs, v4k, _ = clips
    _, want, _ = _two_clis(tmp_path, sbs, v4k, "a")
    assert list(want) == [f"depth4k_{i:06d}.png" for i in range(5)]
    pipe, man, got = _pipeline(tmp_path, sbs, v4k, "a")
    assert got == want
    assert (man["count"], man["width"], man["height"], man["pattern"]) == (5, 2 * SW, 2 * SH, "depth4k_%06d.png")
    assert pipe.last_pass_frames == 2 and pipe.last_flat_guides == 0 and pipe.backend.guided_batches == [2, 2, 1]
    for gb, batches in ((1, [1] * 5), (3, [3, 2])):
        pipe, _, got = _pipeline(tmp_path, sbs, v4k, f"gb{gb}", batch_size=5, guide_batch=gb)
        assert got == want and pipe.backend.guided_batches == batches


def test_pipeline_start_and_guide_offsets(tmp_path, clips):
    sbs, v4k, _ = clips
    _, want, _ = _two_clis(tmp_path, sbs, v4k, "off", start_frame=1, max_frames=3, guide_start_frame=1)
    _, man, got = _pipeline(tmp_path, sbs, v4k, "off", start_frame=1, max_frames=3, guide_start_frame=1)
    assert len(want) == 3 and got == want and man["count"] == 3
    _, _, shifted = _pipeline(tmp_path, sbs, v4k, "off0", start_frame=1, max_frames=3)
    assert shifted != got                                           # the offset really selects other guide frames


def test_pipeline_short_4k_clip_uses_a_flat_guide(tmp_path, clips, capsys):
    sbs, _, short = clips
    up, want, _ = _two_clis(tmp_path, sbs, short, "short")
    pipe, _, got = _pipeline(tmp_path, sbs, short, "short")
    assert up.last_flat_guides == 1 and pipe.last_flat_guides == 1 and got == want
    assert "4K guide video ended after 4" in capsys.readouterr().out


def test_pipeline_keeps_depth_maps_in_the_depth_cache(tmp_path, clips):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    sbs, v4k, _ = clips
    _, _, ddir = _two_clis(tmp_path, sbs, v4k, "keep")
    pipe, _, _ = _pipeline(tmp_path, sbs, v4k, "keep", keep_depth_maps=True)
    cache = pipe.extractor.get_cache_path(sbs, 0, 5)
    assert cache.parent == tmp_path / "pipe_keep" and cache.name == ddir.name
    assert _pngs(cache) == _pngs(ddir)
    ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / "pipe_keep"), cache_dir=str(tmp_path / "pipe_keep"), stereo_only=True,
                                    backend=OracleStereoBackend())
    ex.backend = None                                               # a later depth CLI run finds them cached: nothing computed
    assert ex.process_video_sbs(sbs) == cache
    _, _, _ = _pipeline(tmp_path, sbs, v4k, "nokeep")
    assert not any((tmp_path / "pipe_nokeep").glob("depth_*/depth_*.png"))


def test_pipeline_skips_existing_output_unless_forced(tmp_path, clips):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs, v4k, _ = clips
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w"), batch_size=4, stereo_only=True, backend=OraclePipelineBackend())
    out = str(tmp_path / "o.json")
    assert pipe.run(sbs, v4k, output_path=out, max_frames=2) == out
    assert len(pipe.backend.guided_batches) == 1
    assert pipe.run(sbs, v4k, output_path=out, max_frames=2) == out   # exists: nothing recomputed
    assert len(pipe.backend.guided_batches) == 1
    assert pipe.run(sbs, v4k, output_path=out, max_frames=2, force_reprocess=True) == out
    assert len(pipe.backend.guided_batches) == 2
    # no --output: named after the depth cache directory, like the upscale CLI's default for that directory
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        res = pipe.run(sbs, v4k, max_frames=2)
    finally:
        os.chdir(cwd)
    assert res == f"depth_4k_{pipe.extractor.get_cache_path(sbs, 0, 2).name}.mp4" and (tmp_path / res).exists()


def test_pipeline_errors(tmp_path, clips, capsys, monkeypatch):
    import torch
    from video_3d_pipeline import pipeline
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs, v4k, _ = clips
    rc = pipeline.main([str(tmp_path / "none.npy"), v4k, "--work-dir", str(tmp_path / "w"), "--stereo-only"])
    assert rc == 1 and "Error:" in capsys.readouterr().out
    rc = pipeline.main([sbs, str(tmp_path / "none.npy"), "--work-dir", str(tmp_path / "w"), "--device", "cpu"])
    assert rc == 1 and "Error:" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        pipeline.main(["--definitely-not-a-flag"])
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w"), stereo_only=True, backend=OraclePipelineBackend())
    with pytest.raises(ValueError, match="Could not read video info"):
        pipe.run(sbs, str(tmp_path / "none.npy"), output_path=str(tmp_path / "o.json"))
    with pytest.raises(ValueError, match="Could not read video info"):
        pipe.run(str(tmp_path / "none.npy"), v4k, output_path=str(tmp_path / "o.json"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="CUDA not available but requested"):
            SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w"))
    import torch.distributed as dist
    if not dist.is_initialized():                                 # WORLD_SIZE > 1 without a process group never shards silently
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("RANK", "1")
        with pytest.raises(RuntimeError, match="not initialised"):
            pipe.run(sbs, v4k, output_path=str(tmp_path / "o2.json"))


def test_pipeline_is_exported_and_runs_as_module():
    import subprocess
    import sys
    import video_3d_pipeline as v
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    assert v.SbsTo4kDepthPipeline is SbsTo4kDepthPipeline
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "video_3d_pipeline.pipeline", "--help"], cwd=root, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0 and "--keep-depth-maps" in res.stdout and "--guide-start-frame" in res.stdout
