"""The one-pass SBS -> 4K depth pipeline on the MI355X: its two new kernels bit for bit against the routes they replace, and
its files byte for byte against the depth CLI followed by the upscale CLI (real HIP backends)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _u16(t):
    """int16-viewed u16 device tensor -> NumPy uint16"""
    return t.cpu().numpy().view(np.uint16)


def _as_float(u16):
    return (u16.to(torch.int32) & 0xFFFF).float().contiguous()


# ---------------------------------------------------------------- v3d_depth_to_u16_batch

@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 3, 34])
def test_depth_to_u16_batch_1080p(native, oracle, n):
    g = torch.Generator(device="cuda").manual_seed(n)
    d = torch.rand((n, 1080, 1920), generator=g, device="cuda") * 64
    scale = torch.logspace(-3, 6, n, device="cuda")[:, None, None]       # neighbouring frames with very different ranges
    d = (d * scale).contiguous()
    if n >= 3:
        d[1] = 7.25                                                       # flat frame: max == min -> 0
        d[2] = 0.0                                                        # all-zero frame
    got = native.depth_to_u16_batch(d)
    for f in range(n):
        assert np.array_equal(_u16(got[f]), _u16(native.depth_to_u16(d[f].contiguous()))), f
    for f in sorted({0, n // 2, n - 1, min(2, n - 1)}):
        assert np.array_equal(_u16(got[f]), oracle.depth_to_u16(d[f].cpu().numpy())), f
    if n >= 3:
        assert not _u16(got[1]).any() and not _u16(got[2]).any()
    assert all(_u16(got[f]).max() == 65535 for f in range(n) if f not in (1, 2))


@pytest.mark.timeout(120)
def test_depth_to_u16_batch_odd_sizes(native, oracle):
    rng = np.random.default_rng(3)
    for (H, W) in ((131, 257), (1, 1), (7, 255), (1, 65537)):
        a = (rng.random((5, H, W)) * rng.choice([1e-4, 1, 3e4], (5, 1, 1))).astype(np.float32)
        a[3] = -2.5                                                       # flat negative frame
        d = torch.from_numpy(a).cuda()
        got = native.depth_to_u16_batch(d)
        for f in range(5):
            want = oracle.depth_to_u16(a[f])
            assert np.array_equal(_u16(got[f]), want), (H, W, f)
            assert np.array_equal(_u16(native.depth_to_u16(d[f].contiguous())), want), (H, W, f)


# ---------------------------------------------------------------- v3d_guided_upscale_u16_batch

def _lo_hi(n, Wlo, Hlo, Whi, Hhi, seed, pad=0):
    """u16 depth (with 0 and 65535 present) and a guide whose frames lie `pad` bytes apart beyond their size (strided)"""
    from video_3d_pipeline import synthetic as syn
    rng = np.random.default_rng(seed)
    base = np.stack([syn.gt_disparity(Wlo, Hlo) for _ in range(n)]).astype(np.float64)
    lo = (base / base.max() * 65535 * rng.uniform(0.3, 1, (n, 1, 1))).astype(np.uint16)
    lo[:, :Hlo // 3, : Wlo // 4] = 0
    lo[:, -3:, -5:] = 65535
    lo[0, 0, -1] = 65535
    lo_t = torch.from_numpy(lo.view(np.int16)).cuda()
    gbuf = torch.from_numpy(rng.integers(0, 256, (n, Hhi * Whi + pad), dtype=np.uint8)).cuda()
    guide = gbuf[:, :Hhi * Whi].view(n, Hhi, Whi)
    return lo_t, guide


def _check_u16_route(native, lo, guide, r, what):
    got = native.guided_upscale_u16_batch(lo, guide, r, 1e-3)
    want = native.round_to_u16(native.guided_upscale_batch(_as_float(lo), guide, r, 1e-3))
    a, b = _u16(got), _u16(want)
    assert np.array_equal(a, b), f"{what}: {(a != b).sum()} of {a.size} samples differ"
    return a


@pytest.mark.timeout(300)
@pytest.mark.parametrize("r", [3, 4, 8, 16])
def test_guided_u16_matches_float_then_round(native, r):
    for (Wlo, Hlo, Whi, Hhi, pad) in ((200, 70, 400, 140, 0),           # exact 2x, dense guides
                                      (208, 66, 416, 132, 96),           # exact 2x, strided guides
                                      (96, 54, 384, 108, 40)):           # --no-unsqueeze geometry: 4x across, 2x down
        lo, guide = _lo_hi(3, Wlo, Hlo, Whi, Hhi, r + Wlo, pad)
        assert guide.stride(0) == Whi * Hhi + pad
        a = _check_u16_route(native, lo, guide, r, f"r={r} {Wlo}x{Hlo}->{Whi}x{Hhi}")
        assert a.max() > 30000 and (a == 0).any()


@pytest.mark.timeout(300)
def test_guided_u16_other_routes(native):
    """the two-sweep route (gf_fused 0) and the tiled route (gf_tiled 1) for r in {4, 8}; each option is restored"""
    lo, guide = _lo_hi(2, 232, 70, 464, 140, 11, 24)
    try:
        for key, val in (("gf_fused", 0), ("gf_tiled", 1)):
            native.set_option(key, val)
            try:
                for r in (4, 8):
                    _check_u16_route(native, lo, guide, r, f"{key}={val} r={r}")
            finally:
                native.set_option(key, 1 - val)
    finally:
        assert native.get_option("gf_fused") == 1 and native.get_option("gf_tiled") == 0


@pytest.mark.timeout(300)
def test_guided_u16_full_4k_frames(native, oracle):
    """1920x1080 -> 3840x2160 (the product geometry), the pipeline's default batch, against the float route and the oracle"""
    from video_3d_pipeline import synthetic as syn
    lo, _ = _lo_hi(2, 1920, 1080, 2, 2, 5)
    guide = torch.from_numpy(np.stack([syn.guide_frame(1920, 1080, i) for i in range(2)])).cuda()
    a = _check_u16_route(native, lo, guide, 8, "4K")
    want = oracle.guided_upscale(_u16(lo[1]).astype(np.float32), guide[1].cpu().numpy(), 8, 1e-3)
    assert np.abs(a[1].astype(np.float64) - np.clip(np.rint(want), 0, 65535)).max() <= 1


# ---------------------------------------------------------------- the pipeline against the two CLIs

SW, SH = 384, 96


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("clips")
    np.save(d / "sbs.npy", np.stack([syn.sbs_frame(SW, SH, i) for i in range(7)]))
    g = np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(7)])
    np.save(d / "v4k.npy", g)
    np.save(d / "v4k_short.npy", g[:6])
    gn = np.stack([np.repeat(syn.guide_frame(SW // 2, SH, i, scale=2)[..., None], 3, axis=2) for i in range(7)])
    np.save(d / "v4k_sq.npy", np.ascontiguousarray(np.repeat(gn, 2, axis=2)))      # 4x across for --no-unsqueeze
    return {k: str(d / f"{k}.npy") for k in ("sbs", "v4k", "v4k_short", "v4k_sq")}


def _mono_stub(left_rgb_frames):
    """deterministic stand-in for DPT: a coarse map derived from the left view itself"""
    return [np.ascontiguousarray(f[::8, ::8, 1]).astype(np.float32) * 0.25 + 1 for f in left_rgb_frames]


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def _two_clis(tmp_path, tag, sbs, v4k, unsqueeze=True, mono=None, guide_start_frame=0):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=8, stereo_only=mono is None, unsqueeze_sbs=unsqueeze,
                                    mono_provider=mono)
    ddir = ex.process_video_sbs(sbs)
    up = SimpleDepthUpscaler()
    out = up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / f"cli_{tag}.json"), guide_start_frame=guide_start_frame)
    return up, _pngs(json.loads(open(out).read())["frames_dir"]), ddir


def _pipeline(tmp_path, tag, sbs, v4k, unsqueeze=True, mono=None, guide_batch=8, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=8, stereo_only=mono is None,
                                unsqueeze_sbs=unsqueeze, guide_batch=guide_batch, mono_provider=mono)
    out = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **kw)
    return pipe, _pngs(json.loads(open(out).read())["frames_dir"])


@pytest.mark.timeout(600)
def test_pipeline_equals_the_two_clis_on_gpu(native, tmp_path, clips):
    _, want, ddir = _two_clis(tmp_path, "a", clips["sbs"], clips["v4k"])
    assert len(want) == 7
    for gb in (8, 1, 3):                                    # guided batch sizes: identical bytes
        pipe, got = _pipeline(tmp_path, f"gb{gb}", clips["sbs"], clips["v4k"], guide_batch=gb, keep_depth_maps=gb == 3)
        assert got == want, gb
        assert pipe.last_flat_guides == 0
    cache = pipe.extractor.get_cache_path(clips["sbs"], 0, 7)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)       # --keep-depth-maps: the depth CLI's own bytes


@pytest.mark.timeout(600)
def test_pipeline_short_clip_offset_hybrid_and_squeezed(native, tmp_path, clips):
    up, want, _ = _two_clis(tmp_path, "short", clips["sbs"], clips["v4k_short"])
    pipe, got = _pipeline(tmp_path, "short", clips["sbs"], clips["v4k_short"], guide_batch=3)
    assert up.last_flat_guides == 1 and pipe.last_flat_guides == 1 and got == want
    _, want, _ = _two_clis(tmp_path, "off", clips["sbs"], clips["v4k"], guide_start_frame=1)
    _, got = _pipeline(tmp_path, "off", clips["sbs"], clips["v4k"], guide_start_frame=1)
    assert got == want
    _, want, _ = _two_clis(tmp_path, "mono", clips["sbs"], clips["v4k"], mono=_mono_stub)
    pipe, got = _pipeline(tmp_path, "mono", clips["sbs"], clips["v4k"], mono=_mono_stub)
    assert not pipe.extractor.stereo_only and got == want
    _, plain = _pipeline(tmp_path, "plain", clips["sbs"], clips["v4k"])
    assert plain != got                                     # the provider's maps really were blended in
    _, want, _ = _two_clis(tmp_path, "sq", clips["sbs"], clips["v4k_sq"], unsqueeze=False)
    _, got = _pipeline(tmp_path, "sq", clips["sbs"], clips["v4k_sq"], unsqueeze=False)
    assert got == want


# ---------------------------------------------------------------- two ranks on GPU 0 (gloo carries the barriers)

def _pipeline_worker(rank, world, port, tmp, sbs, v4k):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    for p in (ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from video_3d_pipeline import sharding
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sharding.init_process_group("gloo")
    pipe = SbsTo4kDepthPipeline(work_dir=os.path.join(tmp, "w2"), batch_size=2, stereo_only=True, guide_batch=1)
    pipe.run(sbs, v4k, output_path=os.path.join(tmp, "two.json"))
    assert pipe.last_decoded_frames == len(range(rank, 7, world))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_pipeline_two_ranks_share_one_gpu(native, tmp_path, clips):
    import torch.multiprocessing as mp
    _, want = _pipeline(tmp_path, "one", clips["sbs"], clips["v4k_short"])
    port = 29700 + (os.getpid() % 2000)
    mp.spawn(_pipeline_worker, args=(2, port, str(tmp_path), clips["sbs"], clips["v4k_short"]), nprocs=2, join=True)
    man = json.loads(open(tmp_path / "two.json").read())
    assert man["count"] == 7 and _pngs(man["frames_dir"]) == want
