"""Host side of `--temporal-motion` on the CPU: what the compensated window does for the depth on panning and moving synthetic
clips (oracle matcher, 320x120, 9 frames, sigma-3 noise, R = 2, tau = 12, S = 16), the streaming driver, both CLIs with
oracle-backed stand-ins whose temporal methods come from tests/temporal_mc_ref.py, block sharding, and the off switch."""
import json
import os

import numpy as np
import pytest

import temporal_mc_ref as MR
import temporal_ref as TR
from oracle import oracle as O
from test_host import OracleStereoBackend, OracleUpscaleBackend  # noqa: F401
from test_pipeline_host import OraclePipelineBackend
from test_temporal_host import TemporalPipelineBackend, TemporalStereoBackend, _NumpyBackend, _pngs

W, H, T, R, TAU, S = 320, 120, 9, 2, 12, 16
SW, SH, NF, CLI_PAN, CLI_S = 192, 48, 7, 4, 4


# ---------------------------------------------------------------- quality on the synthetic clips

_runs = {}


def _run(pan, cut_at=None):
    """(left gray, ground truth, per-frame depth, the uncompensated stage's depth and cuts, the compensated stage's depth and
    cuts) of one clip, computed once"""
    key = (pan, cut_at)
    if key not in _runs:
        from video_3d_pipeline import synthetic as syn
        L, Rt, gt = syn.temporal_pan_clip(W, H, T, pan, cut_at=cut_at)
        depth = np.stack([O.disp_to_depth(O.sgbm_compute(l, r)) for l, r in zip(L, Rt)])
        F, Bk, resid = MR.fields(L, S)
        cut = MR.cuts(resid, 20, W, H)
        old_cut = TR.cuts(L, 20)
        old = TR.filter_clip(depth, L, R, TAU, old_cut, 1)
        new = MR.filter_clip(depth, L, R, TAU, cut, F, Bk, 1)
        print(f"pan {pan} cut_at {cut_at}: compensated residual per pixel {np.round(resid / (W * H), 1)}")
        _runs[key] = dict(L=L, gt=gt, depth=depth, old=old, old_cut=old_cut, new=new, cut=cut)
    return _runs[key]


def _pairs(d, pan):
    """(frame t at x, frame t-1 at x + pan): the same scene point under a pan of `pan` pixels per frame"""
    return d[1:, :, :W - pan], d[:-1, :, pan:]


def _background_pairs(run, pan):
    """columns >= 80 (past the matcher's blind band), off the object (|gt - 40| > 1) in both frames, valid in both per-frame maps"""
    ga, gb = _pairs(run["gt"], pan)
    a, b = _pairs(run["depth"], pan)
    return (np.arange(W - pan) >= 80)[None, None] & (np.abs(ga - 40) > 1) & (np.abs(gb - 40) > 1) & (a > 0) & (b > 0)


def _flicker(d, pan, mask):
    a, b = _pairs(d, pan)
    return float(np.abs(a - b)[mask].mean())


@pytest.mark.parametrize("pan", [3, 5, 11])
def test_pan_background_flicker(pan):
    """the uncompensated stage flags every pair of a pan as a cut and returns the per-frame depth; with motion the background's
    flicker along the pan falls to at most 0.75 of the per-frame path's (measured: 0.57 .. 0.59)"""
    run = _run(pan)
    assert run["old_cut"].sum() == 8 and np.array_equal(run["old"], run["depth"])
    assert not run["cut"].any()
    mask = _background_pairs(run, pan)
    assert mask.mean() > 0.3
    f_frame, f_mc = _flicker(run["depth"], pan, mask), _flicker(run["new"], pan, mask)
    print(f"pan {pan}: background flicker along the pan {f_frame:.4f} -> {f_mc:.4f} px ({f_mc / f_frame:.3f}x)")
    assert f_mc <= 0.75 * f_frame


def test_pan_keeps_the_background_error_and_the_valid_share():
    run = _run(5)
    bg = (np.arange(W) >= 80)[None, None] & (np.abs(run["gt"] - 40) > 1) & (run["depth"] > 0)
    e_frame, e_mc = float(np.abs(run["depth"] - run["gt"])[bg].mean()), float(np.abs(run["new"] - run["gt"])[bg].mean())
    inv_frame, inv_mc = float((run["depth"] <= 0).mean()), float((run["new"] <= 0).mean())
    print(f"pan 5: background error {e_frame:.4f} -> {e_mc:.4f} px; invalid {inv_frame:.4f} -> {inv_mc:.4f}")
    assert e_mc <= e_frame and inv_mc <= inv_frame


def test_still_camera_moving_object():
    """pan 0: the static background keeps what the uncompensated stage gives it (at most 1.05x its flicker; measured 1.014x), the
    moving rectangle now has neighbours (flicker along its own motion at most 0.5x the per-frame path's; measured 0.33x) and its
    error against ground truth stays within the existing stage's margin (1.05x; measured 1.004x)"""
    from video_3d_pipeline import synthetic as syn
    run = _run(0)
    assert not run["old_cut"].any() and not run["cut"].any()
    mask = _background_pairs(run, 0)
    s_old, s_mc = _flicker(run["old"], 0, mask), _flicker(run["new"], 0, mask)
    boxes = [syn.temporal_object_box(W, H, t) for t in range(T)]

    def object_flicker(d):
        diffs = []
        for t in range(1, T):
            (x0, y0, x1, y1), (px0, _, px1, _) = boxes[t], boxes[t - 1]
            rows = slice(y0 + 2, y1 - 2)
            valid = (run["depth"][t, rows, x0 + 2:x1 - 2] > 0) & (run["depth"][t - 1, rows, px0 + 2:px1 - 2] > 0)
            diffs.append(np.abs(d[t, rows, x0 + 2:x1 - 2] - d[t - 1, rows, px0 + 2:px1 - 2])[valid])
        return float(np.concatenate(diffs).mean())

    obj = np.zeros((T, H, W), bool)
    for t, (x0, y0, x1, y1) in enumerate(boxes):
        obj[t, y0 + 2:y1 - 2, x0 + 2:x1 - 2] = True
    obj &= run["depth"] > 0
    o_frame, o_mc = object_flicker(run["depth"]), object_flicker(run["new"])
    e_frame, e_mc = float(np.abs(run["depth"] - run["gt"])[obj].mean()), float(np.abs(run["new"] - run["gt"])[obj].mean())
    print(f"pan 0: static flicker {s_old:.4f} (uncompensated) -> {s_mc:.4f}; object flicker {o_frame:.4f} -> {o_mc:.4f}; "
          f"object error {e_frame:.4f} -> {e_mc:.4f}")
    assert s_mc <= 1.05 * s_old
    assert o_mc <= 0.5 * o_frame
    assert e_mc <= 1.05 * e_frame


def test_compensated_cut_rule_finds_the_scene_change_in_a_pan():
    run = _run(5, cut_at=5)
    assert run["old_cut"].sum() == 8
    assert list(run["cut"]) == [0, 0, 0, 0, 0, 1, 0, 0, 0]


# ---------------------------------------------------------------- the streaming driver

class _MotionMethods:
    """temporal_stabilize as HipStereoBackend has it with this feature: the keyword is optional"""

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill, motion_search=0):
        self.seen_motion = getattr(self, "seen_motion", []) + [motion_search]
        if motion_search > 0:
            return MR.stabilize(depth, gray, radius, motion_search, tau, cut_threshold, int(fill), t0, n)
        return TR.stabilize(depth, gray, radius, tau, cut_threshold, int(fill), t0, n)


class _NumpyMotionBackend(_MotionMethods):
    temporal_concat = _NumpyBackend.temporal_concat


class MotionStereoBackend(_MotionMethods, TemporalStereoBackend):
    pass


class MotionPipelineBackend(_MotionMethods, TemporalPipelineBackend):
    pass


@pytest.mark.parametrize("Tn", [1, 7, 11])
def test_streaming_equals_the_whole_clip_call(Tn):
    from video_3d_pipeline.temporal import TemporalStabilizer
    rng = np.random.default_rng(Tn)
    Hh, Ww, Ss = 20, 37, 3
    big = rng.integers(0, 256, (Hh, Ww + 2 * Tn)).astype(np.int64)
    gray = np.stack([big[:, 2 * t:2 * t + Ww] for t in range(Tn)])                  # a pan of 2 px per frame
    gray = np.clip(gray + rng.integers(-6, 7, gray.shape), 0, 255).astype(np.uint8)
    if Tn > 4:
        gray[4:] = 255 - gray[4:]                                                   # a scene cut inside the clip
    depth = (rng.integers(0, 1024, (Tn, Hh, Ww)) / 16.0).astype(np.float32)
    for Rr in (1, 2, 8):
        want = MR.stabilize(depth, gray, Rr, Ss)
        if Tn > 4:
            assert (want != TR.stabilize(depth, gray, Rr)).any()
        for step in (1, 2, 3, 5):
            st = TemporalStabilizer(_NumpyMotionBackend(), Rr, motion_search=Ss)
            parts = []
            for i in range(0, Tn, step):
                out = st.push(depth[i:i + step].copy(), gray[i:i + step].copy())
                parts += [] if out is None else [out]
            out = st.finish()
            parts += [] if out is None else [out]
            assert np.array_equal(np.concatenate(parts), want), (Rr, step)
            assert set(st.backend.seen_motion) == {Ss}


def test_parameter_checks():
    from video_3d_pipeline.temporal import (BlockStabilizer, TemporalStabilizer, cache_suffix, check_motion_search, manifest_entry,
                                            temporal_options)
    assert check_motion_search(0, 0) == 0 and check_motion_search(32, 1) == 32
    for bad in ((33, 2), (-1, 2), (1.5, 2), (True, 2), (4, 0)):
        with pytest.raises(ValueError):
            check_motion_search(*bad)
    with pytest.raises(ValueError):
        TemporalStabilizer(_NumpyMotionBackend(), 2, motion_search=33)
    assert BlockStabilizer(_NumpyMotionBackend(), (2, 12, 20, True), 0, 3, 0, motion_search=5).stab.motion_search == 5
    assert cache_suffix(2, 12, 20, True, 10000, 0) == cache_suffix(2, 12, 20, True)
    assert cache_suffix(2, 12, 20, True, 10000, 16) == cache_suffix(2, 12, 20, True) + "_m16"
    assert cache_suffix(2, 12, 20, True, 9800, 16) == "_temporal_r2_t12_c20_f1_m16_rangeq9800"
    assert manifest_entry(2, 12, 20, True) == manifest_entry(2, 12, 20, True, 10000, 0) and "motion_search" not in manifest_entry(2, 12, 20, True)
    assert manifest_entry(2, 12, 20, True, 10000, 16)["motion_search"] == 16

    class Old:                                               # an argument namespace built before the option existed
        temporal_radius, temporal_tau, temporal_cut, no_temporal_fill = 2, 12, 20, False

    assert temporal_options(Old())["temporal_motion"] == 0


# ---------------------------------------------------------------- the CLIs

@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("mcclips")
    np.save(d / "sbs.npy", syn.temporal_pan_sbs_clip(SW, SH, NF, CLI_PAN, cut_at=4, speed=4))
    rng = np.random.default_rng(5)
    np.save(d / "v4k.npy", rng.integers(0, 256, (NF, 2 * SH, 2 * SW, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


def _depth_cli(tmp_path, sbs, tag, backend, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=3, stereo_only=True, backend=backend, **kw)
    return ex, ex.process_video_sbs(sbs)


def _pipeline(tmp_path, sbs, v4k, tag, backend, run_kw=None, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=3, stereo_only=True, guide_batch=2, backend=backend, **kw)
    out = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **(run_kw or {}))
    return pipe, json.loads(open(out).read())


def test_motion_zero_changes_nothing(tmp_path, clips):
    """S = 0: the stand-ins of tests/test_temporal_host.py, whose temporal_stabilize has no such keyword, still serve; the files
    are byte-identical and the cache key is the same"""
    sbs, v4k = clips
    _, want_dir = _depth_cli(tmp_path, sbs, "r2", TemporalStereoBackend(), temporal_radius=2)
    ex, zero_dir = _depth_cli(tmp_path, sbs, "r2m0", TemporalStereoBackend(), temporal_radius=2, temporal_motion=0)
    assert zero_dir.name == want_dir.name and _pngs(zero_dir) == _pngs(want_dir) and len(_pngs(zero_dir)) == NF
    assert json.loads((zero_dir / "temporal.json").read_text()) == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True}
    _, want = _pipeline(tmp_path, sbs, v4k, "r2", TemporalPipelineBackend(), temporal_radius=2)
    _, zero = _pipeline(tmp_path, sbs, v4k, "r2m0", TemporalPipelineBackend(), temporal_radius=2, temporal_motion=0)
    assert _pngs(zero["frames_dir"]) == _pngs(want["frames_dir"])
    assert {k: v for k, v in zero.items() if k != "frames_dir"} == {k: v for k, v in want.items() if k != "frames_dir"}
    # and with the whole stage off the key is the reference's
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", OracleStereoBackend())
    _, off_dir = _depth_cli(tmp_path, sbs, "off", OracleStereoBackend(), temporal_motion=0)
    assert off_dir.name == plain_dir.name and _pngs(off_dir) == _pngs(plain_dir)


def test_motion_without_a_radius_is_refused(tmp_path, clips):
    from video_3d_pipeline import depth as depth_mod
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    with pytest.raises(ValueError, match="temporal-radius"):
        depth_mod.HybridStereoDepthExtractor(work_dir=str(tmp_path / "x"), cache_dir=str(tmp_path / "x"), stereo_only=True,
                                             backend=OracleStereoBackend(), temporal_motion=8)
    with pytest.raises(ValueError):
        SbsTo4kDepthPipeline(work_dir=str(tmp_path / "y"), stereo_only=True, backend=OraclePipelineBackend(), temporal_motion=8)
    with pytest.raises(ValueError):
        depth_mod.HybridStereoDepthExtractor(work_dir=str(tmp_path / "x"), cache_dir=str(tmp_path / "x"), stereo_only=True,
                                             backend=OracleStereoBackend(), temporal_radius=2, temporal_motion=33)
    assert depth_mod.main([clips[0], "--work-dir", str(tmp_path / "z"), "--stereo-only", "--temporal-motion", "8"]) == 1


def test_depth_cli_and_pipeline_with_motion(tmp_path, clips):
    from video_3d_pipeline import depth as depth_mod
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    from video_3d_pipeline.utils import iter_frames, read_png16
    sbs, v4k = clips
    _, r2_dir = _depth_cli(tmp_path, sbs, "r2", TemporalStereoBackend(), temporal_radius=2)
    be = MotionStereoBackend()
    ex, ddir = _depth_cli(tmp_path, sbs, "m", be, temporal_radius=2, temporal_motion=CLI_S)
    assert set(be.seen_motion) == {CLI_S}
    assert ddir.name != r2_dir.name
    assert ddir.name != _depth_cli(tmp_path, sbs, "m5", MotionStereoBackend(), temporal_radius=2, temporal_motion=CLI_S + 1)[1].name
    entry = {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True, "motion_search": CLI_S}
    assert json.loads((ddir / "temporal.json").read_text()) == entry
    frames = list(iter_frames(sbs))
    depth = OracleStereoBackend().sbs_to_disparity(frames, True)
    gray = np.stack([O.sbs_to_gray(f, True)[0] for f in frames])
    want = MR.stabilize(depth, gray, 2, CLI_S)
    _, _, resid = MR.fields(gray, CLI_S)
    assert list(MR.cuts(resid, 20, SW, SH)) == [0, 0, 0, 0, 1, 0, 0] and TR.cuts(gray, 20).sum() > 1
    got = np.stack([read_png16(ddir / f"depth_{i:06d}.png") for i in range(NF)])
    assert np.array_equal(got, want)
    assert (got != np.stack([read_png16(r2_dir / f"depth_{i:06d}.png") for i in range(NF)])).any()
    # the one-pass pipeline writes the two-CLI route's files and carries the option in its manifest
    up = SimpleDepthUpscaler(backend=OracleUpscaleBackend())
    want4k = _pngs(json.loads(open(up.process_depth_upscaling(str(ddir), v4k, output_path=str(tmp_path / "cli.json"))).read())["frames_dir"])
    pipe, man = _pipeline(tmp_path, sbs, v4k, "m", MotionPipelineBackend(), run_kw=dict(keep_depth_maps=True), temporal_radius=2,
                          temporal_motion=CLI_S)
    assert len(want4k) == NF and _pngs(man["frames_dir"]) == want4k and man["temporal"] == entry
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)
    # the command lines reach the constructors
    seen = {}

    class Spy(depth_mod.HybridStereoDepthExtractor):
        def __init__(self, **kw):
            seen.update(kw)
            raise RuntimeError("stop here")

    orig = depth_mod.HybridStereoDepthExtractor
    depth_mod.HybridStereoDepthExtractor = Spy
    try:
        assert depth_mod.main([sbs, "--temporal-radius", "3", "--temporal-motion", "12"]) == 1
    finally:
        depth_mod.HybridStereoDepthExtractor = orig
    assert (seen["temporal_radius"], seen["temporal_motion"]) == (3, 12)
    import argparse
    parser = argparse.ArgumentParser()
    depth_mod.add_depth_arguments(parser, "force")
    assert depth_mod.depth_options(parser.parse_args([]))["temporal_motion"] == 0
    assert depth_mod.depth_options(parser.parse_args(["--temporal-motion", "7"]))["temporal_motion"] == 7


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_write_what_one_process_writes(tmp_path, clips, monkeypatch, world):
    """contiguous blocks with a halo of R frames give the single-process files with motion on too: the fields only use adjacent
    pairs inside the window"""
    from video_3d_pipeline import sharding
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs, v4k = clips
    kw = dict(batch_size=2, stereo_only=True, temporal_radius=2, temporal_motion=CLI_S)
    one = HybridStereoDepthExtractor(work_dir=str(tmp_path / "o"), cache_dir=str(tmp_path / "o"), backend=MotionStereoBackend(), **kw)
    want_dir = one.process_video_sbs(sbs)
    pone = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "po"), guide_batch=2, backend=MotionPipelineBackend(), **kw)
    want4k = json.loads(open(pone.run(sbs, v4k, output_path=str(tmp_path / "po.json"))).read())
    with monkeypatch.context() as mp:
        mp.setattr(sharding, "_initialized", lambda: True)
        mp.setattr(sharding, "barrier", lambda: None)
        mp.setattr(sharding, "total", lambda v: NF)
        mp.setenv("WORLD_SIZE", str(world))
        for rank in reversed(range(world)):
            mp.setenv("RANK", str(rank))
            ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / "w"), cache_dir=str(tmp_path / "w"), backend=MotionStereoBackend(), **kw)
            got_dir = ex.process_video_sbs(sbs, force_reprocess=True)
            pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "pw"), guide_batch=2, backend=MotionPipelineBackend(), **kw)
            out4k = pipe.run(sbs, v4k, output_path=str(tmp_path / "pw.json"), force_reprocess=True)
    got4k = json.loads(open(out4k).read())
    assert len(_pngs(want_dir)) == NF and _pngs(got_dir) == _pngs(want_dir), world
    assert got4k["count"] == NF and _pngs(got4k["frames_dir"]) == _pngs(want4k["frames_dir"]), world
