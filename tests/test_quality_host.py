"""Host side of --quality-report on the CPU: the measures tell a good disparity from a bad one on the temporally coherent
synthetic clip through the oracle matcher, and the driver (video_3d_pipeline/quality.py inside both CLIs) with a stand-in backend
whose new methods come from tests/quality_ref.py: carries across passes, scene cuts, sharded runs, flags, files, cached runs.

The driver's clips hold the full-width eyes of synthetic.temporal_clip side by side and run with unsqueeze off, so the stand-in's
gray planes are the clip's own left and right views."""
import json
import os

import numpy as np
import pytest

import fill_ref as FR
import quality_ref as QR
import temporal_ref as TR
from oracle import oracle as O
from test_temporal_host import TemporalPipelineBackend, TemporalStereoBackend, _pngs

W, H = 320, 120


class _QualityMethods:
    """what HipStereoBackend adds for the report, NumPy: the planes of the latest pass and quality_ref on them"""

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None, fill_holes=False):
        pairs = [O.sbs_to_gray(f, unsqueeze) for f in frames]
        self._lg, self._rg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        disp = [O.sgbm_compute(l, r) for l, r in pairs]
        self._disp = np.stack([FR.fill_frame(d) if fill_holes else d for d in disp])
        return np.stack([O.disp_to_depth(d) for d in self._disp])

    def right_gray(self, n):
        return self._rg[:n]

    def last_disp16(self, n):
        return self._disp[:n]

    def quality_reproj(self, n, bad_thr):
        return QR.reproj(self._lg[:n], self._rg[:n], self._disp[:n], bad_thr)

    def quality_flicker(self, depth, gray, still, jump16):
        return QR.flicker(depth, gray, still, jump16)

    def quality_fetch(self, records):
        self.__dict__.setdefault("fetched", []).append(len(records))
        return np.array(records)

    def read_quality(self, handle, wait=True):
        return handle

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill, range_quantile=10000, observe=None):
        cut = TR.cuts(gray, cut_threshold)
        filt = TR.filter_clip(depth, gray, radius, tau, cut, int(fill), t0, n)
        if observe is not None:
            observe(filt, gray[t0:t0 + n])
        return TR.to_u16_range(filt, TR.ranges(TR.minmax(depth), cut, radius, t0, n))


class QualityStereoBackend(_QualityMethods, TemporalStereoBackend):
    pass


class QualityPipelineBackend(_QualityMethods, TemporalPipelineBackend):
    pass


@pytest.fixture(scope="module")
def clip3():
    """temporal_clip(320, 120, 3) and its oracle disparity, computed once"""
    from video_3d_pipeline import synthetic as syn
    L, R, _ = syn.temporal_clip(W, H, 3)
    return L, R, np.stack([O.sgbm_compute(l, r) for l, r in zip(L, R)])


@pytest.fixture(scope="module")
def cutclip(tmp_path_factory):
    """temporal_clip(320, 120, 4, cut_at=2) as a full-width side-by-side .npy clip, a random 4K clip, and the oracle's planes"""
    from video_3d_pipeline import synthetic as syn
    L, R, _ = syn.temporal_clip(W, H, 4, cut_at=2)
    d = tmp_path_factory.mktemp("qclips")
    np.save(d / "sbs.npy", np.repeat(np.concatenate([L, R], axis=2)[..., None], 3, axis=3))
    np.save(d / "v4k.npy", np.random.default_rng(4).integers(0, 256, (4, 2 * H, 2 * W, 3), dtype=np.uint8))
    disp = np.stack([O.sgbm_compute(l, r) for l, r in zip(L, R)])
    return str(d / "sbs.npy"), str(d / "v4k.npy"), L, R, disp


# ---------------------------------------------------------------- the measures discriminate

def test_reprojection_tells_the_matcher_from_disparity_zero_and_from_a_shift(clip3):
    """observed with the oracle: sad / sad0 0.109 - 0.116; the disparity shifted by 2 px (+32) gives 5.7 - 6.0 x the sad and a bad
    share of 0.62 against 0.014 - 0.023.  Every margin below is at least 2 x inside those."""
    L, R, disp = clip3
    for f in range(3):
        r = dict(zip(QR.REPROJ_FIELDS, QR.reproj_frame(L[f], R[f], disp[f], 16).tolist()))
        shifted = np.where(disp[f] >= 1, disp[f] + 32, disp[f]).astype(np.int16)
        s = dict(zip(QR.REPROJ_FIELDS, QR.reproj_frame(L[f], R[f], shifted, 16).tolist()))
        print(f"frame {f}: sad/sad0 {r['sad'] / r['sad0']:.3f}, shifted sad x{s['sad'] / r['sad']:.2f}, bad {r['n_bad'] / r['n_cmp']:.4f} -> {s['n_bad'] / s['n_cmp']:.4f}")
        assert r["n_cmp"] == s["n_cmp"] > 0.7 * W * H
        assert r["sad"] < r["sad0"] / 4
        assert s["sad"] > 3 * r["sad"]
        assert s["n_bad"] > 10 * r["n_bad"]


# ---------------------------------------------------------------- parameters and flags

def test_parameter_checks():
    from video_3d_pipeline.quality import QualityMonitor, check_parameters
    assert check_parameters() == (16, 4, 16, 20)
    assert check_parameters(0, 255, 2047.9375, 256) == (0, 255, 32767, 256) and check_parameters(jump=0.0625)[2] == 1
    for bad in (dict(bad_threshold=-1), dict(bad_threshold=256), dict(bad_threshold=1.5), dict(bad_threshold=True), dict(still=-1), dict(still=256),
                dict(still="4"), dict(jump=-0.5), dict(jump=2048), dict(jump=0.03), dict(jump=float("nan")), dict(jump=float("inf")),
                dict(jump=True), dict(cut_threshold=257), dict(cut_threshold=-1)):
        with pytest.raises(ValueError):
            check_parameters(**bad)
        with pytest.raises(ValueError):
            QualityMonitor(None, **bad)


def test_command_lines_reach_the_constructors(cutclip):
    from video_3d_pipeline import depth as depth_mod, pipeline as pipe_mod
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    sbs, v4k = cutclip[:2]
    for mod, name, argv in ((depth_mod, "HybridStereoDepthExtractor", [sbs]), (pipe_mod, "SbsTo4kDepthPipeline", [sbs, v4k])):
        seen = {}
        orig = getattr(mod, name)

        class Spy(orig):
            def __init__(self, **kw):
                seen.update(kw)
                raise RuntimeError("stop here")

        setattr(mod, name, Spy)
        try:
            assert mod.main(argv) == 1
            assert (seen["quality_report"], seen["quality_bad_threshold"], seen["quality_still"], seen["quality_jump"]) == (None, 16, 4, 1.0)
            seen.clear()
            assert mod.main(argv + ["--quality-report"]) == 1 and seen["quality_report"] is True
            assert mod.main(argv + ["--quality-report", "q.json", "--quality-bad-threshold", "8", "--quality-still", "2", "--quality-jump", "0.5"]) == 1
            assert (seen["quality_report"], seen["quality_bad_threshold"], seen["quality_still"], seen["quality_jump"]) == ("q.json", 8, 2, 0.5)
        finally:
            setattr(mod, name, orig)
    for bad in (dict(quality_bad_threshold=256), dict(quality_still=-1), dict(quality_jump=0.03), dict(quality_report=3)):
        with pytest.raises(ValueError):
            HybridStereoDepthExtractor(work_dir="unused", backend=QualityStereoBackend(), **bad)
    assert depth_mod.main([sbs, "--quality-report", "--quality-still", "300"]) == 1          # refused before anything runs


# ---------------------------------------------------------------- the driver

def _depth_cli(tmp_path, sbs, tag, batch, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=batch, stereo_only=True, unsqueeze_sbs=False,
                                    backend=QualityStereoBackend(), **kw)
    return ex, ex.process_video_sbs(sbs)


def _strip(report):
    return {k: v for k, v in report.items()}


def test_report_equals_the_reference_and_does_not_depend_on_the_pass_size(tmp_path, cutclip, capsys):
    sbs, _, L, R, disp = cutclip
    depth = np.stack([O.disp_to_depth(d) for d in disp])
    want_frames = QR.reproj(L, R, disp, 16)
    want_pairs = QR.flicker(depth, L, 4, 16)
    per_px = want_pairs[:, 0] / (W * H)
    print("luma_sad / (W H) per pair:", np.round(per_px, 1))
    assert per_px[1] > 2 * 20 > 20 > 2 * max(per_px[0], per_px[2])          # observed 41.5 against 7.2 - 7.7, c = 20
    reports = {}
    for batch in (1, 2, 3, 4):
        ex, ddir = _depth_cli(tmp_path, sbs, f"b{batch}", batch, quality_report=True)
        rep = reports[batch] = json.loads((ddir / "quality.json").read_text())
        assert sorted(os.listdir(ddir)) == [f"depth_{i:06d}.png" for i in range(4)] + ["quality.json"]
        assert ex.backend.fetched.count(1) >= (4 - 1) // batch                # the bridging pairs came from carried planes
    assert all(r == reports[1] for r in reports.values())
    rep = reports[1]
    assert set(rep) == {"parameters", "reproj_stage", "flicker_stage", "reproj", "flicker", "width", "height", "units", "frames", "pairs"}
    assert rep["parameters"] == {"bad_threshold": 16, "still": 4, "jump": 1.0, "jump16": 16, "cut_threshold": 20}
    assert (rep["reproj_stage"], rep["flicker_stage"], rep["width"], rep["height"]) == ("matcher", "matcher", W, H)
    assert [[f[k] for k in QR.REPROJ_FIELDS] for f in rep["frames"]] == want_frames.tolist() and [f["frame"] for f in rep["frames"]] == [0, 1, 2, 3]
    assert rep["reproj"]["frames"] == 4 and rep["reproj"]["totals"] == dict(zip(QR.REPROJ_FIELDS, want_frames.sum(axis=0).tolist()))
    tot = want_frames.sum(axis=0)
    assert rep["reproj"]["mean_abs_error"] == tot[2] / tot[1] / 16 and rep["reproj"]["valid_share"] == tot[0] / (4 * W * H)
    assert rep["reproj"]["rms_error_d0"] == (tot[6] / tot[1]) ** 0.5 / 16 and rep["reproj"]["bad_share"] == tot[4] / tot[1]
    m = rep["flicker"]["matched"]
    assert set(rep["flicker"]) == {"matched"} and [[p[k] for k in QR.FLICKER_FIELDS] for p in rep["pairs"]["matched"]] == want_pairs.tolist()
    assert [p["cut"] for p in rep["pairs"]["matched"]] == [False, True, False] and [p["frame"] for p in rep["pairs"]["matched"]] == [1, 2, 3]
    assert (m["pairs"], m["cuts"], m["cut_frames"]) == (3, 1, [2])                # exactly the pair into frame 2, left out of every total
    assert m["totals"] == dict(zip(QR.FLICKER_FIELDS, (want_pairs[0] + want_pairs[2]).tolist()))
    assert m["mean_px_per_frame"] == m["totals"]["flicker"] / m["totals"]["n_still"] / 16
    out = capsys.readouterr().out
    assert "Quality report (4 frames" in out and "1 scene cuts skipped" in out and "disparity 0" in out
    # the report changes no output byte and no cache key
    _, plain = _depth_cli(tmp_path, sbs, "plain", 2)
    assert plain.name == ddir.name and _pngs(plain) == _pngs(ddir) and not (plain / "quality.json").exists()


def test_other_thresholds_path_and_fill_stage(tmp_path, cutclip):
    sbs, _, L, R, disp = cutclip
    filled = np.stack([FR.fill_frame(d) for d in disp])
    path = tmp_path / "elsewhere" / "q.json"
    ex, ddir = _depth_cli(tmp_path, sbs, "fill", 3, quality_report=str(path), quality_bad_threshold=8, quality_still=2, quality_jump=0.5,
                          fill_holes=True, temporal_cut=60)
    rep = json.loads(path.read_text())
    assert not (ddir / "quality.json").exists()
    assert rep["reproj_stage"] == rep["flicker_stage"] == "matcher+fill" and rep["parameters"]["cut_threshold"] == 60
    assert [[f[k] for k in QR.REPROJ_FIELDS] for f in rep["frames"]] == QR.reproj(L, R, filled, 8).tolist()
    assert rep["reproj"]["totals"]["n_valid"] == 4 * W * H and rep["reproj"]["valid_share"] == 1.0
    want = QR.flicker(np.stack([O.disp_to_depth(d) for d in filled]), L, 2, 8)
    assert rep["flicker"]["matched"]["cuts"] == 0 and rep["flicker"]["matched"]["totals"] == dict(zip(QR.FLICKER_FIELDS, want.sum(axis=0).tolist()))
    assert ex.manifest_extra()["quality"] == ex.quality.summary and "frames" not in ex.quality.summary


def test_stabilised_series_under_a_radius(tmp_path, cutclip):
    """--temporal-radius 2 without its fill: a second flicker series over the filtered depth, N - 1 pairs, equal to quality_ref on
    temporal_ref.filter_clip; the populations of the two series are equal, so their sums compare"""
    sbs, _, L, R, disp = cutclip
    depth = np.stack([O.disp_to_depth(d) for d in disp])
    for batch in (1, 3):
        ex, ddir = _depth_cli(tmp_path, sbs, f"r2b{batch}", batch, quality_report=True, temporal_radius=2, temporal_fill=False)
        rep = json.loads((ddir / "quality.json").read_text())
        filt = TR.filter_clip(depth, L, 2, 12, TR.cuts(L, 20), 0)
        want = QR.flicker(filt, L, 4, 16)
        s = rep["flicker"]["stabilised"]
        assert [[p[k] for k in QR.FLICKER_FIELDS] for p in rep["pairs"]["stabilised"]] == want.tolist(), batch
        assert (s["pairs"], s["cuts"]) == (3, 1) and s["totals"] == dict(zip(QR.FLICKER_FIELDS, (want[0] + want[2]).tolist()))
        assert s["totals"]["n_still"] == rep["flicker"]["matched"]["totals"]["n_still"]
        assert rep["flicker"]["matched"]["totals"] == dict(zip(QR.FLICKER_FIELDS, (QR.flicker(depth, L, 4, 16)[[0, 2]].sum(axis=0)).tolist()))
        assert json.loads((ddir / "temporal.json").read_text())["radius"] == 2
    # a backend that does not know the keyword is still called as today when the flag is off
    from test_temporal_host import _depth_cli as plain_cli
    _, pdir = plain_cli(tmp_path, sbs, "r2plain", TemporalStereoBackend(), temporal_radius=2, temporal_fill=False, unsqueeze_sbs=False)
    assert pdir.name == ddir.name and _pngs(pdir) == _pngs(ddir)


def test_sharded_run_reports_no_flicker_and_sums_the_reprojection(tmp_path, cutclip, monkeypatch):
    from video_3d_pipeline import sharding
    from video_3d_pipeline.quality import SHARDED_REASON, QualityMonitor
    sbs, _, L, R, disp = cutclip
    want = QR.reproj(L, R, disp, 16)
    totals = []
    with monkeypatch.context() as mp:
        mp.setattr(sharding, "_initialized", lambda: True)
        mp.setattr(sharding, "barrier", lambda: None)
        mp.setattr(sharding, "total", lambda v: v)
        mp.setenv("WORLD_SIZE", "2")
        for rank in (1, 0):
            mp.setenv("RANK", str(rank))
            ex, ddir = _depth_cli(tmp_path, sbs, "w2", 2, quality_report=str(tmp_path / f"rank{rank}.json"))
            s = ex.quality.summary
            assert s["flicker"] is None and s["flicker_reason"] == SHARDED_REASON
            assert [f[0] for f in ex.quality.frames] == [rank, rank + 2]
            assert s["reproj"]["totals"] == dict(zip(QR.REPROJ_FIELDS, want[rank::2].sum(axis=0).tolist()))
            totals.append(s["reproj"]["totals"])
            assert os.path.exists(tmp_path / f"rank{rank}.json") == (rank == 0)
    assert {k: totals[0][k] + totals[1][k] for k in QR.REPROJ_FIELDS} == dict(zip(QR.REPROJ_FIELDS, want.sum(axis=0).tolist()))
    # finish(total=...) is what sums over the ranks
    be = QualityStereoBackend()
    be._lg, be._rg, be._disp = L, R, disp
    q = QualityMonitor(be, consecutive=False)
    q.note_pass([0, 1, 2, 3], 4, np.zeros((4, H, W), np.float32))
    s = q.finish(total=lambda v: 3 * v)
    assert s["reproj"]["frames"] == 12 and s["reproj"]["totals"]["sad"] == 3 * int(want[:, 2].sum()) and s["flicker"] is None
    assert s["reproj"]["mean_abs_error"] == want[:, 2].sum() / want[:, 1].sum() / 16


def test_pipeline_manifest_and_cached_runs(tmp_path, cutclip, capsys):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    from video_3d_pipeline.quality import CACHED_NOTE
    sbs, v4k, L, R, disp = cutclip

    def pipe(tag, run_kw=None, **kw):
        p = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=3, stereo_only=True, unsqueeze_sbs=False, guide_batch=2,
                                 backend=QualityPipelineBackend(), **kw)
        out = p.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **(run_kw or {}))
        return p, json.loads(open(out).read())
    _, plain = pipe("plain")
    p, man = pipe("q", quality_report=True)
    assert "quality" not in plain and {k: v for k, v in man.items() if k not in ("quality", "frames_dir")} == {k: v for k, v in plain.items() if k != "frames_dir"}
    assert _pngs(man["frames_dir"]) == _pngs(plain["frames_dir"]) and len(_pngs(man["frames_dir"])) == 4
    rep = json.loads(open(os.path.join(man["frames_dir"], "quality.json")).read())
    assert set(man["quality"]) == {"parameters", "reproj_stage", "flicker_stage", "reproj", "flicker"}
    assert man["quality"] == {k: rep[k] for k in man["quality"]}
    assert rep["reproj"]["totals"] == dict(zip(QR.REPROJ_FIELDS, QR.reproj(L, R, disp, 16).sum(axis=0).tolist()))
    p2, man2 = pipe("keep", run_kw=dict(keep_depth_maps=True), quality_report=True)
    cache = p2.extractor.get_cache_path(sbs, 0, 4)
    assert json.loads((cache / "quality.json").read_text()) == rep and not os.path.exists(os.path.join(man2["frames_dir"], "quality.json"))
    # existing output: no report, and a note that says how to get one
    capsys.readouterr()
    before = os.path.getmtime(os.path.join(man["frames_dir"], "quality.json"))
    pipe("q", quality_report=True)
    assert CACHED_NOTE in capsys.readouterr().out and os.path.getmtime(os.path.join(man["frames_dir"], "quality.json")) == before
    ex, ddir = _depth_cli(tmp_path, sbs, "cached", 2)
    ex2, ddir2 = _depth_cli(tmp_path, sbs, "cached", 2, quality_report=True)
    assert ddir2 == ddir and CACHED_NOTE in capsys.readouterr().out and not (ddir / "quality.json").exists() and ex2.quality is None
    pipe("plain")
    assert CACHED_NOTE not in capsys.readouterr().out
