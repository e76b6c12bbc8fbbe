"""Host logic of the frame matching on the CPU: the align CLI's --video-only / --refine-video, guide_start_frame_from, and the
one-pass pipeline's --check-guide.  Stand-ins take the place of the HIP backend, as in the other *_host.py tests: signatures and
scores from the NumPy restatement (tests/framematch_ref.py) for the refinement, planted scores for the guide check."""
import json

import numpy as np
import pytest

import framematch_ref as FR
from test_pipeline_host import OraclePipelineBackend, SH, SW, _pngs

TEN = ("video1_path", "video2_path", "time_offset_seconds", "offset_frames", "correlation_strength", "frame_duration", "video1_fps",
       "video2_fps", "sample_rate", "audio_length_analyzed")
NEW = ("guide_start_frame_audio", "guide_start_frame", "visual_status", "visual_shift_frames", "visual_score", "visual_margin",
       "visual_probe_shifts", "visual_probe_scores", "visual_parameters")


class RefMatchBackend:
    """test-only stand-in for the refinement's backend: the left eye of an SBS frame is its left half (gray in all channels)"""

    def sbs_left_signatures(self, frames, unsqueeze):
        assert not unsqueeze
        return FR.signature(np.stack([f[:, :f.shape[1] // 2, 0] for f in frames]))

    def guide_signatures(self, frames, height, width):
        assert all(f.shape[:2] == (height, width) for f in frames)
        return FR.signature(np.stack([f[..., 0] for f in frames]))

    def signature_scores(self, a, b):
        return FR.scores(a, b)

    def read_scores(self, handle):
        return handle


def _save(path, frames, fps=None):
    bgr = np.repeat(frames[..., None], 3, axis=3)
    if fps is None:
        np.save(path, bgr)
    else:
        np.savez(path, frames=bgr, fps=fps)
    return str(path)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("fm")
    left, guide = FR.match_clips(128, 72, 24, speed=6, delay=3)
    static = np.repeat(left[:1], 24, axis=0)
    return dict(dir=d, sbs=_save(d / "sbs.npy", np.concatenate([left, left], axis=2)), guide=_save(d / "guide.npy", guide),
                static=_save(d / "static.npy", np.concatenate([static, static], axis=2)),
                static_guide=_save(d / "static_guide.npy", np.repeat(guide[:1], 31, axis=0)),
                guide25=_save(d / "guide25.npz", guide, fps=25.0))


ARGS = ["--no-unsqueeze", "--refine-window", "12", "--refine-min-score", "0.5", "--refine-min-margin", "0.01"]


def _run(clips, tmp_path, sbs, guide, *extra):
    from video_3d_pipeline import align
    rc = align.main([clips[sbs], clips[guide], "--work-dir", str(tmp_path), *ARGS, *extra], backend=RefMatchBackend())
    f = tmp_path / "alignment_data.json"
    return rc, (json.loads(f.read_text()) if f.exists() else None), str(f)


def test_video_only_writes_the_new_keys_and_nulls(clips, tmp_path, capsys):
    from video_3d_pipeline.align import guide_start_frame_from
    rc, data, path = _run(clips, tmp_path, "sbs", "guide", "--video-only")
    assert rc == 0 and list(data)[:10] == list(TEN) and all(k in data for k in NEW)
    assert [data[k] for k in ("time_offset_seconds", "offset_frames", "correlation_strength", "sample_rate", "audio_length_analyzed")] == [None] * 5
    assert data["video1_path"] == clips["sbs"] and data["video1_fps"] == data["video2_fps"] == 23.976
    assert (data["visual_status"], data["visual_shift_frames"], data["guide_start_frame"], data["guide_start_frame_audio"]) == ("refined", 3, 3, None)
    assert data["visual_probe_shifts"] == [3, 3, 3] and data["visual_score"] > 0.9 and data["visual_margin"] > 0.01
    assert data["visual_parameters"]["window"] == 12 and data["visual_parameters"]["search"] == 4
    assert guide_start_frame_from(path, clips["guide"]) == 3
    assert "refined" in capsys.readouterr().out
    # a seed of its own: the shift is relative to it
    rc, data, _ = _run(clips, tmp_path, "sbs", "guide", "--video-only", "--guide-start-frame", "5")
    assert rc == 0 and (data["visual_shift_frames"], data["guide_start_frame"]) == (-2, 3)


def _fake_find(offset, fps=23.976):
    def find_alignment(self, max_audio_length=300):
        return {"video1_path": self.video1_path, "video2_path": self.video2_path, "time_offset_seconds": offset,
                "offset_frames": offset * fps, "correlation_strength": 0.9, "frame_duration": 1 / fps, "video1_fps": fps,
                "video2_fps": fps, "sample_rate": 22050, "audio_length_analyzed": float(max_audio_length)}
    return find_alignment


def test_refine_video_keeps_the_ten_keys_and_moves_the_start_frame(clips, tmp_path, monkeypatch):
    from video_3d_pipeline import align
    monkeypatch.setattr(align.VideoAligner, "find_alignment", _fake_find(2 / 23.976))          # the audio says 2 frames
    want = _fake_find(2 / 23.976)(align.VideoAligner(clips["sbs"], clips["guide"]))
    rc, data, path = _run(clips, tmp_path, "sbs", "guide", "--refine-video")
    assert rc == 0 and {k: data[k] for k in TEN} == want
    assert (data["guide_start_frame_audio"], data["visual_shift_frames"], data["guide_start_frame"], data["visual_status"]) == (2, 1, 3, "refined")
    assert align.guide_start_frame_from(path, clips["guide"]) == 3
    # without --refine-video nothing is added and guide_start_frame_from rounds the offset as before
    json.dump(want, open(path, "w"))
    assert align.guide_start_frame_from(path, clips["guide"]) == 2
    # a negative audio offset is refused with the advice of guide_start_frame_from
    monkeypatch.setattr(align.VideoAligner, "find_alignment", _fake_find(-1.0))
    rc, _, _ = _run(clips, tmp_path / "neg", "sbs", "guide", "--refine-video")
    assert rc == 1


def test_negative_offset_refusal_is_unchanged_and_advice_matches(clips, tmp_path, capsys, monkeypatch):
    from video_3d_pipeline import align
    f = tmp_path / "neg.json"
    f.write_text(json.dumps({"video1_path": "s", "video2_path": "k", "time_offset_seconds": -0.5, "video1_fps": 24.0}))
    with pytest.raises(ValueError, match=r"--start-frame 12 and pass --guide-start-frame 0"):
        align.guide_start_frame_from(str(f), clips["guide"])
    f.write_text(json.dumps({"time_offset_seconds": None, "guide_start_frame": -4}))
    with pytest.raises(ValueError, match=r"--start-frame 4 and pass --guide-start-frame 0"):
        align.guide_start_frame_from(str(f), clips["guide"])
    monkeypatch.setattr(align.VideoAligner, "find_alignment", _fake_find(-0.5, 24.0))
    assert align.main([clips["sbs"], clips["guide"], "--work-dir", str(tmp_path), "--refine-video"], backend=RefMatchBackend()) == 1
    assert "--start-frame 12 and pass --guide-start-frame 0" in capsys.readouterr().out


def test_undetermined_and_inconsistent_keep_the_seed(clips, tmp_path, capsys):
    from video_3d_pipeline import framematch as FM
    rc, data, _ = _run(clips, tmp_path, "static", "static_guide", "--video-only", "--guide-start-frame", "4")
    assert rc == 0 and (data["visual_status"], data["visual_shift_frames"], data["guide_start_frame"]) == ("undetermined", 0, 4)
    assert "the seed is kept" in capsys.readouterr().out
    # probes that disagree: the second half of the guide clip is cut one frame shorter
    bgr = np.load(clips["guide"])
    cut = np.concatenate([bgr[:14], bgr[15:]])
    np.save(tmp_path / "cut.npy", cut)
    res = FM.refine(clips["sbs"], str(tmp_path / "cut.npy"), 3, search=4, window=8, probes=2, unsqueeze=False, min_score=0.5,
                    min_margin=0.01, backend=RefMatchBackend())
    assert res["probe_shifts"] == [0, -1] and (res["status"], res["shift"], res["guide_start_frame"]) == ("inconsistent", 0, 3)


def test_unequal_fps_is_refused(clips, tmp_path, capsys):
    from video_3d_pipeline import framematch as FM
    with pytest.raises(ValueError, match="frame rates differ"):
        FM.refine(clips["sbs"], clips["guide25"], 0, backend=RefMatchBackend())
    rc, data, _ = _run(clips, tmp_path, "sbs", "guide25", "--video-only")
    assert rc == 1 and data is None and "frame rates differ" in capsys.readouterr().out


# ---------------------------------------------------------------- --check-guide
class PlantedCheckBackend(OraclePipelineBackend):
    """stand-in with planted scores: a "signature" is the frame's clip index (left) or its position in the 4K clip (guide, read
    from the frame's first pixel), and Z(i, g) = peak where g - i == self.true_shift, else 0.2"""

    def __init__(self, true_shift=0, peak=0.9):
        super().__init__()
        self.true_shift, self.peak, self.noted = true_shift, peak, []

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None):
        self._n = len(frames)
        return super().sbs_to_disparity(frames, unsqueeze, mono_provider)

    def left_gray(self, n):
        assert n == self._n
        return np.zeros((n, 1, 1), np.uint8)

    def frame_signatures(self, gray):
        k = len(self.noted)
        self.noted += list(range(k, k + len(gray)))
        return list(range(k, k + len(gray)))                      # frames arrive in clip order: the clip index

    def guide_luma(self, frames, height, width, capacity):
        self._tags = [None if f is None else int(f[0, 0, 0]) for f in frames]
        return super().guide_luma(frames, height, width, capacity)

    def guide_scores(self, rows, luma):
        z = np.array([[np.nan if g is None else (self.peak if g - i == self.true_shift else 0.2) for g in self._tags] for i in rows])
        scale = 1 << 20
        return np.nan_to_num(z * scale).astype(np.int64), np.full(len(rows), scale, np.int64), \
            np.array([0 if g is None else scale for g in self._tags], np.int64)

    def read_scores(self, handle):
        return handle


@pytest.fixture()
def tagged(tmp_path):
    from video_3d_pipeline import synthetic as syn
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(10)])
    guides = np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(10)])
    guides[:, 0, 0, :] = np.arange(10)[:, None]                   # the 4K frame's own index in its first pixel
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", guides)
    return str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy")


def _pipe(tmp_path, tagged, tag, backend, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"w_{tag}"), batch_size=5, stereo_only=True, guide_batch=5, backend=backend, **kw)
    out = pipe.run(tagged[0], tagged[1], output_path=str(tmp_path / f"{tag}.json"))
    man = json.loads(open(out).read())
    return man, _pngs(man["frames_dir"])


def test_check_guide_manifest_and_warning(tmp_path, tagged, capsys):
    plain, want = _pipe(tmp_path, tagged, "plain", OraclePipelineBackend())
    assert "guide_match" not in plain
    capsys.readouterr()
    man, got = _pipe(tmp_path, tagged, "ok", PlantedCheckBackend(0), check_guide=True, check_guide_min=0.5)
    out = capsys.readouterr().out
    assert got == want                                             # no output PNG changes by a byte
    gm = man["guide_match"]
    assert set(gm) >= {"frames_checked", "frames_below", "skipped", "median", "min", "worst_frame", "suspected_shift"}
    assert (gm["frames_checked"], gm["frames_below"], gm["skipped"], gm["suspected_shift"]) == (10, 0, 0, 0)
    assert abs(gm["median"] - 0.9) < 1e-6 and "Guide check: 10 frames checked" in out and "Warning" not in out
    # the guide is one frame late: every pair scores 0.2, the in-batch search finds +1 in both batches -> warning
    man, got = _pipe(tmp_path, tagged, "late", PlantedCheckBackend(1), check_guide=True, check_guide_min=0.5)
    out = capsys.readouterr().out
    gm = man["guide_match"]
    assert got == want and (gm["frames_checked"], gm["frames_below"], gm["suspected_shift"], gm["worst_frame"]) == (10, 10, 1, 0)
    assert "Warning" in out and "python -m video_3d_pipeline.align --refine-video" in out
    # a low peak alone (median below the threshold, shift 0) warns too; a threshold below it does not
    _pipe(tmp_path, tagged, "low", PlantedCheckBackend(0, peak=0.4), check_guide=True, check_guide_min=0.5)
    assert "--refine-video" in capsys.readouterr().out
    _pipe(tmp_path, tagged, "low2", PlantedCheckBackend(0, peak=0.4), check_guide=True, check_guide_min=0.3)
    assert "Warning" not in capsys.readouterr().out


def test_check_guide_skips_flat_guides(tmp_path, tagged, capsys):
    short = np.load(tagged[1])[:7]
    np.save(tmp_path / "short.npy", short)
    man, _ = _pipe(tmp_path, (tagged[0], str(tmp_path / "short.npy")), "short", PlantedCheckBackend(0), check_guide=True)
    gm = man["guide_match"]
    assert (gm["frames_checked"], gm["skipped"], gm["frames_below"], gm["suspected_shift"]) == (7, 3, 0, 0)
