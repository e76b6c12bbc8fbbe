"""Frame matching end to end on the device: a 320 x 180 temporal SBS clip and its 640 x 360 guide clip delayed by 3 frames, as
.npy stacks.  `align --video-only` must find the delay, the pipeline's --check-guide must confirm the aligned pairing and flag
the unaligned one, and the flag must not change an output byte.  The restatement (tests/framematch_ref.py) gives these clips, on
the CPU, shift +3 for the refinement (M = 0.998, margin 0.095) and, at guide start 0, an in-batch winner of +2 in every batch of
8 (the search is capped at +-2) with per-pair scores around 0.88."""
import json
import os

import numpy as np
import pytest

import framematch_ref as FR

pytestmark = pytest.mark.gpu
N = 30


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("fmpipe")
    sbs, guide = FR.match_sbs_clips(320, 180, N, delay=3)
    np.save(d / "sbs.npy", sbs)
    np.save(d / "g4k.npy", guide)
    return d, str(d / "sbs.npy"), str(d / "g4k.npy")


def _pipeline(d, sbs, g4k, tag, *extra):
    from video_3d_pipeline import pipeline
    out = d / f"{tag}.json"
    rc = pipeline.main([sbs, g4k, "--output", str(out), "--work-dir", str(d / f"w_{tag}"), "--stereo-only", *extra])
    assert rc == 0
    man = json.loads(out.read_text())
    return man, {f: open(os.path.join(man["frames_dir"], f), "rb").read() for f in sorted(os.listdir(man["frames_dir"]))}


def test_align_finds_the_delay_and_check_guide_confirms_it(native, clips, capsys):
    from video_3d_pipeline import align
    d, sbs, g4k = clips
    assert align.main([sbs, g4k, "--video-only", "--work-dir", str(d / "al"), "--refine-min-score", "0.5", "--refine-min-margin", "0.01"]) == 0
    data = json.loads((d / "al" / "alignment_data.json").read_text())
    print(f"align --video-only: {data['visual_status']} shift {data['visual_shift_frames']} score {data['visual_score']:.4f} "
          f"margin {data['visual_margin']:.4f}")
    assert (data["visual_status"], data["visual_shift_frames"], data["guide_start_frame"]) == ("refined", 3, 3)
    capsys.readouterr()
    man, _ = _pipeline(d, sbs, g4k, "aligned", "--alignment-file", str(d / "al" / "alignment_data.json"), "--check-guide")
    out = capsys.readouterr().out
    gm = man["guide_match"]
    print(gm)
    assert (gm["suspected_shift"], gm["frames_below"], gm["frames_checked"], gm["skipped"]) == (0, 0, N, 0)
    assert "Guide check:" in out and "--refine-video" not in out


def test_check_guide_flags_the_unaligned_run_and_changes_no_byte(native, clips, capsys):
    d, sbs, g4k = clips
    man, got = _pipeline(d, sbs, g4k, "off", "--guide-start-frame", "0", "--check-guide")
    out = capsys.readouterr().out
    gm = man["guide_match"]
    print(gm)
    assert gm["suspected_shift"] == 2 and gm["frames_checked"] == N          # the in-batch search is capped at +-2
    assert "Warning" in out and "python -m video_3d_pipeline.align --refine-video" in out
    plain, want = _pipeline(d, sbs, g4k, "plain", "--guide-start-frame", "0")
    assert "guide_match" not in plain and len(want) == N and got == want
