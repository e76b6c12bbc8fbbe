"""--match-colour through the real HIP backend: the convert CLI on two frames of a 480 x 270 synthetic clip whose SBS copy (eyes
stored side by side at full width) is graded as in the quality experiment (colour_ref.grade), under a 960 x 540 "4K" release of the
ungraded left view.  One depth run and one upscale serve the three conversions.  Every output equals the NumPy composition
colour_ref histograms -> table -> apply -> stereo_source_ref.render bit for bit; the run without the flag equals the composition
without the colour steps, the parent's bytes."""
import json
import os

import numpy as np
import pytest

import colour_ref as CR
import stereo_pack_ref as P
import stereo_source_ref as X

pytestmark = pytest.mark.gpu

EW, EH, NF = 480, 270, 2


def _zoom2(a):
    from scipy.ndimage import zoom
    return np.clip(np.rint(zoom(a.astype(np.float32), (2, 2, 1), order=1, mode="nearest", grid_mode=True)), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def run(native, tmp_path_factory):
    """-> (convert(tag, *flags) -> manifest, reference(tables or None) -> frames): the clips, the depth run and its upscale, made once"""
    from video_3d_pipeline import convert, depth
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.upscale import SimpleDepthUpscaler
    from video_3d_pipeline.utils import iter_frames, read_png16
    d = tmp_path_factory.mktemp("colourclips")
    pairs = [syn.stereo_pair(EW, EH, i) for i in range(NF)]
    graded = CR.grade(np.stack([np.hstack(p) for p in pairs]))
    v4k_frames = np.stack([_zoom2(p[0]) for p in pairs])
    sbs, v4k = str(d / "sbs.npy"), str(d / "v4k.npy")
    np.save(sbs, graded)
    np.save(v4k, v4k_frames)
    work = str(d / "work")
    assert depth.main([sbs, "--work-dir", work, "--stereo-only", "--no-unsqueeze", "--depth-range", "metric", "--fill-holes"]) == 0
    ddir = [os.path.join(work, x) for x in sorted(os.listdir(work)) if x.startswith("depth_") and os.path.isdir(os.path.join(work, x))]
    up = SimpleDepthUpscaler().process_depth_upscaling(ddir[0], v4k, output_path=str(d / "up.json"))
    depths = [read_png16(os.path.join(json.loads(open(up).read())["frames_dir"], f"depth4k_{i:06d}.png")) for i in range(NF)]

    def conv(tag, *flags):
        out = d / f"3d_{tag}.json"
        assert convert.main([v4k, up, "--output", str(out), "--parallax", "source", "--fill-from-source", sbs, *flags]) == 0
        man = json.loads(out.read_text())
        return man, list(iter_frames(man["frames_dir"]))

    def reference(man, tables):
        from video_3d_pipeline.convert import fill_map_q16
        q = fill_map_q16(None, (EW, EH), (2 * EW, 2 * EH))
        gains = (man["gain_left"], man["gain_right"], man["conv"])
        frames = []
        for i in range(NF):
            s = graded[i] if tables is None else CR.apply(graded[i][None], tables[i], (EW, 0, 2 * EW, EH))[0]
            frames.append(X.render(v4k_frames[i], depths[i], *gains, P.FULL_SBS, False, s, 2, *q))
        return frames
    return conv, reference, graded, v4k_frames


def _same(got, want):
    assert len(got) == len(want) == NF
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"frame {i}: {int((g != w).sum())} bytes differ"


def test_without_the_flag_the_parents_bytes(run):
    conv, reference, _, _ = run
    man, got = conv("off")
    assert not {"match_colour", "colour_probe_frames", "colour_lut"} & set(man)
    _same(got, reference(man, None))


def test_clip_mode(run):
    conv, reference, graded, v4k_frames = run
    man, got = conv("clip", "--match-colour", "clip", "--match-probes", "2")
    assert man["match_colour"] == "clip" and man["colour_probe_frames"] == [0, 1]
    table = CR.lut(CR.hist(graded, (0, 0, EW, EH)), CR.hist(v4k_frames), NF)
    side = json.loads(open(man["colour_lut"]).read())
    assert np.array_equal(np.array(side["lut"], np.uint8), table[0])
    assert (np.diff(table[0].astype(int), axis=1) >= 0).all() and not np.array_equal(table[0], np.arange(256)[None].repeat(3, 0))
    want = reference(man, [table] * NF)
    _same(got, want)
    assert any(not np.array_equal(w, u) for w, u in zip(want, reference(man, None)))           # the match does change the fill


def test_frame_mode(run):
    conv, reference, graded, v4k_frames = run
    man, got = conv("frame", "--match-colour", "frame")
    assert man["match_colour"] == "frame" and "colour_lut" not in man
    tables = [CR.lut(CR.hist(graded[i][None], (0, 0, EW, EH)), CR.hist(v4k_frames[i][None]), 1) for i in range(NF)]
    assert not np.array_equal(tables[0], tables[1])
    _same(got, reference(man, tables))
