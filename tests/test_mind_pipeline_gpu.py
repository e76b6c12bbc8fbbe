"""--min-disparity through the real HIP backends on a small .npy clip whose scene lies behind the screen: the files of the depth
CLI and the one-pass pipeline equal the C-ABI pieces composed by hand (matcher at the window, rebias, hole filling, depth,
normalisation), quality.json equals tests/quality_ref.py on the cropped arrays, and `auto` chooses what the pure rule gives for
the scores computed by hand."""
import json
import os

import numpy as np
import pytest

import quality_ref as QR
from test_fill_pipeline_gpu import _depth_dir, _pngs

pytestmark = pytest.mark.gpu

SW, SH, NF, BEHIND = 192, 64, 3, 24
M = -32


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """temporal_clip's views with the left one moved BEHIND columns (d = d0 - 24: most of the scene at negative disparity), as a
    full-width side-by-side clip, and a random 4K clip"""
    from video_3d_pipeline import synthetic as syn
    L, R, _ = syn.temporal_clip(SW + BEHIND, SH, NF)
    L, R = L[:, :, BEHIND:], R[:, :, :SW]
    d = tmp_path_factory.mktemp("mindclips")
    np.save(d / "sbs.npy", np.repeat(np.concatenate([L, R], axis=2)[..., None], 3, axis=3))
    np.save(d / "v4k.npy", np.random.default_rng(9).integers(0, 256, (NF, 2 * SH, 2 * SW, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


def _planes(native, sbs, m, unsqueeze=False):
    """the clip through the binding by hand: gray split, a matcher at window m, the rebias, the filled disparity, both depths"""
    from video_3d_pipeline.utils import iter_frames
    dev = native.to_device(np.stack(list(iter_frames(sbs))))
    lg, rg = native.sbs_to_gray_batch(dev, unsqueeze)
    h = native.StereoSGBM(lg.shape[2], lg.shape[1], NF, minDisparity=m)
    rel = h.compute(lg, rg) - 16 * m
    assert h.sync_errors() == 0
    h.close()
    filled = native.fill_holes_disp16_batch(rel.contiguous())
    out = dict(lg=lg, rg=rg, rel=rel, filled=filled, u16=native.depth_to_u16_batch(native.disp_to_depth(rel)),
               u16_filled=native.depth_to_u16_batch(native.disp_to_depth(filled)))
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def planes(native, clips):
    return _planes(native, clips[0], M)


def _cropped(p, key, m, bad=16):
    k = -m
    w = p["lg"].shape[2] - k
    c = lambda a: np.ascontiguousarray(a)
    return QR.reproj(c(p["lg"][:, :, :w]), c(p["rg"][:, :, k:]), c(p[key][:, :, :w]), bad)


def _maps(d):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), f"depth_{i:06d}.png")) for i in range(NF)])


def _depth_cli(tmp_path, tag, sbs, *flags):
    from video_3d_pipeline import depth as depth_mod
    work = str(tmp_path / f"cli_{tag}")
    assert depth_mod.main([sbs, "--work-dir", work, "--stereo-only", "--no-unsqueeze", *flags]) == 0
    return _depth_dir(work)


def _pipeline_cli(tmp_path, tag, sbs, v4k, *flags):
    from video_3d_pipeline import pipeline as pipe_mod
    work, out = str(tmp_path / f"pipe_{tag}"), str(tmp_path / f"pipe_{tag}.json")
    assert pipe_mod.main([sbs, v4k, "--work-dir", work, "--output", out, "--stereo-only", "--no-unsqueeze", "--keep-depth-maps", *flags]) == 0
    return _depth_dir(work), json.loads(open(out).read())


def test_the_window_alone(native, tmp_path, clips, planes):
    sbs, v4k = clips
    rel = planes["rel"]
    assert rel.min() == -16 and rel.max() <= 1023 and (rel[:, :, :64 + M] == -16).all() and (rel[:, :, SW + M:] == -16).all()
    off = _depth_cli(tmp_path, "off", sbs)
    on = _depth_cli(tmp_path, "on", sbs, "--min-disparity", str(M))
    assert os.path.basename(on) != os.path.basename(off)
    assert np.array_equal(_maps(on).view(np.int16), planes["u16"].view(np.int16))
    # the scene is behind the screen and [0, 64) misses it: with the oracle on the CPU 64.8 % of the pixels are valid at -32, 32.5 % at 0
    assert (rel >= 16).mean() > 1.5 * (_planes(native, sbs, 0)["rel"] >= 16).mean()
    assert json.loads(open(os.path.join(on, "min_disparity.json")).read()) == {"min_disparity": M}
    pdir, man = _pipeline_cli(tmp_path, "on", sbs, v4k, "--min-disparity", str(M))
    assert man["min_disparity"] == M and os.path.basename(pdir) == os.path.basename(on) and _pngs(pdir) == _pngs(on)
    _, man_off = _pipeline_cli(tmp_path, "off", sbs, v4k)
    assert "min_disparity" not in man_off and set(man) == set(man_off) | {"min_disparity"}


def test_with_hole_filling_and_the_quality_report(native, tmp_path, clips, planes, capsys):
    sbs, v4k = clips
    on = _depth_cli(tmp_path, "fq", sbs, "--min-disparity", str(M), "--fill-holes", "--quality-report")
    assert np.array_equal(_maps(on).view(np.int16), planes["u16_filled"].view(np.int16))
    rep = json.loads(open(os.path.join(on, "quality.json")).read())
    want = _cropped(planes, "filled", M)
    assert [[f[k] for k in QR.REPROJ_FIELDS] for f in rep["frames"]] == want.tolist() and rep["baseline_disparity"] == M
    assert rep["reproj"]["totals"] == dict(zip(QR.REPROJ_FIELDS, want.sum(axis=0).tolist())) and rep["reproj_stage"] == "matcher+fill"
    assert 0 < rep["reproj"]["totals"]["sad"] < rep["reproj"]["totals"]["sad0"]
    assert "baseline_disparity" in capsys.readouterr().out
    # without the fill the report reads the matcher's own (rebiased) disparity
    q = _depth_cli(tmp_path, "q", sbs, "--min-disparity", str(M), "--quality-report")
    rep_q = json.loads(open(os.path.join(q, "quality.json")).read())
    assert [[f[k] for k in QR.REPROJ_FIELDS] for f in rep_q["frames"]] == _cropped(planes, "rel", M).tolist()
    pdir, man = _pipeline_cli(tmp_path, "fq", sbs, v4k, "--min-disparity", str(M), "--fill-holes", "--quality-report")
    assert _pngs(pdir) == _pngs(on) and json.loads(open(os.path.join(pdir, "quality.json")).read()) == rep
    assert man["min_disparity"] == M and man["fill_holes"] is True and man["quality"]["baseline_disparity"] == M


def test_auto_chooses_what_the_rule_gives_for_the_scores(native, tmp_path, clips, capsys):
    from video_3d_pipeline.depth import MIN_DISPARITY_CANDIDATES, choose_min_disparity
    sbs, v4k = clips
    scores = {}
    for m in MIN_DISPARITY_CANDIDATES:
        rec = _cropped(_planes(native, sbs, m), "rel", m)
        scores[m] = int((rec[:, 1] - rec[:, 4]).sum())
    want = choose_min_disparity(scores)
    print("scores", scores, "->", want)
    assert want != 0
    auto = _depth_cli(tmp_path, "auto", sbs, "--min-disparity", "auto")
    explicit = _depth_cli(tmp_path, "explicit", sbs, "--min-disparity", str(want))
    assert os.path.basename(auto) == os.path.basename(explicit) and _pngs(auto) == _pngs(explicit)
    side = json.loads(open(os.path.join(auto, "min_disparity.json")).read())
    assert side == {"min_disparity": want, "min_disparity_scores": {str(m): s for m, s in scores.items()}}
    assert "--min-disparity auto" in capsys.readouterr().out
    pdir, man = _pipeline_cli(tmp_path, "auto", sbs, v4k, "--min-disparity", "auto")
    assert man["min_disparity"] == want and man["min_disparity_scores"] == side["min_disparity_scores"] and _pngs(pdir) == _pngs(auto)
