"""--quality-report through the real HIP backends on the small synthetic clip of tests/test_fill_pipeline_gpu.py: the flag changes no
output byte of either CLI, the records of quality.json are tests/quality_ref.py on the planes recomputed through the binding
(gray split, matcher, hole filling when on), the stabilised flicker series is quality_ref on tests/temporal_ref.py's filter of the
device depth, and with --fill-holes the reprojection reads the filled disparity."""
import json
import os

import numpy as np
import pytest

import quality_ref as QR
import temporal_ref as TR
from test_fill_pipeline_gpu import NF, SH, SW, _depth_dir, _pngs, clips  # noqa: F401  (clips: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def planes(native, clips):
    """the clip's planes through the binding, computed once: left / right gray, int16 disparity, the filled one, both depths"""
    from video_3d_pipeline.utils import iter_frames
    dev = native.to_device(np.stack(list(iter_frames(clips[0]))))
    lg, rg = native.sbs_to_gray_batch(dev, True)
    m = native.StereoSGBM(SW, SH, NF)
    disp = m.compute(lg, rg)
    assert m.sync_errors() == 0
    m.close()
    filled = native.fill_holes_disp16_batch(disp)
    out = dict(lg=lg, rg=rg, disp=disp, filled=filled, depth=native.disp_to_depth(disp), depth_filled=native.disp_to_depth(filled))
    return {k: v.cpu().numpy() for k, v in out.items()}


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


def _records(items, fields):
    return [[r[k] for k in fields] for r in items]


def test_flag_changes_no_output_and_records_equal_the_reference(native, tmp_path, clips, planes, capsys):
    sbs, v4k = clips
    off = _depth_cli(tmp_path, "off", sbs)
    on = _depth_cli(tmp_path, "on", sbs, "--quality-report")
    assert os.path.basename(on) == os.path.basename(off) and _pngs(on) == _pngs(off) and len(_pngs(on)) == NF
    assert sorted(os.listdir(on)) == sorted(os.listdir(off) + ["quality.json"])
    assert "Quality report (3 frames" in capsys.readouterr().out
    rep = json.loads(open(os.path.join(on, "quality.json")).read())
    want = QR.reproj(planes["lg"], planes["rg"], planes["disp"], 16)
    assert _records(rep["frames"], QR.REPROJ_FIELDS) == want.tolist()
    assert rep["reproj"]["totals"] == dict(zip(QR.REPROJ_FIELDS, want.sum(axis=0).tolist())) and rep["reproj_stage"] == "matcher"
    assert 0 < rep["reproj"]["totals"]["n_cmp"] and rep["reproj"]["totals"]["sad"] < rep["reproj"]["totals"]["sad0"]
    wantf = QR.flicker(planes["depth"], planes["lg"], 4, 16)
    assert _records(rep["pairs"]["matched"], QR.FLICKER_FIELDS) == wantf.tolist() and rep["flicker"]["matched"]["cuts"] == 0
    assert rep["flicker"]["matched"]["totals"] == dict(zip(QR.FLICKER_FIELDS, wantf.sum(axis=0).tolist()))
    # the one-pass pipeline: same depth maps, same 4K maps, the same report next to the kept depth maps and in the manifest
    pdir_off, man_off = _pipeline_cli(tmp_path, "off", sbs, v4k)
    pdir, man = _pipeline_cli(tmp_path, "on", sbs, v4k, "--quality-report")
    assert _pngs(pdir) == _pngs(pdir_off) == _pngs(off) and _pngs(man["frames_dir"]) == _pngs(man_off["frames_dir"])
    assert "quality" not in man_off and json.loads(open(os.path.join(pdir, "quality.json")).read()) == rep
    assert man["quality"] == {k: rep[k] for k in ("parameters", "reproj_stage", "flicker_stage", "reproj", "flicker")}


def test_stabilised_series_equals_the_reference_filter(native, tmp_path, clips, planes):
    sbs, _ = clips
    ddir = _depth_cli(tmp_path, "r2", sbs, "--temporal-radius", "2", "--no-temporal-fill", "--quality-report")
    rep = json.loads(open(os.path.join(ddir, "quality.json")).read())
    filt = TR.filter_clip(planes["depth"], planes["lg"], 2, 12, TR.cuts(planes["lg"], 20), 0)
    want = QR.flicker(filt, planes["lg"], 4, 16)
    assert len(rep["pairs"]["stabilised"]) == NF - 1 and _records(rep["pairs"]["stabilised"], QR.FLICKER_FIELDS) == want.tolist()
    assert rep["flicker"]["stabilised"]["totals"] == dict(zip(QR.FLICKER_FIELDS, want.sum(axis=0).tolist()))
    assert _records(rep["pairs"]["matched"], QR.FLICKER_FIELDS) == QR.flicker(planes["depth"], planes["lg"], 4, 16).tolist()
    assert rep["flicker"]["stabilised"]["totals"]["n_still"] == rep["flicker"]["matched"]["totals"]["n_still"]


def test_fill_holes_is_what_the_reprojection_reads(native, tmp_path, clips, planes):
    sbs, _ = clips
    ddir = _depth_cli(tmp_path, "fill", sbs, "--fill-holes", "--quality-report", "--quality-bad-threshold", "8")
    rep = json.loads(open(os.path.join(ddir, "quality.json")).read())
    assert rep["reproj_stage"] == "matcher+fill" and rep["reproj"]["totals"]["n_valid"] == NF * SW * SH
    assert _records(rep["frames"], QR.REPROJ_FIELDS) == QR.reproj(planes["lg"], planes["rg"], planes["filled"], 8).tolist()
    assert _records(rep["pairs"]["matched"], QR.FLICKER_FIELDS) == QR.flicker(planes["depth_filled"], planes["lg"], 4, 16).tolist()
