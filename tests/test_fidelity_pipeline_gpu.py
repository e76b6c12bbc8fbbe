"""--fidelity-report through the real HIP backends, on the clips of tests/test_source_parallax_pipeline_gpu.py (480 x 270 eyes stored
side by side, a 960 x 540 "4K" release): the depth, upscale and convert CLIs with and without the flag.  The flag changes no output
byte (also with --match-colour clip, --verify-source and the device PNG encoder), the per-frame records are tests/fidelity_ref.py
applied to the contract's render without fill, to the frames as written and to the 4K frame, and the figures mean what they say:
the written eye scores no lower than the warp alone, and a run whose depth is a constant plane scores lower than the matcher's.

Measured on one MI355X (2 frames, cells of 2 x 2; SSIM / PSNR of the clip): warp 0.8453 / 23.11 dB, final 0.9077 / 25.68 dB, ceiling
0.9999 / 63.14 dB; with --match-colour clip --verify-source warp 0.8449 / 23.24 dB, final 0.9859 / 35.15 dB, ceiling 0.9988 / 44.85 dB
(the clips share one grading, so the fitted table only moves the stored left eye away from the frame); with a constant depth plane
warp 0.2288 / 15.92 dB, final 0.2549 / 16.10 dB."""
import json
import os

import numpy as np
import pytest

import colour_ref as CR
import fidelity_ref as F
import stereo_source_ref as X
from test_source_parallax_pipeline_gpu import EH, EW, FLAGS, NF, _three_clis, clips  # noqa: F401

pytestmark = pytest.mark.gpu

Q = (32768, -16384, 32768, -16384)                             # a 480 x 270 eye under a 960 x 540 frame: cells of 2 x 2
W, H = 2 * EW, 2 * EH
BAD = 48
RUNS = {"r": (), "tb": ("--layout", "full-tb"), "cm": ("--match-colour", "clip", "--match-probes", "2", "--verify-source"),
        "png": ("--png-encoder", "gpu")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, clips):
    """one depth and upscale run, then the convert CLI on it: every set of flags without and with --fidelity-report, and one run on
    a constant depth plane"""
    from video_3d_pipeline import convert
    from video_3d_pipeline.utils import iter_frames, write_png16
    tmp = tmp_path_factory.mktemp("fidelity")
    sbs, v4k, _ = clips
    base = ("--parallax", "source", "--fill-from-source", sbs)
    _, up, _ = _three_clis(tmp, "plain", sbs, v4k, FLAGS, base)
    upj = str(tmp / "up_plain.json")
    mans = {}
    for tag, extra in RUNS.items():
        for flag, suffix in (((), "_off"), (("--fidelity-report",), "")):
            assert convert.main([v4k, upj, "--output", str(tmp / f"3d_{tag}{suffix}.json"), *base, *extra, *flag]) == 0
            mans[tag + suffix] = json.loads(open(tmp / f"3d_{tag}{suffix}.json").read())
    flat = tmp / "flat_frames"
    flat.mkdir()
    for i in range(NF):
        write_png16(flat / f"depth4k_{i:06d}.png", np.full((H, W), 1 << 14, np.uint16))
    (tmp / "up_flat.json").write_text(json.dumps(dict(up, frames_dir=str(flat))))
    assert convert.main([v4k, str(tmp / "up_flat.json"), "--output", str(tmp / "3d_flat.json"), *base, "--fidelity-report"]) == 0
    mans["flat"] = json.loads(open(tmp / "3d_flat.json").read())
    reports = {k: json.loads(open(m["fidelity_report"]["path"]).read()) for k, m in mans.items() if "fidelity_report" in m}
    return mans, {k: list(iter_frames(m["frames_dir"])) for k, m in mans.items()}, reports, list(iter_frames(sbs)), list(iter_frames(v4k)), up


def test_the_flag_changes_no_output_byte(native, runs):
    mans, frames, reports, _, _, _ = runs
    for tag in RUNS:
        assert len(frames[tag]) == NF and all(np.array_equal(a, b) for a, b in zip(frames[tag], frames[tag + "_off"])), tag
        a, b = mans[tag], mans[tag + "_off"]
        paths = ("frames_dir", "colour_lut")                    # colour_lut.json lies in the run's own frames directory
        assert {k: v for k, v in a.items() if k not in ("fidelity_report",) + paths} == {k: v for k, v in b.items() if k not in paths}
        if "colour_lut" in a:
            assert json.loads(open(a["colour_lut"]).read()) == json.loads(open(b["colour_lut"]).read())
        assert a["fidelity_report"]["path"] == os.path.join(os.path.dirname(a["frames_dir"]), f"3d_{tag}_fidelity.json")
    assert reports["png"]["frames"] == reports["r"]["frames"]   # the records are read after the encoder's own copy back


def _rows(report, name):
    from video_3d_pipeline.fidelity import FIELDS
    return [[f[name][k] for k in FIELDS] for f in report["frames"]]


def test_the_records_are_the_reference(native, runs):
    from video_3d_pipeline.utils import read_png16
    mans, frames, reports, sbs, v4k, up = runs
    assert F.V.cell(Q[0], Q[2]) == (2, 2)
    man = mans["r"]
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    assert gains[0] == 0
    depth = [read_png16(os.path.join(up["frames_dir"], f"depth4k_{i:06d}.png")) for i in range(NF)]
    for tag, code, right, left in (("r", 0, lambda f: f[:, W:], lambda f: f[:, :W]), ("tb", 2, lambda f: f[H:], lambda f: f[:H])):
        rep = reports[tag]
        assert rep["parameters"]["cell"] == [2, 2] and rep["parameters"]["bad_threshold"] == BAD and (rep["width"], rep["height"]) == (W, H)
        for i in range(NF):
            warp = X.render(v4k[i], depth[i], *gains, code, False, sbs[i], 0, *Q)
            assert np.array_equal(left(frames[tag][i]), v4k[i])
            for name, E, eye in (("warp", right(warp), 1), ("final", right(frames[tag][i]), 1), ("ceiling", v4k[i], 0)):
                want = F.fidelity(np.ascontiguousarray(E), sbs[i], eye, *Q, BAD).tolist()
                assert _rows(rep, name)[i] == want, (tag, name, i)
    # --match-colour clip: every series against the stored eyes in the grading the render saw, the table over both of them
    lut = np.array(json.loads(open(mans["cm"]["colour_lut"]).read())["lut"], np.uint8)
    graded = CR.apply(np.stack(sbs), lut, (0, 0, 2 * EW, EH))
    for i in range(NF):
        warp = X.render(v4k[i], depth[i], *gains, 0, False, graded[i], 0, *Q)
        for name, E, eye in (("warp", warp[:, W:], 1), ("final", frames["cm"][i][:, W:], 1), ("ceiling", v4k[i], 0)):
            assert _rows(reports["cm"], name)[i] == F.fidelity(np.ascontiguousarray(E), graded[i], eye, *Q, BAD).tolist(), (name, i)


def test_the_figures_mean_what_they_say(native, runs):
    """no invented thresholds: the eye as written (with the stored eye's samples in it) scores no lower than the warp alone, and a
    constant depth plane strictly lower than the matcher's depth"""
    mans, _, reports, _, _, _ = runs
    s = {k: r["series"] for k, r in reports.items()}
    for tag in ("r", "tb", "cm", "flat"):
        t = s[tag]
        print(f"{tag}: " + "; ".join(f"{n} SSIM {t[n]['ssim']:.4f} PSNR {t[n]['psnr']} dB mean abs {t[n]['mean_abs']:.3f} bad {t[n]['bad_share']:.4f}"
                                     for n in ("warp", "final", "ceiling")))
        assert t["final"]["ssim"] >= t["warp"]["ssim"] and t["final"]["contains_source_samples"] is True
        assert t["warp"]["frames"] == NF and t["warp"]["totals"]["n_cells"] == NF * EW * EH
        assert t["warp"]["totals"]["n_win"] == NF * ((EW - 8) // 4 + 1) * ((EH - 8) // 4 + 1)
        assert mans[tag]["fidelity_report"]["summary"]["warp"]["ssim"] == t["warp"]["ssim"]
    assert s["tb"]["warp"] == s["r"]["warp"] and s["tb"]["final"] == s["r"]["final"]          # the packing does not reach the eyes
    assert s["flat"]["warp"]["ssim"] < s["r"]["warp"]["ssim"]
    assert s["flat"]["ceiling"] == s["r"]["ceiling"]
