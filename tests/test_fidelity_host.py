"""Host logic of --fidelity-report on the CPU: the flag's dependencies and their messages, the summary's arithmetic, the schema of
fidelity.json and of the manifest entry, the convert step over a NumPy stand-in backend (tests/stereo_source_ref.py +
tests/fidelity_ref.py in place of the HIP entries), HipRenderBackend's own sequence of calls over stand-ins for torch's device
side and for the native module (the extra render goes to scratch; histograms, table, then the table over the whole SBS frame), that
there is no cache suffix and nothing changes without the flag, and the null summary of a sharded run."""
import contextlib
import json
import math
import types
from pathlib import Path

import numpy as np
import pytest

import colour_ref as CR
import fidelity_ref as F
import stereo_pack_ref as P
import stereo_source_ref as X
import verify_ref as V
from test_convert_host import H4, W4, _pngs, _read_clip, sbs_clips  # noqa: F401
from test_pipeline_host import SH, SW
from test_source_parallax_host import SourceRenderBackend, _PackPipelineBackend, _convert, _pipeline

BAD = 48


def _eyes(out, layout, W, H):
    return (out[:, :, :W], out[:, :, W:]) if layout == P.FULL_SBS else (out[:, :H], out[:, H:])


class FidelityRenderBackend(SourceRenderBackend):
    """the source-fill stand-in plus the measurements of convert.HipRenderBackend through tests/fidelity_ref.py"""

    def __init__(self):
        super().__init__()
        self.requests, self.asked, self._handle, self.scratch = [], 0, None, []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        fid = None if source is None else source.get("fidelity")
        self.requests.append(fid)
        out = super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)
        self._handle = None
        if fid is not None:
            assert layout in (P.FULL_SBS, P.FULL_TB)
            H, W = depths[0].shape
            sbs = np.stack(source["frames"])
            warp = np.stack([X.render(f, d, gain_left, gain_right, conv, layout, subpixel, s, 0, *source["q"])
                             for f, d, s in zip(frames, depths, sbs)])
            self.scratch.append(warp)
            recs = [F.fidelity_batch(np.ascontiguousarray(_eyes(warp, layout, W, H)[1]), sbs, 1, *source["q"], fid["bad_thr"]),
                    F.fidelity_batch(np.ascontiguousarray(_eyes(out, layout, W, H)[1]), sbs, 1, *source["q"], fid["bad_thr"])]
            if fid["ceiling"]:
                recs.append(F.fidelity_batch(np.ascontiguousarray(_eyes(out, layout, W, H)[0]), sbs, 0, *source["q"], fid["bad_thr"]))
            self._handle = recs
        return out

    def fidelity_handle(self):
        self.asked += 1
        handle, self._handle = self._handle, None
        return handle

    def read_fidelity(self, handle, wait=True):
        return handle


@pytest.fixture()
def run(sbs_clips):
    tmp, sbs, v4k, _ = sbs_clips
    _pipeline(tmp, sbs, v4k, "f", _PackPipelineBackend(), ctor=dict(depth_range="metric", fill_holes=True))
    return tmp, sbs, v4k, [v4k, tmp / "depth_f.json", "--parallax", "source", "--fill-from-source", sbs]


def _q():
    from video_3d_pipeline.register import map_to_q16
    return map_to_q16(1, 0, SW // 2, W4) + map_to_q16(1, 0, SH, H4)


def test_plan_and_cli_refusals(run, capsys):
    from video_3d_pipeline import fidelity
    from video_3d_pipeline.convert import VERIFY_LAYOUTS, DepthTo3DConverter, StereoPlan
    assert fidelity.LAYOUTS == VERIFY_LAYOUTS and fidelity.FIELDS == ("n_cells", "sad", "ssd", "n_bad", "n_win", "ssim_q20")
    assert fidelity.BAD_MAX == F.BAD_MAX and fidelity.SSIM_ONE == F.ONE and len(fidelity.FIELDS) == F.FIELDS
    with pytest.raises(ValueError, match="--fill-from-source"):
        StereoPlan(fidelity_report=True)
    assert StereoPlan(parallax="source", fidelity_report=True).fidelity_report is True
    for layout in ("half-sbs", "half-tb", "interlaced", "anaglyph-colour", "anaglyph-dubois"):
        with pytest.raises(ValueError, match="full-sbs, full-tb"):
            StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, fidelity_report=True)
    for layout in ("full-sbs", "full-tb"):
        assert StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, fidelity_report="r.json").fidelity_report == "r.json"
    assert StereoPlan(parallax="source", fill_from_source="s.npy").fidelity_report is None
    for bad in (-1, 766, 1.5, True, "48"):
        with pytest.raises(ValueError, match="bad threshold"):
            fidelity.check_parameters(bad)
    be = FidelityRenderBackend()
    with pytest.raises(ValueError, match="--fill-from-source"):  # a run over clips without the SBS clip
        DepthTo3DConverter(backend=be, parallax="source", fidelity_report=True).process_conversion(
            run[2], str(run[0] / "depth_f.json"), output_path=str(run[0] / "o.json"))
    assert not be.calls
    tmp, sbs, v4k, base = run
    out = ["--output", tmp / "o.json"]
    for args, word in (([v4k, tmp / "depth_f.json", "--parallax", "source", "--fidelity-report"], "--fidelity-report needs --fill-from-source"),
                       ([v4k, tmp / "depth_f.json", "--fidelity-report", tmp / "r.json"], "--fill-from-source"),
                       (base + ["--fidelity-report", "--layout", "half-sbs"], "--fidelity-report works on the layouts full-sbs, full-tb"),
                       (base + ["--layout", "anaglyph-dubois", "--fidelity-report"], "squeezes, interleaves or mixes it")):
        be = FidelityRenderBackend()
        assert _convert(args + out, be) == 1 and not be.calls, args
        assert word in capsys.readouterr().out, args
    assert not (tmp / "o.json").exists()


def test_summary_arithmetic():
    from video_3d_pipeline import fidelity as M
    one = M.SSIM_ONE
    rec = {"warp": [(0, np.array([100, 300, 1200, 5, 4, 3 * one], np.int64)), (1, np.array([100, 0, 0, 0, 4, 4 * one], np.int64))],
           "final": [(1, np.array([100, 0, 0, 0, 0, 0], np.int64))], "ceiling": None}
    s = M.summary(rec)
    w = s["series"]["warp"]
    assert w["frames"] == 2 and w["totals"] == dict(n_cells=200, sad=300, ssd=1200, n_bad=5, n_win=8, ssim_q20=7 * one)
    assert w["mean_abs"] == 300 / 600 and w["bad_share"] == 5 / 200 and w["ssim"] == 7 / 8
    assert w["psnr"] == pytest.approx(10 * math.log10(65025 / 2.0))
    assert [f["frame"] for f in w["worst_frames"]] == [0, 1] and w["worst_frames"][0]["ssim"] == 0.75 and w["worst_frames"][1]["psnr"] == math.inf
    f = s["series"]["final"]
    assert f["ssim"] is None and f["psnr"] == math.inf and f["mean_abs"] == 0 and f["worst_frames"] == [] and f["contains_source_samples"] is True
    assert s["series"]["ceiling"] is None and "contains_source_samples" not in w
    assert s["frames"][0] == {"frame": 0, "warp": dict(n_cells=100, sad=300, ssd=1200, n_bad=5, n_win=4, ssim_q20=3 * one, mean_abs=1.0,
                                                       psnr=pytest.approx(10 * math.log10(65025 / 4.0)), bad_share=0.05, ssim=0.75)}
    assert sorted(s["frames"][1]) == ["final", "frame", "warp"] and s["frames"][1]["final"]["ssim"] is None
    assert M.figures(dict.fromkeys(M.FIELDS, 0)) == dict(mean_abs=None, psnr=None, bad_share=None, ssim=None)
    # the ten worst frames by SSIM, ties by frame
    many = [(i, np.array([10, 1, 1, 0, 2, (2 * one * (i % 7)) // 7], np.int64)) for i in range(25)]
    worst = M.series_summary(many)["worst_frames"]
    assert [f["frame"] for f in worst] == [0, 7, 14, 21, 1, 8, 15, 22, 2, 9]
    assert json.loads(json.dumps(M._jsonable(s)))["series"]["final"]["psnr"] == "inf"


@pytest.mark.parametrize("layout", ["full-sbs", "full-tb"])
def test_cli_records_report_and_manifest(run, capsys, layout):
    tmp, sbs, v4k, base = run
    q, code = _q(), P.FULL_SBS if layout == "full-sbs" else P.FULL_TB
    plain = SourceRenderBackend()                              # predates the report: no fidelity_handle at all
    assert _convert(base + ["--layout", layout, "--output", tmp / "plain.json"], plain) == 0
    capsys.readouterr()
    be = FidelityRenderBackend()
    assert _convert(base + ["--layout", layout, "--fidelity-report", "--output", tmp / "r.json"], be) == 0
    text = capsys.readouterr().out
    a, b = json.loads((tmp / "plain.json").read_text()), json.loads((tmp / "r.json").read_text())
    assert be.requests == [{"bad_thr": BAD, "ceiling": True}] * 2 and be.asked == 2 and be.calls == plain.calls == [(4, 2, q), (1, 2, q)]
    assert _pngs(a["frames_dir"]) == _pngs(b["frames_dir"])
    assert {k: v for k, v in b.items() if k not in ("fidelity_report", "frames_dir")} == {k: v for k, v in a.items() if k != "frames_dir"}
    entry = b["fidelity_report"]
    assert entry["path"] == str(tmp / "r_fidelity.json") and sorted(entry) == ["height", "parameters", "path", "summary", "width"]
    data = json.loads((tmp / "r_fidelity.json").read_text())
    assert sorted(data) == ["frames", "height", "parameters", "series", "units", "width"]
    cx, cy = V.cell(q[0], q[2])
    assert data["parameters"]["bad_threshold"] == BAD and data["parameters"]["cell"] == [cx, cy] and (data["width"], data["height"]) == (W4, H4)
    # the records are the reference applied to the frames as written, to the render without fill and to the 4K frame
    got, frames4k, sbs_frames = _read_clip(b["frames_dir"]), _read_clip(v4k), _read_clip(sbs)
    gains = (b["gain_left"], b["gain_right"], b["conv"])
    assert gains[0] == 0 and len(data["frames"]) == 5 and [f["frame"] for f in data["frames"]] == list(range(5))
    from video_3d_pipeline.utils import read_png16
    dman = json.loads((tmp / "depth_f.json").read_text())
    from video_3d_pipeline import fidelity as M
    tot = {k: np.zeros(6, np.int64) for k in M.SERIES}
    for i, row in enumerate(data["frames"]):
        d = read_png16(f"{dman['frames_dir']}/depth4k_{i:06d}.png")
        EL, ER = (e[0] for e in _eyes(got[i][None], code, W4, H4))
        warp = _eyes(X.render(frames4k[i], d, *gains, code, False, sbs_frames[i], 0, *q)[None], code, W4, H4)[1][0]
        assert np.array_equal(EL, frames4k[i])
        for name, E, eye in (("warp", warp, 1), ("final", ER, 1), ("ceiling", EL, 0)):
            want = F.fidelity(np.ascontiguousarray(E), sbs_frames[i], eye, *q, BAD)
            assert [row[name][k] for k in M.FIELDS] == want.tolist(), (i, name)
            tot[name] += want
    for name in M.SERIES:
        s = data["series"][name]
        t = dict(zip(M.FIELDS, tot[name].tolist()))
        assert s["totals"] == t and s["frames"] == 5
        for k, v in M._jsonable(M.figures(t)).items():
            assert s[k] == v and entry["summary"][name][k] == v
        assert "worst_frames" in s and "worst_frames" not in entry["summary"][name]
    assert data["series"]["final"]["contains_source_samples"] is True and entry["summary"]["final"]["contains_source_samples"] is True
    assert text.count("Fidelity report (5 frames") == 1 and "  warp (" in text and "  final (" in text and "  ceiling (" in text
    # the scratch renders are not the output: where a hole was filled they differ from the written frames
    assert len(be.scratch) == 2 and any((w != g).any() for w, g in zip(np.concatenate(be.scratch), got))
    # the existing output is used: no report is made, and the run says so
    be = FidelityRenderBackend()
    assert _convert(base + ["--layout", layout, "--fidelity-report", "--output", tmp / "r.json"], be) == 0 and not be.calls
    assert "Fidelity report: none was made" in capsys.readouterr().out
    # a path of its own
    assert _convert(base + ["--layout", layout, "--fidelity-report", tmp / "sub" / "mine.json", "--output", tmp / "p.json"], FidelityRenderBackend()) == 0
    assert json.loads((tmp / "sub" / "mine.json").read_text()) == data
    assert json.loads((tmp / "p.json").read_text())["fidelity_report"]["path"] == str(tmp / "sub" / "mine.json")


def test_a_rendered_left_eye_has_no_ceiling(run, capsys):
    """left gain != 0 cannot come from --parallax source today; the monitor is told so directly"""
    from video_3d_pipeline.fidelity import CEILING_REASON, FidelityMonitor
    be = FidelityRenderBackend()
    m = FidelityMonitor(ceiling=False)
    assert m.request() == {"bad_thr": BAD, "ceiling": False}
    be._handle = [np.array([[64, 1, 1, 0, 1, 1 << 19]], np.int64), np.array([[64, 0, 0, 0, 1, 1 << 20]], np.int64)]
    m.note(be, [3], (16, 16), (32768, 0, 32768, 0))
    entry = m.finish(Path("x.json"), None, 1)[0]["fidelity_report"]
    assert entry["summary"]["ceiling"] is None and entry["ceiling_reason"] == CEILING_REASON and m.data["series"]["ceiling"] is None
    assert m.data["frames"] == [{"frame": 3, "warp": dict(n_cells=64, sad=1, ssd=1, n_bad=0, n_win=1, ssim_q20=1 << 19, mean_abs=1 / 192,
                                                          psnr=pytest.approx(10 * math.log10(65025 * 192)), bad_share=0.0, ssim=0.5),
                                 "final": dict(n_cells=64, sad=0, ssd=0, n_bad=0, n_win=1, ssim_q20=1 << 20, mean_abs=0.0, psnr=math.inf,
                                               bad_share=0.0, ssim=1.0)}]
    m.report()
    assert "ceiling: not measured" in capsys.readouterr().out
    with pytest.raises(RuntimeError, match="without measuring"):
        m.note(be, [4], (16, 16), (32768, 0, 32768, 0))


def test_no_cache_suffix_and_nothing_changes_without_the_flag(run, monkeypatch):
    tmp, sbs, v4k, base = run
    monkeypatch.chdir(tmp)
    assert _convert(base + ["--fidelity-report"], FidelityRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_depth_f.mp4").exists() or (tmp / "3d_full-sbs_srcpx_srcfill_depth_f_frames").is_dir()
    be = FidelityRenderBackend()
    assert _convert(base + ["--output", tmp / "new.json"], be) == 0
    assert be.requests == [None, None] and be.asked == 0
    assert "fidelity_report" not in json.loads((tmp / "new.json").read_text())
    from video_3d_pipeline.convert import StereoPlan
    plan = StereoPlan(parallax="source", fill_from_source=sbs)
    assert "fidelity" not in plan.source_kwargs([np.zeros((SH, SW, 3), np.uint8)], (W4, H4))["source"]


def test_a_sharded_run_has_a_null_summary(capsys):
    from video_3d_pipeline.fidelity import SHARDED_REASON, FidelityMonitor
    be = FidelityRenderBackend()
    m = FidelityMonitor()
    be._handle = [np.zeros((1, 6), np.int64)] * 3
    m.note(be, [0], (16, 16), (32768, 0, 32768, 0))
    assert m.finish(Path("x.json"), None, 2) == ({"fidelity_report": {"path": None, "summary": None, "reason": SHARDED_REASON}}, {}) and m.data is None
    m.report()
    assert "not made" in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------------------------------
# HipRenderBackend's own sequence, over stand-ins for torch's device side and the native module
# ------------------------------------------------------------------------------------------------------------------------
def _host_backend(log):
    import torch
    from video_3d_pipeline.convert import HipRenderBackend

    class HostTorch:
        uint8, int16, int32, int64, Tensor = torch.uint8, torch.int16, torch.int32, torch.int64, torch.Tensor
        from_numpy = staticmethod(torch.from_numpy)

        @staticmethod
        def empty(*a, pin_memory=False, device=None, **k):
            return torch.zeros(*a, **k)

        class cuda:
            device = staticmethod(lambda d: contextlib.nullcontext())

    def name_of(t, be):
        for k, v in be._bufs.items():
            if v.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
                return k
        return "?"

    class RefNative:
        FIDELITY_FIELDS = 6
        stereo_output_size = staticmethod(P.output_size)

        @staticmethod
        def bgr_hist_batch(t, rect=None):
            log.append(("hist", name_of(t, be), tuple(rect)))
            return torch.from_numpy(CR.hist(t.numpy(), rect).astype(np.int64))

        @staticmethod
        def colour_lut_batch(hs, hd, group):
            log.append(("table", group))
            return torch.from_numpy(CR.lut(hs.numpy(), hd.numpy(), group))

        @staticmethod
        def bgr_lut_batch(src, lut, rect=None, out=None):
            log.append(("lut", name_of(src, be), tuple(rect)))
            out[...] = torch.from_numpy(CR.apply(src.numpy(), lut.numpy(), rect))

        @staticmethod
        def render_stereo_source_batch(fd, dd, gl, gr, conv, layout, sd, fill_eyes, ax, bx, ay, by, out=None, subpixel=False):
            log.append(("render", name_of(out, be), fill_eyes))
            for i in range(len(fd)):
                out[i] = torch.from_numpy(X.render(fd[i].numpy(), dd[i].numpy().view(np.uint16), gl, gr, conv, layout, subpixel, sd[i].numpy(),
                                                   fill_eyes, ax, bx, ay, by))

        @staticmethod
        def verify_eye_source_batch(eye_bgr, sbs, eye, ax, bx, ay, by, tau, out=None):
            log.append(("verify", name_of(eye_bgr, be), eye))
            want, counts = V.verify_batch(eye_bgr.numpy(), sbs.numpy(), eye, ax, bx, ay, by, tau)
            eye_bgr[...] = torch.from_numpy(want)
            out[...] = torch.from_numpy(counts.astype(np.int32))

        @staticmethod
        def eye_fidelity_batch(eye_bgr, sbs, eye, ax, bx, ay, by, bad_thr, out=None, ws=None):
            log.append(("fidelity", name_of(eye_bgr, be), eye))
            out[...] = torch.from_numpy(F.fidelity_batch(np.ascontiguousarray(eye_bgr.numpy()), sbs.numpy(), eye, ax, bx, ay, by, bad_thr))

    class HostRenderBackend(HipRenderBackend):
        def __init__(self):
            self.torch, self.native, self.device, self._bufs = HostTorch, RefNative, "cpu", {}

        def _synchronize(self):
            pass

        def _event(self):
            return types.SimpleNamespace(query=lambda: True, synchronize=lambda: None)

    be = HostRenderBackend()
    return be


@pytest.mark.parametrize("layout", [P.FULL_SBS, P.FULL_TB])
@pytest.mark.parametrize("mode", [None, "clip", "frame"])
def test_backend_sequence_scratch_render_and_whole_frame_table(layout, mode):
    rng = np.random.default_rng(3)
    W, H, n = 48, 32, 2
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    depths = [rng.integers(0, 65536, (H, W), dtype=np.uint16) for _ in range(n)]
    sbs = [rng.integers(0, 256, (H // 2, W, 3), dtype=np.uint8) for _ in range(n)]
    q, gains = (32768, -16384, 32768, -16384), (0, -(3 << 8), 0)
    eye_rect, frame_rect = (0, 0, W // 2, H // 2), (0, 0, W, H)
    table = CR.lut(CR.hist(np.stack(sbs), eye_rect), CR.hist(np.stack(frames), frame_rect), n)
    match = None if mode is None else dict(mode=mode, table=table[0] if mode == "clip" else None, eye_rect=eye_rect, frame_rect=frame_rect)

    def call(fid, verify):
        log = []
        be = _host_backend(log)
        src = dict(frames=sbs, fill_eyes=2, q=q)
        if match is not None:
            src["match"] = match
        if verify:
            src["verify"] = dict(tau=48)
        if fid:
            src["fidelity"] = dict(bad_thr=BAD, ceiling=True)
        out = np.array(be.render_batch(frames, depths, *gains, layout, capacity=4, source=src))
        return be, log, out
    for verify in (False, True):
        plain_be, plain_log, plain = call(False, verify)
        be, log, out = call(True, verify)
        assert np.array_equal(out, plain), "the report changed an output byte"
        assert plain_be.fidelity_handle() is None and "fidelity_out_dev" not in plain_be._bufs
        half, whole = (W // 2, 0, W, H // 2), (0, 0, W, H // 2)
        pre = {None: [], "clip": [("lut", "sbs_dev", whole)],
               "frame": [("hist", "sbs_dev", eye_rect), ("hist", "frames_dev", frame_rect), ("table", 1), ("lut", "sbs_dev", whole)]}[mode]
        assert [(e[0], e[1], half) if e[0] == "lut" else e for e in pre] + [("render", "out_dev", 2)] + \
            ([("verify", "out_dev", 1)] if verify else []) == plain_log
        assert log == pre + [("render", "out_dev", 2)] + ([("verify", "out_dev", 1)] if verify else []) + \
            [("render", "fidelity_out_dev", 0), ("fidelity", "fidelity_out_dev", 1), ("fidelity", "out_dev", 1), ("fidelity", "out_dev", 0)]
        # the records: the reference on the render without fill, on the written right eye, on the 4K frame -- against the stored
        # eyes in the grading the render saw them in
        recs = be.read_fidelity(be.fidelity_handle())
        assert be.fidelity_handle() is None and len(recs) == 3 and all(r.shape == (n, 6) for r in recs)
        graded = np.stack(sbs) if mode is None else CR.apply(np.stack(sbs), table[0] if mode == "clip" else
                                                             CR.lut(CR.hist(np.stack(sbs), eye_rect), CR.hist(np.stack(frames), frame_rect), 1),
                                                             (0, 0, W, H // 2))
        warp = np.stack([X.render(f, d, *gains, layout, False, s, 0, *q) for f, d, s in zip(frames, depths, graded)])
        for r, (img, eye) in zip(recs, ((_eyes(warp, layout, W, H)[1], 1), (_eyes(out, layout, W, H)[1], 1), (_eyes(out, layout, W, H)[0], 0))):
            assert np.array_equal(r, F.fidelity_batch(np.ascontiguousarray(img), graded, eye, *q, BAD))
        assert np.array_equal(_eyes(out, layout, W, H)[0], np.stack(frames))
