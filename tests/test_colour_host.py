"""Host logic of --match-colour on the CPU: colour.common_rects, the refusals of the plan and the CLI, the convert step's calls,
manifest keys and files over a NumPy stand-in backend (tests/colour_ref.py + tests/stereo_source_ref.py in place of the HIP
entries), and the experiment of DESIGN.md section 4, "Colour matching", done with the references."""
import json

import numpy as np
import pytest

import colour_ref as CR
import stereo_pack_ref as P
import stereo_ref as R
import stereo_source_ref as X
from test_convert_host import H4, W4, _pngs, _read_clip, sbs_clips  # noqa: F401
from test_pipeline_host import SH, SW
from test_source_parallax_host import SourceRenderBackend, _PackPipelineBackend, _convert, _pipeline


class ColourRenderBackend(SourceRenderBackend):
    """the source-fill stand-in plus the colour calls of convert.HipRenderBackend, each recorded"""

    def __init__(self):
        super().__init__()
        self.colour, self.matches = [], []

    def colour_probe(self, sbs_frames, frames, eye_rect, frame_rect):
        self.colour.append(("probe", len(sbs_frames), tuple(eye_rect), tuple(frame_rect)))
        return CR.hist(np.stack(sbs_frames), eye_rect), CR.hist(np.stack(frames), frame_rect)

    def colour_table(self, hists):
        hs, hd = (np.concatenate([h[k] for h in hists]) for k in (0, 1))
        self.colour.append(("table", len(hs)))
        table = CR.lut(hs, hd, len(hs))
        return table, table[0].copy()

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        match = None if source is None else source.get("match")
        self.matches.append(match)
        if match is not None:
            sbs = np.stack(source["frames"])
            Hs, Ws = sbs.shape[1:3]
            table = match["table"]
            if match["mode"] == "frame":
                table = CR.lut(CR.hist(sbs, match["eye_rect"]), CR.hist(np.stack(frames), match["frame_rect"]), 1)
            # a shared table has lut_stride 0, per-frame tables 768
            self.colour.append(("apply", len(sbs), 0 if np.asarray(table).reshape(-1, 3, 256).shape[0] == 1 else 768))
            source = {k: v for k, v in source.items() if k != "match"}
            source["frames"] = list(CR.apply(sbs, table, (Ws // 2, 0, Ws, Hs)))
        return super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)


# ------------------------------------------------------------------------------------------------------------------------
# the rectangles
# ------------------------------------------------------------------------------------------------------------------------
def test_common_rects():
    from video_3d_pipeline.colour import common_rects
    eye, frame = (960, 1080), (3840, 2160)
    assert common_rects(None, eye, frame) == ((0, 0, 960, 1080), (0, 0, 3840, 2160)) == common_rects((1, 0, 1, 0), eye, frame)
    # a crop: the 4K frame shows the middle half of the eye's width
    assert common_rects((0.5, 0.25, 1, 0), eye, frame) == ((240, 0, 720, 1080), (0, 0, 3840, 2160))
    # a letterbox: the eye's picture fills the middle 80 % of the frame's height (eye = 1.25 frame - 0.125)
    assert common_rects((1, 0, 1.25, -0.125), eye, frame) == ((0, 0, 960, 1080), (0, 216, 3840, 1944))
    # a shift: the frame's left edge is an eighth into the eye
    assert common_rects((1, 0.125, 1, 0), eye, frame) == ((120, 0, 960, 1080), (0, 0, 3360, 2160))
    # the map is taken as the binary number it is: 0.1 as a float lies above 1/10, and inward rounding gives 97 and 3455, not 96 and 3456
    assert common_rects((1, 0.1, 1, 0), eye, frame) == ((97, 0, 960, 1080), (0, 0, 3455, 2160))
    # inward rounding: a third of an odd-sized plane
    e, f = common_rects((1, 1 / 3, 1, 0), (100, 50), (200, 100))
    assert e == (34, 0, 100, 50) and f[0] == 0 and f[2] in (133, 134) and f[2] / 200 <= 2 / 3 + 1e-9
    for bad in ((1, 1.0, 1, 0), (1, 2, 1, 0), (1, 0, 1, -1.5), (1, 0, 1, 1 - 1e-6), (0, 0, 1, 0), (-1, 1, 1, 0)):
        with pytest.raises(ValueError):
            common_rects(bad, eye, frame)


def test_plan_and_cli_refusals(sbs_clips, capsys):
    from video_3d_pipeline.convert import DepthTo3DConverter, StereoPlan
    with pytest.raises(ValueError, match="--fill-from-source"):
        StereoPlan(parallax="source", match_colour="clip")
    with pytest.raises(ValueError, match="--match-colour"):
        StereoPlan(parallax="source", fill_from_source="s.npy", match_probes=8)
    with pytest.raises(ValueError, match="clip"):
        StereoPlan(parallax="source", fill_from_source="s.npy", match_colour="frame", match_probes=8)
    for probes in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="--match-probes"):
            StereoPlan(parallax="source", fill_from_source="s.npy", match_colour="clip", match_probes=probes)
    with pytest.raises(ValueError, match="--match-colour"):
        StereoPlan(parallax="source", fill_from_source="s.npy", match_colour="scene")
    plan = StereoPlan(parallax="source", fill_from_source="s.npy", match_colour="clip")
    assert (plan.match_colour, plan.match_probes) == ("clip", 16)
    with pytest.raises(ValueError, match="source="):
        conv = DepthTo3DConverter(backend=ColourRenderBackend(), parallax="source")
        conv.set_source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": 8}, 8)
        conv.render_frame(np.zeros((2, 8, 3), np.uint8), np.zeros((2, 8), np.uint16), colour_table=np.zeros((3, 256), np.uint8))
    tmp, sbs, v4k, _ = sbs_clips
    _pipeline(tmp, sbs, v4k, "r", _PackPipelineBackend(), ctor=dict(depth_range="metric", fill_holes=True))
    base = [v4k, tmp / "depth_r.json", "--output", tmp / "o.json", "--parallax", "source"]
    for extra, word in ((["--match-colour", "clip"], "--fill-from-source"),
                        (["--match-probes", "4"], "--match-colour"),
                        (["--fill-from-source", sbs, "--match-probes", "4"], "--match-colour"),
                        (["--fill-from-source", sbs, "--match-colour", "frame", "--match-probes", "4"], "clip"),
                        (["--fill-from-source", sbs, "--match-colour", "clip", "--match-probes", "0"], "[1, 64]")):
        be = ColourRenderBackend()
        assert _convert(base + extra, be) == 1 and not be.calls and not be.colour, extra
        assert word in capsys.readouterr().out, extra
    assert not (tmp / "o.json").exists()


# ------------------------------------------------------------------------------------------------------------------------
# the convert CLI over the stand-in
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def graded(sbs_clips):
    """the clips of sbs_clips, the depth run of a --fill-from-source conversion, and a graded copy of the SBS clip"""
    tmp, sbs, v4k, _ = sbs_clips
    _pipeline(tmp, sbs, v4k, "f", _PackPipelineBackend(), ctor=dict(depth_range="metric", fill_holes=True))
    np.save(tmp / "sbs_graded.npy", CR.grade(np.stack(_read_clip(sbs))))
    return tmp, str(tmp / "sbs_graded.npy"), v4k, tmp / "depth_f.json"


def _expected(frames4k, depth_json, man, sbs_frames, tables):
    from video_3d_pipeline.utils import read_png16
    dman = json.loads(depth_json.read_text())
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    from video_3d_pipeline.register import map_to_q16
    q = map_to_q16(1, 0, SW // 2, W4) + map_to_q16(1, 0, SH, H4)
    out = []
    for i in range(man["count"]):
        d = read_png16(f"{dman['frames_dir']}/depth4k_{i:06d}.png")
        s = CR.apply(sbs_frames[i][None], tables[i], (SW // 2, 0, SW, SH))[0]
        out.append(X.render(frames4k[i], d, *gains, P.FULL_SBS, False, s, 2, *q))
    return out


def test_clip_mode_one_probe_pass_one_table(graded):
    tmp, sbs, v4k, depth = graded
    be = ColourRenderBackend()
    assert _convert([v4k, depth, "--output", tmp / "c.json", "--parallax", "source", "--fill-from-source", sbs, "--match-colour", "clip",
                     "--match-probes", "3"], be) == 0
    man = json.loads((tmp / "c.json").read_text())
    n = man["count"]
    assert n == 5 and man["match_colour"] == "clip" and man["colour_probe_frames"] == [0, 2, 4]
    eye, frame = (0, 0, SW // 2, SH), (0, 0, W4, H4)
    assert be.colour[:2] == [("probe", 3, eye, frame), ("table", 3)]                  # one probe pass (3 <= 4 pairs: one upload), one table
    assert be.colour[2:] == [("apply", 4, 0), ("apply", 1, 0)]                        # the shared table on every batch
    assert all(m["mode"] == "clip" and m["table"] is be.matches[0]["table"] for m in be.matches)
    frames4k, sbs_frames = _read_clip(v4k), _read_clip(sbs)
    table = CR.lut(CR.hist(np.stack([sbs_frames[i] for i in (0, 2, 4)]), eye), CR.hist(np.stack([frames4k[i] for i in (0, 2, 4)]), frame), 3)
    side = json.loads(open(man["colour_lut"]).read())
    assert man["colour_lut"] == str(tmp / "c_frames" / "colour_lut.json")
    assert np.array_equal(np.array(side["lut"], np.uint8), table[0]) and side["probe_frames"] == [0, 2, 4] and side["channels"] == "BGR"
    assert side["eye_rect"] == list(eye) and side["frame_rect"] == list(frame)
    got = _read_clip(man["frames_dir"])
    want = _expected(frames4k, depth, man, sbs_frames, [table] * n)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert any(not np.array_equal(w, u) for w, u in zip(want, _expected(frames4k, depth, man, sbs_frames, [np.arange(256, dtype=np.uint8)[None].repeat(3, 0)] * n)))
    # the NumPy surface applies a table the same way
    from video_3d_pipeline.convert import DepthTo3DConverter
    from video_3d_pipeline.utils import read_png16
    dman = json.loads(depth.read_text())
    conv = DepthTo3DConverter(backend=ColourRenderBackend(), parallax="source")
    conv.set_source_parallax(dman["depth_range"], W4)
    d = read_png16(f"{dman['frames_dir']}/depth4k_000000.png")
    assert np.array_equal(conv.render_frame(frames4k[0], d, source=sbs_frames[0], colour_table=table[0]), got[0])
    # more probes than frames: every frame once
    be = ColourRenderBackend()
    assert _convert([v4k, depth, "--output", tmp / "c2.json", "--parallax", "source", "--fill-from-source", sbs, "--match-colour", "clip"], be) == 0
    assert json.loads((tmp / "c2.json").read_text())["colour_probe_frames"] == [0, 1, 2, 3, 4]
    assert [c for c in be.colour if c[0] != "apply"] == [("probe", 4, eye, frame), ("probe", 1, eye, frame), ("table", 5)]


def test_frame_mode_no_probe_pass(graded):
    tmp, sbs, v4k, depth = graded
    be = ColourRenderBackend()
    assert _convert([v4k, depth, "--output", tmp / "f.json", "--parallax", "source", "--fill-from-source", sbs, "--match-colour", "frame"], be) == 0
    man = json.loads((tmp / "f.json").read_text())
    assert man["match_colour"] == "frame" and "colour_probe_frames" not in man and "colour_lut" not in man
    assert not (tmp / "f_frames" / "colour_lut.json").exists()
    assert be.colour == [("apply", 4, 768), ("apply", 1, 0)] and all(m["mode"] == "frame" and m["table"] is None for m in be.matches)
    frames4k, sbs_frames = _read_clip(v4k), _read_clip(sbs)
    tables = [CR.lut(CR.hist(sbs_frames[i][None], (0, 0, SW // 2, SH)), CR.hist(frames4k[i][None], None), 1) for i in range(5)]
    assert all(np.array_equal(g, w) for g, w in zip(_read_clip(man["frames_dir"]), _expected(frames4k, depth, man, sbs_frames, tables)))


def test_nothing_changes_without_the_flag(graded):
    """a --fill-from-source run: the calls, the manifest keys and the bytes of a backend that knows nothing of colour; and the cache
    names: unchanged without the flag, `_cm` / `_cmf` appended with it"""
    tmp, sbs, v4k, depth = graded
    args = ["--parallax", "source", "--fill-from-source", sbs]
    old, new = SourceRenderBackend(), ColourRenderBackend()
    assert _convert([v4k, depth, "--output", tmp / "old.json"] + args, old) == 0
    assert _convert([v4k, depth, "--output", tmp / "new.json"] + args, new) == 0
    assert old.calls == new.calls and not new.colour and new.matches == [None, None]
    a, b = json.loads((tmp / "old.json").read_text()), json.loads((tmp / "new.json").read_text())
    assert sorted(a) == sorted(b) and not {"match_colour", "colour_probe_frames", "colour_lut"} & set(b)
    assert _pngs(a["frames_dir"]) == _pngs(b["frames_dir"])
    assert sorted(p.name for p in (tmp / "new_frames").iterdir()) == sorted(p.name for p in (tmp / "old_frames").iterdir())
    import os
    from video_3d_pipeline.convert import DepthTo3DConverter
    names = {}
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        for mode in (None, "clip", "frame"):
            kw = {} if mode is None else {"match_colour": mode}
            conv = DepthTo3DConverter(backend=ColourRenderBackend(), parallax="source", fill_from_source=sbs, **kw)
            names[mode] = os.path.basename(conv.process_conversion(v4k, str(depth), max_frames=1))
    finally:
        os.chdir(cwd)
    assert names == {None: "3d_full-sbs_srcpx_srcfill_depth_f.mp4", "clip": "3d_full-sbs_srcpx_srcfill_cm_depth_f.mp4",
                     "frame": "3d_full-sbs_srcpx_srcfill_cmf_depth_f.mp4"}


# ------------------------------------------------------------------------------------------------------------------------
# the experiment
# ------------------------------------------------------------------------------------------------------------------------
def test_colour_match_quality():
    """The setup of tests/test_source_parallax_host.py::test_source_parallax_quality (synthetic.stereo_pair(480, 270, 0), ground-truth
    metric depth, the holes of the right eye filled from the stored 2:1 squeezed right eye), with the SBS frame graded per BGR channel
    by colour_ref.grade (gamma (1.25, 0.9, 0.8), gain (0.85, 1.0, 1.12), offset (-6, 10, 14)).  Mean absolute BGR error of the hole
    pixels against the true right eye; the table is fitted left eye -> 4K frame (= the left view) and applied to the right eye.

    Measured with these references: ungraded source 4.89, graded and unmatched 36.74, graded and matched 4.68 (the stretched
    background without any source fill: 35.43)."""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline._native import stereo_gains
    from video_3d_pipeline.colour import common_rects
    from video_3d_pipeline.convert import fill_map_q16, source_parallax
    W, H = 480, 270
    L, Rt = syn.stereo_pair(W, H, 0)
    dR = syn.gt_disparity(W, H)
    dL = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in np.argsort(dR[y], kind="stable"):
            t = int(round(x + float(dR[y, x])))
            if 0 <= t < W:
                dL[y, t] = max(dL[y, t], dR[y, x])
        idx = np.flatnonzero(dL[y] > 0)
        for x in np.flatnonzero(dL[y] == 0):
            a, b = idx[idx < x], idx[idx > x]
            dL[y, x] = min(([dL[y, a[-1]]] if len(a) else []) + ([dL[y, b[0]]] if len(b) else []))
    D = np.rint(dL / 64 * 65535).astype(np.uint16)
    p = source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": W}, W)
    gains = stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    hole = ~X.hit_mask(D, gains[1], gains[2])
    assert 0.02 <= hole.mean() <= 0.15

    def err(E):
        return float(np.abs(E.astype(int) - Rt.astype(int)).mean(axis=2)[hole].mean())

    sbs = syn.sbs_frame(W, H, 0)
    q = fill_map_q16(None, (W // 2, H), (W, H))
    graded = CR.grade(sbs)
    eye_rect, frame_rect = common_rects(None, (W // 2, H), (W, H))
    table = CR.lut(CR.hist(graded[None], eye_rect), CR.hist(L[None], frame_rect), 1)
    matched_sbs = CR.apply(graded[None], table, (W // 2, 0, W, H))[0]
    assert np.array_equal(matched_sbs[:, :W // 2], graded[:, :W // 2])               # the left eye is only measured
    plain = R.render(L, D, *gains)[:, W:]
    eyes = {name: X.eyes(L, D, *gains, False, s, 2, *q)[1] for name, s in (("ungraded", sbs), ("unmatched", graded), ("matched", matched_sbs))}
    ungraded, unmatched, matched = (err(eyes[k]) for k in ("ungraded", "unmatched", "matched"))
    print(f"hole error: background {err(plain):.2f}, ungraded source {ungraded:.2f}, graded unmatched {unmatched:.2f}, graded matched {matched:.2f}")
    assert matched <= ungraded + 0.25 * (unmatched - ungraded)
    for E in eyes.values():                                                          # hit pixels are untouched by the fill and by the match
        assert np.array_equal(E[~hole], plain[~hole])
