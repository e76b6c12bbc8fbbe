"""Host logic of --verify-source on the CPU: the refusals of the plan and the CLI, the convert step's calls, manifest block, summary
and warning over a NumPy stand-in backend (tests/stereo_source_ref.py + tests/verify_ref.py in place of the HIP entries), the NumPy
surface, that nothing changes without the flag, and the experiment of DESIGN.md section 4, "Source-verified right eye", done with
the references and the oracle's matcher."""
import json

import numpy as np
import pytest

import stereo_pack_ref as P
import stereo_source_ref as X
import verify_ref as V
from test_convert_host import H4, W4, _pngs, _read_clip, sbs_clips  # noqa: F401
from test_pipeline_host import SH, SW
from test_source_parallax_host import SourceRenderBackend, _PackPipelineBackend, _convert, _pipeline


class VerifyRenderBackend(SourceRenderBackend):
    """the source-fill stand-in plus the verification of convert.HipRenderBackend: the right eye of the packed frame through
    tests/verify_ref.py, the counters kept for verify_counts()"""

    def __init__(self):
        super().__init__()
        self.verified, self.asked, self._counts = [], 0, None

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        verify = None if source is None else source.get("verify")
        self.verified.append(verify)
        out = super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)
        self._counts = None
        if verify is not None:
            assert layout in (P.FULL_SBS, P.FULL_TB)
            H, W = depths[0].shape
            eye = out[:, :, W:] if layout == P.FULL_SBS else out[:, H:]
            eye[...], self._counts = V.verify_batch(eye, np.stack(source["frames"]), 1, *source["q"], verify["tau"])
        return out

    def verify_counts(self):
        self.asked += 1
        counts, self._counts = self._counts, None
        return counts


@pytest.fixture()
def run(sbs_clips):
    """the clips of sbs_clips and the depth run of a --fill-from-source conversion -> the convert CLI's base arguments"""
    tmp, sbs, v4k, _ = sbs_clips
    _pipeline(tmp, sbs, v4k, "f", _PackPipelineBackend(), ctor=dict(depth_range="metric", fill_holes=True))
    return tmp, sbs, v4k, [v4k, tmp / "depth_f.json", "--parallax", "source", "--fill-from-source", sbs]


def _q():
    from video_3d_pipeline.register import map_to_q16
    return map_to_q16(1, 0, SW // 2, W4) + map_to_q16(1, 0, SH, H4)


def test_plan_and_cli_refusals(run, capsys):
    from video_3d_pipeline.convert import DEFAULT_VERIFY_TAU, DepthTo3DConverter, StereoPlan, check_verify_source
    assert DEFAULT_VERIFY_TAU == V.DEFAULT_TAU == 48 and V.TAU_MAX == 765
    with pytest.raises(ValueError, match="--fill-from-source"):
        StereoPlan(verify_source=48)
    assert StereoPlan(parallax="source", verify_source=48).verify_source == 48     # the NumPy surface: the SBS frame comes per call
    for layout in ("half-sbs", "half-tb", "interlaced", "anaglyph-colour", "anaglyph-dubois"):
        with pytest.raises(ValueError, match="full-sbs, full-tb"):
            StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, verify_source=48)
    for tau in (-1, 766, 2.5, True, "48"):
        with pytest.raises(ValueError, match="--verify-source"):
            StereoPlan(parallax="source", fill_from_source="s.npy", verify_source=tau)
    for layout in ("full-sbs", "full-tb"):
        assert StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, verify_source=0).verify_source == 0
    assert check_verify_source(765, "full-tb", "s.npy") == 765
    assert StereoPlan(parallax="source", fill_from_source="s.npy").verify_source is None
    with pytest.raises(ValueError, match="--fill-from-source"):
        DepthTo3DConverter(backend=VerifyRenderBackend(), verify_source=48)
    be = VerifyRenderBackend()
    with pytest.raises(ValueError, match="--fill-from-source"):  # a run over clips without the SBS clip
        DepthTo3DConverter(backend=be, parallax="source", verify_source=48).process_conversion(
            run[2], str(run[0] / "depth_f.json"), output_path=str(run[0] / "o.json"))
    assert not be.calls
    tmp, sbs, v4k, base = run
    out = ["--output", tmp / "o.json"]
    for args, word in (([v4k, tmp / "depth_f.json", "--parallax", "source", "--verify-source"], "--fill-from-source"),
                       ([v4k, tmp / "depth_f.json", "--verify-source", "48"], "--fill-from-source"),
                       (base + ["--verify-source", "--layout", "half-sbs"], "full-sbs, full-tb"),
                       (base + ["--layout", "anaglyph-dubois", "--verify-source", "20"], "full-sbs, full-tb"),
                       (base + ["--verify-source", "766"], "[0, 765]"),
                       (base + ["--verify-source", "-1"], "[0, 765]")):
        be = VerifyRenderBackend()
        assert _convert(args + out, be) == 1 and not be.calls, args
        assert word in capsys.readouterr().out, args
    assert not (tmp / "o.json").exists()


@pytest.mark.parametrize("layout", ["full-sbs", "full-tb"])
def test_cli_calls_manifest_summary_and_warning(run, capsys, layout):
    tmp, sbs, v4k, base = run
    q, code = _q(), P.FULL_SBS if layout == "full-sbs" else P.FULL_TB
    cx, cy = V.cell(q[0], q[2])
    cells = -(-W4 // cx) * -(-H4 // cy)
    plain = SourceRenderBackend()
    assert _convert(base + ["--layout", layout, "--output", tmp / "plain.json"], plain) == 0
    unverified = _read_clip(json.loads((tmp / "plain.json").read_text())["frames_dir"])
    sbs_frames = _read_clip(sbs)
    capsys.readouterr()
    be = VerifyRenderBackend()
    assert _convert(base + ["--layout", layout, "--verify-source", "--output", tmp / "v.json"], be) == 0
    text = capsys.readouterr().out
    man = json.loads((tmp / "v.json").read_text())
    assert be.verified == [{"tau": 48}, {"tau": 48}] and be.asked == 2 and be.calls == [(4, 2, q), (1, 2, q)]
    got = _read_clip(man["frames_dir"])
    shares = []
    for i in range(5):
        U = unverified[i]
        E = U[:, W4:] if code == P.FULL_SBS else U[H4:]
        want, n = V.verify(E, sbs_frames[i], 1, *q, 48)
        shares.append(n / cells)
        assert np.array_equal(got[i], P.pack(U[:, :W4] if code == P.FULL_SBS else U[:H4], want, code)), i
    rec = man["verify_source"]
    assert rec == {"tau": 48, "cell": [cx, cy], "replaced_share": float(np.mean(shares)), "replaced_share_max": max(shares)}
    assert {k: v for k, v in man.items() if k not in ("verify_source", "frames_dir")} == \
        {k: v for k, v in json.loads((tmp / "plain.json").read_text()).items() if k != "frames_dir"}
    # the 4K clip of these fixtures is noise, another picture than the SBS clip: nearly every cell disagrees, and the run says so
    assert rec["replaced_share"] > 0.25
    assert text.count("Source verify: tau 48") == 1 and f"cells of {cx} x {cy}" in text
    assert text.count("Warning: --verify-source") == 1 and "--match-colour" in text and "align --register-spatial" in text
    # a threshold nothing can pass: the frames of the unverified run, a share of 0, the summary and no warning
    be = VerifyRenderBackend()
    assert _convert(base + ["--layout", layout, "--verify-source", "765", "--output", tmp / "z.json"], be) == 0
    text = capsys.readouterr().out
    man = json.loads((tmp / "z.json").read_text())
    assert man["verify_source"] == {"tau": 765, "cell": [cx, cy], "replaced_share": 0.0, "replaced_share_max": 0.0}
    assert "Source verify: tau 765" in text and "Warning: --verify-source" not in text
    assert all(np.array_equal(a, b) for a, b in zip(_read_clip(man["frames_dir"]), unverified))


def test_colour_matching_comes_first(run):
    """with --match-colour the verification compares against the corrected eye: the backend's source entry carries both"""
    from test_colour_host import ColourRenderBackend

    class Both(ColourRenderBackend, VerifyRenderBackend):
        pass
    tmp, sbs, v4k, base = run
    be = Both()
    assert _convert(base + ["--match-colour", "clip", "--match-probes", "2", "--verify-source", "30", "--output", tmp / "b.json"], be) == 0
    assert be.verified == [{"tau": 30}, {"tau": 30}] and all(m is not None for m in be.matches) and ("table", 2) in be.colour
    man = json.loads((tmp / "b.json").read_text())
    assert man["verify_source"]["tau"] == 30 and man["match_colour"] == "clip"


def test_default_output_name_carries_the_threshold(run, monkeypatch):
    tmp, sbs, v4k, base = run
    monkeypatch.chdir(tmp)
    assert _convert(base + ["--verify-source", "20"], VerifyRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_vs20_depth_f.mp4").exists() or (tmp / "3d_full-sbs_srcpx_srcfill_vs20_depth_f_frames").is_dir()
    assert _convert(base, SourceRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_depth_f_frames").is_dir()


def test_numpy_surface(run):
    from video_3d_pipeline.convert import DepthTo3DConverter
    from video_3d_pipeline.utils import read_png16
    tmp, sbs, v4k, _ = run
    dman = json.loads((tmp / "depth_f.json").read_text())
    frames4k, sbs_frames = _read_clip(v4k), _read_clip(sbs)
    d = read_png16(f"{dman['frames_dir']}/depth4k_000000.png")
    for layout, code in (("full-sbs", P.FULL_SBS), ("full-tb", P.FULL_TB)):
        plain = DepthTo3DConverter(backend=SourceRenderBackend(), parallax="source", layout=layout)
        plain.set_source_parallax(dman["depth_range"], W4)
        U = plain.render_frame(frames4k[0], d, source=sbs_frames[0])
        be = VerifyRenderBackend()
        conv = DepthTo3DConverter(backend=be, parallax="source", layout=layout, verify_source=40)
        conv.set_source_parallax(dman["depth_range"], W4)
        got = conv.render_frame(frames4k[0], d, source=sbs_frames[0])
        EL, ER = (U[:, :W4], U[:, W4:]) if code == P.FULL_SBS else (U[:H4], U[H4:])
        want, n = V.verify(ER, sbs_frames[0], 1, *_q(), 40)
        assert np.array_equal(got, P.pack(EL, want, code)) and n > 0 and be.verified == [{"tau": 40}]
        cx, cy = V.cell(_q()[0], _q()[2])
        assert conv.plan.steps[0].shares == [n / (-(-W4 // cx) * -(-H4 // cy))]
        # without a source frame there is nothing to verify against: the plain render, no verify entry, nothing counted
        assert np.array_equal(conv.render_frame(frames4k[0], d), P.render(frames4k[0], d, *conv.gains, code))
        assert be.verified == [{"tau": 40}, None] and be.asked == 1


def test_nothing_changes_without_the_flag(run):
    """no verify entry in the backend's calls, no counters asked for, no manifest key, the bytes of a backend that predates it"""
    tmp, sbs, v4k, base = run
    old = SourceRenderBackend()                                # has no verify_counts at all
    assert _convert(base + ["--output", tmp / "old.json"], old) == 0
    be = VerifyRenderBackend()
    assert _convert(base + ["--output", tmp / "new.json"], be) == 0
    assert be.verified == [None, None] and be.asked == 0 and be.calls == old.calls
    a, b = json.loads((tmp / "old.json").read_text()), json.loads((tmp / "new.json").read_text())
    assert sorted(a) == sorted(b) and "verify_source" not in b
    assert _pngs(a["frames_dir"]) == _pngs(b["frames_dir"])
    from video_3d_pipeline.convert import StereoPlan
    plan = StereoPlan(parallax="source", fill_from_source=sbs)
    assert "verify" not in plan.source_kwargs([np.zeros((SH, SW, 3), np.uint8)], (W4, H4))["source"]


# ------------------------------------------------------------------------------------------------------------------------
# the experiment
# ------------------------------------------------------------------------------------------------------------------------
def _zoom2(a):
    from scipy.ndimage import zoom
    return np.clip(np.rint(zoom(a.astype(np.float32), (2, 2, 1), order=1, mode="nearest", grid_mode=True)), 0, 255).astype(np.uint8)


def _truth_in_the_left_view(dR):
    """the ground-truth disparity carried into the left view, as tests/test_source_parallax_host.py does"""
    H, W = dR.shape
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
    return dL


@pytest.mark.parametrize("seed", [0, 1])
def test_verify_quality(oracle, seed):
    """synthetic.stereo_pair(480, 270, seed), frame and truth enlarged 2x, the SBS frame's eye 240 x 270 (cells of 4 x 2), depth: the
    oracle matcher's disparity, scanline-filled and repeated 2x, or the ground truth; --parallax source gains; error: mean absolute
    BGR error of the right eye against the true one.

    Measured with these references (seed 0 / seed 1): matcher's disparity, source fill alone 4.32 / 4.22, verified at tau 48
    2.27 / 2.30 (ratio 0.525 / 0.544, 6.6 % / 6.5 % of the cells replaced); ground truth 1.51 / 1.52 -> 1.43 / 1.44 with 0.25 % of
    the cells replaced."""
    import fill_ref
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline._native import stereo_gains
    from video_3d_pipeline.convert import fill_map_q16, source_parallax
    W, H = 480, 270
    L, Rt = syn.stereo_pair(W, H, seed)
    frame, truth = _zoom2(L), _zoom2(Rt)
    sbs = syn.sbs_frame(W, H, seed)
    q = fill_map_q16(None, (W // 2, H), (2 * W, 2 * H))
    assert q == (16384, -24576, 32768, -16384) and V.cell(q[0], q[2]) == (4, 2)
    cells = (2 * W // 4) * (2 * H // 2)
    wl, wr = oracle.sbs_to_gray(sbs, True)
    matcher = np.maximum(fill_ref.fill_frame(oracle.sgbm_compute(wl, wr)), 0) / 16.0
    p = source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": W}, 2 * W)
    gains = stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])

    def err(E):
        return float(np.abs(E.astype(int) - truth.astype(int)).mean())

    def both(d):
        D = np.repeat(np.repeat(np.rint(d / 64 * 65535).astype(np.uint16), 2, axis=0), 2, axis=1)
        ER = X.eyes(frame, D, *gains, False, sbs, 2, *q)[1]
        out, n = V.verify(ER, sbs, 1, *q, 48)
        return err(ER), err(out), n / cells
    e0, e1, share = both(matcher)
    print(f"seed {seed}, matcher's disparity: source fill {e0:.2f}, verified {e1:.2f} (ratio {e1 / e0:.3f}), {share:.2%} of the cells replaced")
    assert e1 <= 0.65 * e0
    g0, g1, gshare = both(_truth_in_the_left_view(syn.gt_disparity(W, H)))
    print(f"seed {seed}, ground truth: source fill {g0:.2f}, verified {g1:.2f}, {gshare:.2%} of the cells replaced")
    assert gshare <= 0.01 and g1 <= g0
