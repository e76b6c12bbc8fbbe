"""Host logic of --fuse-source on the CPU: the refusals of the plan and the CLI, the convert step's calls, manifest block and notes
over a NumPy stand-in backend (tests/stereo_source_ref.py, tests/verify_ref.py and tests/fuse_ref.py in place of the HIP entries), the
NumPy surface, that nothing changes without the flag, and the quality condition of DESIGN.md section 4, "Source-fused right eye",
on synthetic scenes with a known true right eye, done with the references alone."""
import json

import numpy as np
import pytest

import fuse_ref as F
import stereo_pack_ref as P
import stereo_source_ref as X
import verify_ref as V
from test_convert_host import H4, W4, _pngs, _read_clip, sbs_clips  # noqa: F401
from test_pipeline_host import SH, SW
from test_source_parallax_host import SourceRenderBackend, _convert
from test_verify_host import VerifyRenderBackend, _q, run  # noqa: F401


class FuseRenderBackend(VerifyRenderBackend):
    """the source-fill and verify stand-in plus the fusion of convert.HipRenderBackend: the right eye of the packed frame, verified
    or not, through tests/fuse_ref.py"""

    def __init__(self):
        super().__init__()
        self.fused = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        fuse = None if source is None else source.get("fuse")
        self.fused.append(fuse)
        out = super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)
        if fuse is not None:
            assert layout in (P.FULL_SBS, P.FULL_TB)
            H, W = depths[0].shape
            eye = out[:, :, W:] if layout == P.FULL_SBS else out[:, H:]
            eye[...] = F.fuse_batch(eye, np.stack(source["frames"]), 1, *source["q"])
        return out


def test_plan_and_cli_refusals(run, capsys):  # noqa: F811
    from video_3d_pipeline.convert import DepthTo3DConverter, StereoPlan, check_source_rules
    from video_3d_pipeline.verify import SourceFuser, check_fuse_source
    with pytest.raises(ValueError, match="--fuse-source needs parallax='source'"):
        StereoPlan(fuse_source=True)
    assert StereoPlan(parallax="source", fuse_source=True).fuse_source is True       # the NumPy surface: the SBS frame comes per call
    for layout in ("half-sbs", "half-tb", "interlaced", "anaglyph-colour", "anaglyph-dubois"):
        with pytest.raises(ValueError, match="--fuse-source works on the layouts full-sbs, full-tb"):
            StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, fuse_source=True)
    for layout in ("full-sbs", "full-tb"):
        plan = StereoPlan(parallax="source", fill_from_source="s.npy", layout=layout, fuse_source=True)
        assert [type(s) for s in plan.steps] == [SourceFuser] and plan.steps[0].output_tag == "_fu" and plan.steps[0].on_surface
    with pytest.raises(ValueError) as e:
        check_source_rules(None, layout="full-sbs", fuse_source=True)
    assert str(e.value) == ("--fuse-source needs --fill-from-source: it fuses the rendered right eye with the SBS clip's stored right "
                            "eye, which only the source fill uploads")
    assert check_source_rules(None, layout="half-sbs", fuse_source=False) is None and check_fuse_source("full-tb", "s.npy") is None
    be = FuseRenderBackend()
    with pytest.raises(ValueError, match="--fill-from-source"):  # a run over clips without the SBS clip
        DepthTo3DConverter(backend=be, parallax="source", fuse_source=True).process_conversion(
            run[2], str(run[0] / "depth_f.json"), output_path=str(run[0] / "o.json"))
    assert not be.calls
    tmp, sbs, v4k, base = run
    out = ["--output", tmp / "o.json"]
    for args, word in (([v4k, tmp / "depth_f.json", "--parallax", "source", "--fuse-source"], "--fuse-source needs --fill-from-source"),
                       ([v4k, tmp / "depth_f.json", "--fuse-source"], "--fuse-source needs --fill-from-source"),
                       (base + ["--fuse-source", "--layout", "half-sbs"], "--fuse-source works on the layouts full-sbs, full-tb"),
                       (base + ["--layout", "anaglyph-dubois", "--fuse-source"], "full-sbs, full-tb")):
        be = FuseRenderBackend()
        assert _convert(args + out, be) == 1 and not be.calls, args
        assert word in capsys.readouterr().out, args
    assert not (tmp / "o.json").exists()


def test_a_stored_eye_finer_than_the_frame_is_refused(run):  # noqa: F811
    """more than one stored sample per pixel on either axis: a ValueError that names the flag, before the backend is called"""
    from video_3d_pipeline.convert import StereoPlan
    from video_3d_pipeline.verify import SourceFuser
    tmp, sbs, v4k, _ = run
    plan = StereoPlan(parallax="source", fill_from_source=sbs, fuse_source=True)
    assert "fuse" in plan.source_kwargs([np.zeros((H4, 2 * W4, 3), np.uint8)], (W4, H4))["source"]            # one sample per pixel
    for shape in ((H4, 2 * W4 + 2, 3), (H4 + 1, 2 * W4, 3), (2 * H4, 4 * W4, 3)):
        with pytest.raises(ValueError, match="--fuse-source: the map has .* stored samples per pixel"):
            plan.source_kwargs([np.zeros(shape, np.uint8)], (W4, H4))
    assert StereoPlan(parallax="source", fill_from_source=sbs).source_kwargs([np.zeros((2 * H4, 4 * W4, 3), np.uint8)], (W4, H4))
    step = SourceFuser()
    assert step.check_map((65536, 0, 65536, 0)) is None and step.check_map((4096, 5, 4096, -5)) is None
    for q in ((65537, 0, 65536, 0), (65536, 0, 1 << 20, 0)):
        with pytest.raises(ValueError, match="--fuse-source"):
            step.check_map(q)


@pytest.mark.parametrize("layout", ["full-sbs", "full-tb"])
@pytest.mark.parametrize("verify", [False, True])
def test_cli_calls_manifest_and_notes(run, capsys, layout, verify):  # noqa: F811
    tmp, sbs, v4k, base = run
    q, code = _q(), P.FULL_SBS if layout == "full-sbs" else P.FULL_TB
    plain = SourceRenderBackend()
    assert _convert(base + ["--layout", layout, "--output", tmp / "plain.json"], plain) == 0
    unfused = _read_clip(json.loads((tmp / "plain.json").read_text())["frames_dir"])
    sbs_frames = _read_clip(sbs)
    capsys.readouterr()
    be = FuseRenderBackend()
    flags = ["--verify-source", "30"] if verify else []
    assert _convert(base + ["--layout", layout, "--fuse-source", "--output", tmp / "f.json"] + flags, be) == 0
    text = capsys.readouterr().out
    man = json.loads((tmp / "f.json").read_text())
    assert be.fused == [{}, {}] and be.calls == [(4, 2, q), (1, 2, q)] and be.verified == [{"tau": 30} if verify else None] * 2
    got = _read_clip(man["frames_dir"])
    for i in range(5):
        U = unfused[i]
        E = U[:, W4:] if code == P.FULL_SBS else U[H4:]
        if verify:
            E = V.verify(E, sbs_frames[i], 1, *q, 30)[0]
        want = F.fuse(E, sbs_frames[i], 1, *q)
        assert (want != E).any()
        assert np.array_equal(got[i], P.pack(U[:, :W4] if code == P.FULL_SBS else U[:H4], want, code)), i
    assert man["fuse_source"] == {"samples_per_pixel": [q[0] / 65536, q[2] / 65536]} == {"samples_per_pixel": [0.25, 0.5]}
    assert list(man)[-1] == "fuse_source" and (list(man)[-2] == "verify_source") == verify
    assert {k: v for k, v in man.items() if k not in ("fuse_source", "verify_source", "frames_dir")} == \
        {k: v for k, v in json.loads((tmp / "plain.json").read_text()).items() if k != "frames_dir"}
    # without --match-colour the run says once whose grading the low band carries
    assert text.count("the right eye's low band now carries the SBS release's grading") == 1
    assert text.count("Source fuse: the right eye's low band from the stored eye, 0.25 x 0.5 stored samples per pixel") == 1
    assert not verify or text.index("Source verify:") < text.index("Source fuse: the right eye's low band from")


def test_with_colour_matching_the_note_stays_away_and_the_steps_keep_their_order(run, capsys):  # noqa: F811
    from test_colour_host import ColourRenderBackend
    from test_fidelity_host import FidelityRenderBackend

    class All(ColourRenderBackend, FidelityRenderBackend, FuseRenderBackend):
        def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
            self.keys = list(source)
            return super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)
    tmp, sbs, v4k, base = run
    be = All()
    capsys.readouterr()
    assert _convert(base + ["--match-colour", "clip", "--match-probes", "2", "--verify-source", "30", "--fuse-source", "--fidelity-report",
                            "--output", tmp / "a.json"], be) == 0
    text = capsys.readouterr().out
    assert be.keys == ["frames", "fill_eyes", "q", "match", "verify", "fuse", "fidelity"] and be.fused == [{}, {}]
    assert "SBS release's grading" not in text and text.count("Source fuse:") == 1
    man = json.loads((tmp / "a.json").read_text())
    assert list(man)[-5:] == ["colour_probe_frames", "colour_lut", "verify_source", "fuse_source", "fidelity_report"]


def test_default_output_name_carries_the_tag(run, monkeypatch):  # noqa: F811
    tmp, sbs, v4k, base = run
    monkeypatch.chdir(tmp)
    assert _convert(base + ["--fuse-source"], FuseRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_fu_depth_f_frames").is_dir()
    assert _convert(base + ["--verify-source", "20", "--fuse-source"], FuseRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_vs20_fu_depth_f_frames").is_dir()
    assert _convert(base, SourceRenderBackend()) == 0
    assert (tmp / "3d_full-sbs_srcpx_srcfill_depth_f_frames").is_dir()


def test_numpy_surface(run):  # noqa: F811
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
        EL, ER = (U[:, :W4], U[:, W4:]) if code == P.FULL_SBS else (U[:H4], U[H4:])
        for tau in (None, 40):
            be = FuseRenderBackend()
            conv = DepthTo3DConverter(backend=be, parallax="source", layout=layout, verify_source=tau, fuse_source=True)
            conv.set_source_parallax(dman["depth_range"], W4)
            got = conv.render_frame(frames4k[0], d, source=sbs_frames[0])
            E = ER if tau is None else V.verify(ER, sbs_frames[0], 1, *_q(), tau)[0]
            assert np.array_equal(got, P.pack(EL, F.fuse(E, sbs_frames[0], 1, *_q()), code)) and be.fused == [{}]
            assert conv.plan.steps[-1].scales == [0.25, 0.5]
            # without a source frame there is nothing to fuse with: the plain render
            assert np.array_equal(conv.render_frame(frames4k[0], d), P.render(frames4k[0], d, *conv.gains, code)) and be.fused == [{}, None]


def test_nothing_changes_without_the_flag(run):  # noqa: F811
    """no fuse entry in the backend's calls, no step, no manifest key, no tag, the bytes of a backend that predates it"""
    from video_3d_pipeline.convert import StereoPlan
    from video_3d_pipeline.verify import SourceFuser
    tmp, sbs, v4k, base = run
    old = SourceRenderBackend()
    assert _convert(base + ["--output", tmp / "old.json"], old) == 0
    be = FuseRenderBackend()
    assert _convert(base + ["--output", tmp / "new.json"], be) == 0
    assert be.fused == [None, None] and be.calls == old.calls
    a, b = json.loads((tmp / "old.json").read_text()), json.loads((tmp / "new.json").read_text())
    assert list(a) == list(b) and "fuse_source" not in b
    assert _pngs(a["frames_dir"]) == _pngs(b["frames_dir"])
    for kw in (dict(), dict(fuse_source=False), dict(verify_source=48, match_colour="clip", fidelity_report=True)):
        plan = StereoPlan(parallax="source", fill_from_source=sbs, **kw)
        assert not any(isinstance(s, SourceFuser) for s in plan.steps) and plan.fuse_source is False
        assert "fuse" not in plan.source_kwargs([np.zeros((SH, SW, 3), np.uint8)], (W4, H4))["source"]
        assert "_fu" not in "".join(s.output_tag for s in plan.steps)


# ------------------------------------------------------------------------------------------------------------------------
# the quality condition
# ------------------------------------------------------------------------------------------------------------------------
QW, QH = 768, 128
GAINS = (0, -48 * 256, 0)                                      # eye_split 0, max_shift 48, convergence 0
Q = X.identity_map(QW // 4, QW) + X.identity_map(QH // 2, QH)


def _shift(depth):
    """the whole pixels the render moves a source of this depth by in the right eye (tests/stereo_ref.py)"""
    return (GAINS[1] * (int(depth) - GAINS[2]) + (1 << 23)) >> 24


def _box(a):
    """u8 [QH,QW,3] reduced 4 x 2 with the contract's rounding"""
    return ((a.reshape(QH // 2, 2, QW // 4, 4, 3).astype(np.int64).sum(axis=(1, 3)) * 2 + 8) // 16).astype(np.uint8)


def quality_scene(sigma, errors, seed=0):
    """two textured layers (a far plane, a nearer one over the lower rows) and three foreground rectangles, every layer with a
    texture of its own (Gaussian-filtered noise of smoothness sigma, +-30 levels) -> (the 4K frame = the left eye, the depth the
    render gets, the SBS frame: both eyes box-reduced 4 x 2, the true right eye).  The true right eye moves every layer, mask and
    texture, by the shift the render gives its depth, so a render from the clean depth is exact outside the disocclusions.
    errors: the depth handed to the render gets a wrong-depth blob on the far plane, every rectangle's depth bleeding 6 px past its
    edges, and a patch of the far plane's depth inside the first rectangle; the truth stays"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    pad = 64
    lower = np.zeros((QH, QW), bool)
    lower[70:] = True
    layers = [(6000, np.ones((QH, QW), bool)), (20000, lower)]
    for x0, x1, y0, y1, d in ((90, 210, 20, 100, 42000), (330, 420, 40, 120, 52000), (560, 690, 10, 80, 62000)):
        m = np.zeros((QH, QW), bool)
        m[y0:y1, x0:x1] = True
        layers.append((d, m))
    left, right, depth = np.zeros((QH, QW, 3), np.uint8), np.zeros((QH, QW, 3), np.uint8), np.zeros((QH, QW), np.uint16)
    for k, (d, m) in enumerate(layers):
        t = gaussian_filter(rng.standard_normal((QH, QW + 2 * pad, 3)), (sigma, sigma, 0))
        tex = np.clip(128 + 30 * (t - t.mean()) / t.std(), 0, 255).astype(np.uint8)
        s = _shift(d)
        left[m] = tex[:, pad:pad + QW][m]
        depth[m] = d
        src = np.arange(QW) - s                                 # target x shows the layer's column x - s
        ok = (src >= 0) & (src < QW)
        mr = np.zeros_like(m)
        mr[:, ok] = m[:, src[ok]]
        if k == 0:
            mr[:] = True                                        # the far plane goes on beyond the frame
        right[mr] = tex[:, pad - s:pad - s + QW][mr]
    if errors:
        yy, xx = np.mgrid[:QH, :QW]
        depth[(yy - 35) ** 2 + (xx - 480) ** 2 < 14 ** 2] = 45000
        for d, m in layers[2:]:
            grown = m.copy()
            for k in range(1, 7):
                grown[:, k:] |= m[:, :-k]
                grown[:, :-k] |= m[:, k:]
            depth[grown & ~m & (depth < d)] = d
        depth[50:70, 120:160] = 6000
    return left, depth, np.concatenate([_box(left), _box(right)], axis=1), right


def psnr(a, b):
    return float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


@pytest.mark.parametrize("sigma", [0.7, 1.5])
@pytest.mark.parametrize("errors", [False, True], ids=["clean", "errors"])
def test_fusion_beats_its_input(sigma, errors):
    """PSNR of the right eye against the true one, in dB, with the references alone (source fill | + verify at tau 48 | fill -> fuse |
    fill -> verify -> fuse):
        sigma 0.7, clean depth     31.55  31.42  32.01  31.90
        sigma 0.7, depth errors    27.42  28.44  28.59  29.06
        sigma 1.5, clean depth     35.86  35.64  37.54  37.35
        sigma 1.5, depth errors    29.00  32.45  32.97  34.08
    Fusion beats its own input on every scene, by +0.46 dB at the least; no figure is fixed here"""
    frame, depth, sbs, truth = quality_scene(sigma, errors)
    assert Q == (16384, -24576, 32768, -16384)
    fill = X.eyes(frame, depth, *GAINS, False, sbs, 2, *Q)[1]
    verified, replaced = V.verify(fill, sbs, 1, *Q, 48)
    rows = [psnr(e, truth) for e in (fill, verified, F.fuse(fill, sbs, 1, *Q), F.fuse(verified, sbs, 1, *Q))]
    print(f"sigma {sigma}, {'depth errors' if errors else 'clean depth'}: fill {rows[0]:.2f}, + verify {rows[1]:.2f}, fill -> fuse "
          f"{rows[2]:.2f}, fill -> verify -> fuse {rows[3]:.2f} dB ({replaced} cells replaced)")
    assert (fill != truth).any() and (not errors or replaced > 0)
    assert rows[2] > rows[0], "fuse(fill) does not beat fill"
    assert rows[3] > rows[1], "fuse(verify(fill)) does not beat verify(fill)"
