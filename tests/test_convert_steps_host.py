"""The convert step's source-eye options as steps (verify.SourceStep), on the CPU over the NumPy stand-in backends of the colour,
verify and fidelity host tests: all three options in one run, the dependency rules' messages word for word, and a step the
conversion has never heard of."""
import json

import pytest

from test_colour_host import ColourRenderBackend
from test_convert_host import _pngs, sbs_clips  # noqa: F401
from test_fidelity_host import FidelityRenderBackend
from test_source_parallax_host import SourceRenderBackend, _convert
from test_verify_host import VerifyRenderBackend, run  # noqa: F401

KEYS = ["frames", "fill_eyes", "q", "match", "verify", "fidelity"]


class AllRenderBackend(ColourRenderBackend, FidelityRenderBackend, VerifyRenderBackend):
    """the three stand-ins in the order of convert.HipRenderBackend: the colour match, the render and its verification, then the
    measurement of what was written; the keys of every call's source dict are kept"""

    def __init__(self):
        super().__init__()
        self.keys = []

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        self.keys.append(None if source is None else list(source))
        return super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)


def test_all_three_options_in_one_run(run, capsys):  # noqa: F811
    tmp, sbs, v4k, base = run
    flags = base + ["--match-colour", "clip", "--match-probes", "2", "--verify-source", "30"]
    runs = {}
    for name, extra in (("with", ["--fidelity-report"]), ("without", [])):
        (tmp / name).mkdir()
        capsys.readouterr()
        be = AllRenderBackend()
        assert _convert(flags + extra + ["--output", tmp / name / "o.json"], be) == 0
        text = (tmp / name / "o.json").read_text().replace(str(tmp / name), "<out>")
        runs[name] = be, json.loads(text), capsys.readouterr().out
    (be, man, text), (be0, man0, text0) = runs["with"], runs["without"]
    # the report changes no manifest key but its own, no PNG byte and not the table
    assert {k: v for k, v in man.items() if k != "fidelity_report"} == man0 and "fidelity_report" not in man0
    assert list(man)[-4:] == ["colour_probe_frames", "colour_lut", "verify_source", "fidelity_report"]
    assert _pngs(tmp / "with" / "o_frames") == _pngs(tmp / "without" / "o_frames") and "colour_lut.json" in _pngs(tmp / "with" / "o_frames")
    assert be.keys == [KEYS] * 2 and be0.keys == [KEYS[:-1]] * 2
    assert be.verified == be0.verified == [{"tau": 30}] * 2 and be.requests == [{"bad_thr": 48, "ceiling": True}] * 2
    assert all(m["mode"] == "clip" for m in be.matches) and ("table", 2) in be.colour and be0.requests == [None, None]
    entry = man["fidelity_report"]
    assert entry["path"] == "<out>/o_fidelity.json" and (tmp / "with" / "o_fidelity.json").is_file()
    assert sorted(entry["summary"]) == ["ceiling", "final", "warp"] and all(s is not None and s["frames"] == 5 for s in entry["summary"].values())
    assert text.count("Source verify:") == 1 == text0.count("Source verify:") and text.count("Fidelity report") == 1
    assert text.index("Colour match:") < text.index("Source verify:") < text.index("Fidelity report") and "Fidelity report" not in text0


# the refusals as the parent commit worded them: (the rules' keywords, the message of a run over clips, the NumPy surface's)
RULES = [
    (dict(fill_from_source="s.npy", parallax="invented"),
     "--fill-from-source needs --parallax source: the holes of an invented parallax do not line up with the real eye", None),
    (dict(fill_from_source=None, source_start_frame=2), "--source-start-frame needs --fill-from-source", None),
    (dict(fill_from_source=None, match_colour="clip"),
     "--match-colour needs --fill-from-source: it corrects the colours of the SBS clip's right eye, which only the source fill reads", None),
    (dict(fill_from_source="s.npy", match_probes=4),
     "--match-probes needs --match-colour clip: it counts the frame pairs the clip's one table is fitted to", None),
    (dict(fill_from_source="s.npy", match_colour="frame", match_probes=4),
     "--match-probes needs --match-colour clip: frame mode fits every batch to its own frames", None),
    (dict(fill_from_source=None, layout="full-sbs", verify_source=48),
     "--verify-source needs --fill-from-source: it checks the rendered right eye against the SBS clip's stored right eye, which only the source fill uploads",
     "--verify-source needs parallax='source' (--parallax source --fill-from-source): it checks the rendered right eye against the SBS clip's stored right eye, which only the source fill uploads"),
    (dict(fill_from_source="s.npy", layout="half-sbs", verify_source=48),
     "--verify-source works on the layouts full-sbs, full-tb, in which the right eye lies unpacked in the output; half-sbs squeezes, interleaves or mixes it", None),
    (dict(fill_from_source=None, layout="full-tb", fidelity_report=True),
     "--fidelity-report needs --fill-from-source: it measures the rendered right eye against the SBS clip's stored right eye, which only the source fill uploads",
     "--fidelity-report needs parallax='source' (--parallax source --fill-from-source): it measures the rendered right eye against the SBS clip's stored right eye, which only the source fill uploads"),
    (dict(fill_from_source="s.npy", layout="anaglyph-dubois", fidelity_report="r.json"),
     "--fidelity-report works on the layouts full-sbs, full-tb, in which the right eye lies unpacked in the output; anaglyph-dubois squeezes, interleaves or mixes it", None),
]


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("options,message,surface", RULES, ids=[" ".join(k for k in r[0] if k != "layout") for r in RULES])
def test_every_rule_in_both_wordings(options, message, surface, clip):
    from video_3d_pipeline.convert import check_source_rules, check_verify_source
    from video_3d_pipeline.fidelity import check_fidelity_report
    want = message if clip or surface is None else surface
    options = dict(options)
    fill = options.pop("fill_from_source")
    with pytest.raises(ValueError) as e:
        check_source_rules(fill, clip=clip, **options)
    assert str(e.value) == want
    # the two public names over it say the same
    thin = {"verify_source": lambda: check_verify_source(48, options["layout"], fill, clip),
            "fidelity_report": lambda: check_fidelity_report(options["layout"], fill, clip)}
    for key, call in thin.items():
        if key in options:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == want


def test_rules_pass_and_the_plan_and_the_cli_word_them_alike(run, capsys):  # noqa: F811
    from video_3d_pipeline.convert import StereoPlan, check_source_rules, check_verify_source
    assert check_source_rules("s.npy", layout="full-tb", source_start_frame=3, match_colour="clip", match_probes=4, verify_source=0,
                              fidelity_report=True) is None
    assert check_source_rules(None) is None and check_source_rules(None, layout="half-sbs") is None
    assert check_source_rules(True, layout="full-sbs", verify_source=48, clip=False) is None      # the plan: parallax == "source"
    assert check_verify_source(765, "full-sbs", "s.npy") == 765
    for kw, (_, _, surface) in ((dict(verify_source=48), RULES[5]), (dict(fidelity_report=True), RULES[7])):
        with pytest.raises(ValueError) as e:
            StereoPlan(**kw)
        assert str(e.value) == surface
    tmp, sbs, v4k, base = run
    for extra, (_, message, _) in ((["--verify-source"], RULES[5]), (["--fidelity-report"], RULES[7]), (["--source-start-frame", "2"], RULES[1])):
        assert _convert([v4k, tmp / "depth_f.json", "--parallax", "source", "--output", tmp / "o.json"] + extra, SourceRenderBackend()) == 1
        assert capsys.readouterr().out == f"Error: {message}\n"


def test_the_conversion_drives_a_step_it_does_not_know(run):  # noqa: F811
    from video_3d_pipeline.convert import DepthTo3DConverter
    from video_3d_pipeline.verify import SourceStep

    class Dummy(SourceStep):
        key, output_tag = "dummy", "_dm"

        def __init__(self):
            self.noted, self.prepared = [], 0

        def prepare(self, backend, plan, video_4k_path, guide_start, count, frame_size):
            self.prepared += 1

        def request(self):
            return {"n": self.prepared}

        def note(self, backend, indices, frame_size, q):
            self.noted.append((list(indices), tuple(frame_size), tuple(q)))

        def finish(self, output_path, frames_dir, world):
            return {"dummy_batches": len(self.noted)}, {frames_dir / "dummy.txt": "its side file"}

    class Recording(SourceRenderBackend):
        def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
            self.sources.append(source)
            return super().render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, subpixel, source)

    tmp, sbs, v4k, _ = run
    be, step = Recording(), Dummy()
    be.sources = []
    conv = DepthTo3DConverter(backend=be, parallax="source", fill_from_source=sbs, verify_source=None)
    conv.plan.steps.append(step)
    out = conv.process_conversion(v4k, str(tmp / "depth_f.json"), output_path=str(tmp / "d.json"))
    man = json.loads(open(out).read())
    assert step.prepared == 1 and [list(s) for s in be.sources] == [["frames", "fill_eyes", "q", "dummy"]] * 2
    assert all(s["dummy"] == {"n": 1} for s in be.sources)
    from test_convert_host import H4, W4
    assert step.noted == [([0, 1, 2, 3], (W4, H4), be.calls[0][2]), ([4], (W4, H4), be.calls[1][2])]
    assert man["dummy_batches"] == 2 and list(man)[-1] == "dummy_batches"
    assert (tmp / "d_frames" / "dummy.txt").read_text() == "its side file"
    plain = SourceRenderBackend()
    assert _convert([v4k, tmp / "depth_f.json", "--parallax", "source", "--fill-from-source", sbs, "--output", tmp / "p.json"], plain) == 0
    assert plain.calls == be.calls
    assert {k: v for k, v in _pngs(man["frames_dir"]).items() if k != "dummy.txt"} == _pngs(json.loads((tmp / "p.json").read_text())["frames_dir"])
    # its tag is in the default output's name, like the others'
    import os
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        assert os.path.basename(conv.process_conversion(v4k, str(tmp / "depth_f.json"), max_frames=1)) == "3d_full-sbs_srcpx_srcfill_dm_depth_f.mp4"
    finally:
        os.chdir(cwd)


def test_the_numpy_surface_asks_the_verifier_alone(run):  # noqa: F811
    """render_frame prepares no step: after a run with all three options its call carries the verify entry and is noted by the verifier,
    and neither the run's colour table nor a fidelity request goes with it"""
    from test_convert_host import _read_clip
    from video_3d_pipeline.convert import DepthTo3DConverter
    from video_3d_pipeline.utils import read_png16
    tmp, sbs, v4k, _ = run
    be = AllRenderBackend()
    conv = DepthTo3DConverter(backend=be, parallax="source", fill_from_source=sbs, match_colour="frame", verify_source=40, fidelity_report=True)
    conv.process_conversion(v4k, str(tmp / "depth_f.json"), output_path=str(tmp / "s.json"))
    assert be.keys == [KEYS] * 2 and be.asked == 4 and len(conv.plan.steps[1].shares) == 5      # the counts and the records, per batch
    d = read_png16(json.loads((tmp / "depth_f.json").read_text())["frames_dir"] + "/depth4k_000000.png")
    conv.render_frame(_read_clip(v4k)[0], d, source=_read_clip(sbs)[0])
    assert be.keys[-1] == ["frames", "fill_eyes", "q", "verify"] and be.requests[-1] is None and be.matches[-1] is None
    assert be.asked == 5 and len(conv.plan.steps[1].shares) == 6
