"""The host side of --verify-source: where the matcher's disparity was wrong the warp shows wrong picture content, and the film's
stored right eye says so (v3d_verify_eye_source_batch; contract: tests/verify_ref.py).  And what the convert step's four source-eye
options share: colour.ColourMatcher, SourceVerifier, SourceFuser and fidelity.FidelityMonitor are the SourceSteps of StereoPlan.steps,
which is all the conversion knows of them, and check_source_rules holds what they need of the other flags.  --fuse-source
(SourceFuser; v3d_fuse_eye_source_batch; contract: tests/fuse_ref.py) then takes the right eye's low band from the stored eye."""
import numpy as np

# --verify-source: the threshold's default and range (mean absolute difference of a cell's channel sums per pixel, the three channels
# added: 0 .. 765).  48 is a convention exposed as a flag, like the matcher's min_score: not a film measurement
DEFAULT_VERIFY_TAU, VERIFY_TAU_MAX = 48, 765
VERIFY_LAYOUTS = ("full-sbs", "full-tb")       # the packings in which the right eye lies unpacked in the output
VERIFY_WARN_SHARE = 0.25


class SourceStep:
    """What the conversion asks of a source-eye option.  key: its entry in a render call's `source` dict, request(): its value;
    output_tag: its suffix in the default output name; cached_note: printed when an existing output is used instead; on_surface:
    DepthTo3DConverter.render_frame, which prepares nothing, asks it too.
    check_map(q): when a render call's map is known, before the call: ValueError for a map the step cannot work under;
    prepare(backend, plan, video_4k_path, guide_start, count, frame_size): before the render loop, on every rank;
    note(backend, indices, frame_size, q): after a render call that carried the request (the batch's clip frames, the call's map);
    finish(output_path, frames_dir, world): after the last frame and the barrier; prints its summary -> (its manifest entries, its
    side files {path: text}, which rank 0 writes)"""
    key, output_tag, cached_note, on_surface = None, "", None, False

    def check_map(self, q):
        pass


def check_source_rules(fill_from_source, *, parallax="source", layout=None, source_start_frame=0, match_colour=None, match_probes=None,
                       verify_source=None, fidelity_report=None, fuse_source=None, clip: bool = True):
    """Every "X needs Y" rule of the source-eye options, for the options handed over (a default: off, or not this caller's to check).
    clip: a run over clips, which needs the SBS clip's path (the NumPy surface gets the SBS frame per call: its parallax="source")"""
    if fill_from_source is not None and parallax != "source":
        raise ValueError("--fill-from-source needs --parallax source: the holes of an invented parallax do not line up with the real eye")
    if source_start_frame and not fill_from_source:
        raise ValueError("--source-start-frame needs --fill-from-source")
    if match_colour is None and match_probes is not None:
        raise ValueError("--match-probes needs --match-colour clip: it counts the frame pairs the clip's one table is fitted to")
    if match_colour is not None and fill_from_source is None:
        raise ValueError("--match-colour needs --fill-from-source: it corrects the colours of the SBS clip's right eye, which only the source fill reads")
    if match_colour not in (None, "clip") and match_probes is not None:
        raise ValueError("--match-probes needs --match-colour clip: frame mode fits every batch to its own frames")
    needs = "--fill-from-source" if clip else "parallax='source' (--parallax source --fill-from-source)"
    for flag, verb, value in (("--verify-source", "checks the rendered right eye against", verify_source),
                              ("--fidelity-report", "measures the rendered right eye against", fidelity_report),
                              ("--fuse-source", "fuses the rendered right eye with", fuse_source or None)):
        if value is not None and not fill_from_source:
            raise ValueError(f"{flag} needs {needs}: it {verb} the SBS clip's stored right eye, which only the source fill uploads")
        if value is not None and layout not in VERIFY_LAYOUTS:
            raise ValueError(f"{flag} works on the layouts {', '.join(VERIFY_LAYOUTS)}, in which the right eye lies unpacked in "
                             f"the output; {layout} squeezes, interleaves or mixes it")


def check_verify_source(tau, layout, fill_from_source, clip: bool = True):
    """--verify-source TAU against its range and the flags it depends on -> tau as an int; ValueError otherwise"""
    if isinstance(tau, bool) or not isinstance(tau, (int, np.integer)) or not 0 <= tau <= VERIFY_TAU_MAX:
        raise ValueError(f"--verify-source takes an integer threshold in [0, {VERIFY_TAU_MAX}], got {tau!r}")
    check_source_rules(fill_from_source, layout=layout, verify_source=tau, clip=clip)
    return int(tau)


class SourceVerifier(SourceStep):
    """--verify-source: the render calls' source entry gains verify=dict(tau), and note adds up what the backend counted"""
    key, on_surface = "verify", True

    def __init__(self, tau: int):
        self.tau, self.output_tag = tau, f"_vs{tau}"
        self.shares = []                    # replaced cells / cells of every verified frame this process rendered
        self.cell = (None, None)            # known after the first batch

    def prepare(self, backend, plan, video_4k_path, guide_start, count, frame_size):
        check_verify_source(self.tau, plan.params["layout"], plan.fill_from_source)      # a run over clips: now the SBS clip has to be there

    def request(self):
        return dict(tau=self.tau)

    def note(self, backend, indices, frame_size, q):
        """the backend's replaced cells per frame -> shares of the frame's cells"""
        from ._native import verify_cell
        counts = backend.verify_counts()
        if counts is None:
            raise RuntimeError("--verify-source: the backend rendered without verifying")
        cx, cy = verify_cell(q[0], q[2])
        cells = -(-frame_size[0] // cx) * -(-frame_size[1] // cy)
        self.cell = (cx, cy)
        self.shares += [int(c) / cells for c in counts]

    def finish(self, output_path, frames_dir, world):
        """the manifest's verify_source block; the shares are this process's own, so null under torchrun"""
        alone = world == 1 and bool(self.shares)
        rec = {"tau": self.tau, "cell": list(self.cell),
               "replaced_share": float(np.mean(self.shares)) if alone else None,
               "replaced_share_max": float(np.max(self.shares)) if alone else None}
        if rec["replaced_share"] is not None:
            print(f"Source verify: tau {rec['tau']}, cells of {rec['cell'][0]} x {rec['cell'][1]} pixels: "
                  f"{rec['replaced_share']:.2%} of the right eye's cells replaced on average, {rec['replaced_share_max']:.2%} at most")
            if rec["replaced_share"] > VERIFY_WARN_SHARE:
                print(f"Warning: --verify-source replaced {rec['replaced_share']:.0%} of the right eye: the SBS clip disagrees with "
                      f"the render almost everywhere, as another grading or another framing makes it.  Try --match-colour, or a "
                      f"depth run whose map came from `align --register-spatial`")
        return {"verify_source": rec}, {}


FUSE_SCALE_MAX = 65536                         # Q16: one stored sample per pixel at most


def check_fuse_source(layout, fill_from_source, clip: bool = True):
    """--fuse-source against the flags it depends on; ValueError otherwise"""
    check_source_rules(fill_from_source, layout=layout, fuse_source=True, clip=clip)


class SourceFuser(SourceStep):
    """--fuse-source: the render calls' source entry gains fuse={}, and the right eye leaves the backend as E - LP(E) + P: its low
    band from the stored eye, its detail above the stored eye's resolution from the render (and the verification)"""
    key, on_surface, output_tag = "fuse", True, "_fu"

    def __init__(self):
        self.scales = None                  # stored samples per pixel (x, y), known after the first batch

    def prepare(self, backend, plan, video_4k_path, guide_start, count, frame_size):
        from . import sharding
        check_fuse_source(plan.params["layout"], plan.fill_from_source)
        if plan.match_colour is None and sharding.rank_world()[0] == 0:
            print("Source fuse: without --match-colour the right eye's low band now carries the SBS release's grading")

    def check_map(self, q):
        if q[0] > FUSE_SCALE_MAX or q[2] > FUSE_SCALE_MAX:
            raise ValueError(f"--fuse-source: the map has {q[0] / 65536:g} x {q[2] / 65536:g} stored samples per pixel, more than one: "
                             f"the stored eye is finer than the frame and fusing has nothing to add")

    def request(self):
        return {}

    def note(self, backend, indices, frame_size, q):
        self.scales = [q[0] / 65536, q[2] / 65536]

    def finish(self, output_path, frames_dir, world):
        if self.scales is not None:
            print(f"Source fuse: the right eye's low band from the stored eye, {self.scales[0]:g} x {self.scales[1]:g} stored samples per pixel")
        return {"fuse_source": {"samples_per_pixel": self.scales}}, {}
