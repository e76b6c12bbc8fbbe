"""Colour matching for --fill-from-source (the convert CLI's --match-colour).

The SBS clip whose right eye fills the disocclusions comes from another release than the 4K frame around the holes: another
grading, another tone mapping, another black level.  Its LEFT eye and the 4K frame show the same view, so a per-channel transfer
curve is fitted left eye -> 4K frame by exact histogram matching (v3d_bgr_hist_batch twice, v3d_colour_lut_batch) and applied to the
RIGHT eye (v3d_bgr_lut_batch, in place on the uploaded SBS frames) before v3d_render_stereo_source_batch samples it.  The fit needs
no depth and no render.  Bit-exact contract: tests/colour_ref.py.

    clip   one table for the whole run, from `probes` frame pairs spread over the frames that will be rendered; every rank of a
           torchrun job reads the same probes and builds the same table, and one table cannot flicker
    frame  every render batch fits one table per frame to its own frames: for clips whose grading difference changes from scene to
           scene; neighbouring frames get slightly different tables, which can show as flicker in the filled regions
"""
import json
from fractions import Fraction

import numpy as np

from .verify import SourceStep

MODES = ("clip", "frame")
DEFAULT_PROBES = 16
PROBE_BATCH = 4                     # probe pairs per upload: the render loop's own staging size


def check_parameters(mode, probes):
    if mode not in MODES:
        raise ValueError(f"--match-colour must be one of {MODES}, got {mode!r}")
    if isinstance(probes, bool) or not isinstance(probes, (int, np.integer)) or not 1 <= probes <= 64:
        raise ValueError(f"--match-probes must be an integer in [1, 64], got {probes!r}")


def _axis(A, B, n_eye: int, n_frame: int):
    """one axis of the applied spatial map, s = A u + B between normalised frame and eye coordinates -> ((eye lo, hi), (frame lo,
    hi)) in pixels, both rounded inward"""
    A, B = Fraction(A), Fraction(B)
    if A <= 0:
        raise ValueError(f"spatial map scale {float(A):g} is not positive")
    u0, u1 = max(Fraction(0), -B / A), min(Fraction(1), (1 - B) / A)         # the frame's part whose image lies inside the eye
    s0, s1 = A * u0 + B, A * u1 + B                                          # the eye's part that it covers
    ceil = lambda q: -((-q).__floor__())
    return (ceil(s0 * n_eye), (s1 * n_eye).__floor__()), (ceil(u0 * n_frame), (u1 * n_frame).__floor__())


def common_rects(spatial_map, eye_size, frame_size):
    """-> (eye_rect, frame_rect), each (x0, y0, x1, y1): the part of the 4K frame whose image lies inside the SBS clip's eye and the
    part of the eye it covers, under the spatial map (Ax, Bx, Ay, By) the depth run applied (eye = A frame + B in normalised plane
    coordinates); None = the whole eye against the whole frame.  The eye is the LEFT half of the stored SBS frame, so eye_rect is a
    rectangle of that frame as it stands; a squeezed eye needs no special case (a histogram does not care about resolution).
    ValueError when the two do not overlap by a pixel."""
    (We, He), (Wf, Hf) = eye_size, frame_size
    Ax, Bx, Ay, By = spatial_map if spatial_map is not None else (1, 0, 1, 0)
    (ex0, ex1), (fx0, fx1) = _axis(Ax, Bx, int(We), int(Wf))
    (ey0, ey1), (fy0, fy1) = _axis(Ay, By, int(He), int(Hf))
    eye, frame = (ex0, ey0, ex1, ey1), (fx0, fy0, fx1, fy1)
    for name, (x0, y0, x1, y1) in (("eye", eye), ("4K frame", frame)):
        if x0 >= x1 or y0 >= y1:
            raise ValueError(f"--match-colour: the spatial map {tuple(float(v) for v in (Ax, Bx, Ay, By))} leaves no common part of the "
                             f"{name} ({We}x{He} eye, {Wf}x{Hf} frame)")
    return eye, frame


class ColourMatcher(SourceStep):
    """--match-colour of the convert CLI.  The backend supplies colour_probe(sbs_frames, frames, eye_rect, frame_rect) -> histograms
    and colour_table(list of them) -> (the table where the render wants it, its NumPy copy u8 [3,256])"""
    key = "match"

    def __init__(self, mode: str, probes: int = DEFAULT_PROBES):
        check_parameters(mode, probes)
        self.mode, self.probes, self.output_tag = mode, int(probes), {"clip": "_cm", "frame": "_cmf"}[mode]
        self.eye_rect = self.frame_rect = self.table = self.table_np = None
        self.probe_frames = []

    def prepare(self, backend, plan, video_path, guide_start, count, frame_size):
        """the two rectangles; in clip mode the probe pass and the table (depth frame i: SBS frame source_start_frame + i, 4K frame guide_start + i)"""
        from .framematch import probe_starts
        from .utils import get_video_info, iter_frames
        sbs_path, source_start, src_info = plan.fill_from_source, plan.source_start_frame, get_video_info(plan.fill_from_source)
        self.eye_rect, self.frame_rect = common_rects(plan.spatial_map, (src_info['width'] // 2, src_info['height']), frame_size)
        if self.mode != "clip":
            return
        self.probe_frames, _ = probe_starts(int(count), 1, self.probes)
        hists = []
        for k in range(0, len(self.probe_frames), PROBE_BATCH):
            idx = self.probe_frames[k:k + PROBE_BATCH]
            sbs = [next(iter_frames(sbs_path, source_start + i, 1), None) for i in idx]
            v4k = [next(iter_frames(video_path, guide_start + i, 1), None) for i in idx]
            if any(f is None for f in sbs + v4k):
                raise ValueError(f"--match-colour: a probe frame among {idx} could not be read from {sbs_path} / {video_path}")
            hists.append(backend.colour_probe(sbs, v4k, self.eye_rect, self.frame_rect))
        self.table, self.table_np = backend.colour_table(hists)
        print(f"Colour match: one table from {len(self.probe_frames)} frame pairs")

    def request(self):
        """the mode, the clip table (None in frame mode) and the two rectangles"""
        return dict(mode=self.mode, table=self.table, eye_rect=self.eye_rect, frame_rect=self.frame_rect)

    def note(self, backend, indices, frame_size, q):
        """the render applied the table: nothing comes back"""

    def finish(self, output_path, frames_dir, world):
        """clip mode: the probe frames and colour_lut.json"""
        if self.mode != "clip":
            return {"match_colour": self.mode}, {}
        probes, path = [int(i) for i in self.probe_frames], frames_dir / "colour_lut.json"
        lut = {"channels": "BGR", "eye_rect": list(self.eye_rect), "frame_rect": list(self.frame_rect), "probe_frames": probes,
               "lut": np.asarray(self.table_np).reshape(3, 256).astype(int).tolist()}
        return {"match_colour": self.mode, "colour_probe_frames": probes, "colour_lut": str(path)}, {path: json.dumps(lut)}
