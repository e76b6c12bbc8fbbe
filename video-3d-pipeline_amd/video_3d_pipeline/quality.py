"""Stereo quality report (opt-in: `--quality-report [PATH]`): two measures of a run's own depth that need no ground truth.

Every stage that changes the depth is optional (`--fill-holes`, `--temporal-radius`, `--range-percentile`, the hybrid blend), and a
real 3D release has no ground truth to judge a setting against.  While a depth pass is resident the device holds what two
ground-truth-free measures need, and this module reads them there:

  * reprojection error: how well the right view, pulled back through the matcher's int16 disparity, explains the left view --
    next to the same pixels at disparity 0, the baseline a useless disparity would reach;
  * flicker: how far the fixed-point depth of pixels whose luma stood still moves from one frame to the next -- of the depth the
    pass hands on ("matched") and, with `--temporal-radius`, of the filtered depth ("stabilised").

Both are integer sums over pixels with a bit-exact contract (include/v3d_hip.h; tests/quality_ref.py restates it).  The report
changes no output byte, adds no cache suffix and no synchronisation point: records are enqueued with the pass, copied to pinned
memory without blocking and read only once their event has fired (the pass's own synchronise sees to that), the rest at the end.

Populations matter: a stage that fills invalid pixels (`--temporal-radius` with its fill on, `--fill-holes`) adds pixels to
`n_still` / `n_valid`, and the new pixels may move more than the old ones.  Every sum is therefore reported next to its
population, and two settings compare only where the populations are equal.
"""
import json
import math
from collections import deque
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from .temporal import DEFAULT_CUT

REPROJ_FIELDS = ("n_valid", "n_cmp", "sad", "ssd", "n_bad", "sad0", "ssd0", "n_bad0")
FLICKER_FIELDS = ("luma_sad", "n_still", "flicker", "n_jump")
DEFAULT_BAD, DEFAULT_STILL, DEFAULT_JUMP = 16, 4, 1.0      # conventions, not measurements: gray levels, gray levels, pixels
SHARDED_REASON = "flicker needs consecutive frames; a sharded run (world > 1) gives a rank no complete sequence"
CACHED_NOTE = "Quality report: none was made, the existing output was used; --force recomputes"


def check_parameters(bad_threshold=DEFAULT_BAD, still=DEFAULT_STILL, jump=DEFAULT_JUMP, cut_threshold=DEFAULT_CUT):
    """validated (bad_threshold, still, jump16, cut_threshold): gray levels in [0, 255] twice, the jump in 1/16 px in [0, 32767]
    from a finite number of pixels that is a multiple of 1/16, the temporal stage's cut threshold in [0, 256]"""
    for name, v, hi in (("quality bad threshold", bad_threshold, 255), ("quality still threshold", still, 255), ("quality cut threshold", cut_threshold, 256)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not 0 <= v <= hi:
            raise ValueError(f"{name} must be an integer in [0, {hi}], got {v!r}")
    if isinstance(jump, (bool, np.bool_)) or not isinstance(jump, (int, float, np.integer, np.floating)) or not math.isfinite(jump):
        raise ValueError(f"quality jump must be a finite number of pixels, got {jump!r}")
    j16 = round(jump * 16)
    if abs(jump * 16 - j16) > 1e-6 or not 0 <= j16 <= 32767:
        raise ValueError(f"quality jump must be a multiple of 1/16 px in [0, 2047.9375], got {jump!r}")
    return int(bad_threshold), int(still), int(j16), int(cut_threshold)


def reproj_summary(t: Dict[str, int], pixels: int) -> Dict:
    """totals of the reprojection records -> the figures of the report, in gray levels (None where nothing was compared)"""
    n = t["n_cmp"]
    f = lambda num: None if n == 0 else num / n
    rms = lambda ssd: None if n == 0 else math.sqrt(ssd / n) / 16
    return dict(valid_share=None if pixels == 0 else t["n_valid"] / pixels, compared_share=None if pixels == 0 else n / pixels,
                mean_abs_error=None if n == 0 else t["sad"] / n / 16, mean_abs_error_d0=None if n == 0 else t["sad0"] / n / 16,
                rms_error=rms(t["ssd"]), rms_error_d0=rms(t["ssd0"]), bad_share=f(t["n_bad"]), bad_share_d0=f(t["n_bad0"]))


class _FlickerSeries:
    """one sequence of consecutive frames fed a pass at a time: the pass's own pairs in one call, the pair that bridges two passes
    from a private copy of the previous pass's last depth and gray plane"""

    def __init__(self, monitor, name):
        self.m, self.name = monitor, name
        self.carry = None                    # (depth [1,H,W], gray [1,H,W], clip index of that frame)
        self.records: List = []              # (clip index of the pair's second frame, int64 [4])

    def push(self, first_index, depth, gray):
        be, m = self.m.backend, self.m
        n = len(depth)
        if n == 0:
            return
        if self.carry is not None:
            d2, g2 = be.temporal_concat(self.carry[0], depth[:1]), be.temporal_concat(self.carry[1], gray[:1])
            m._enqueue(be.quality_flicker(d2, g2, m.still, m.jump16), self.records, [first_index])
        if n > 1:
            m._enqueue(be.quality_flicker(depth, gray, m.still, m.jump16), self.records, list(range(first_index + 1, first_index + n)))
        self.carry = (be.temporal_concat(None, depth[n - 1:]), be.temporal_concat(None, gray[n - 1:]), first_index + n - 1)

    def totals(self, cut_limit):
        rec = sorted(self.records, key=lambda r: r[0])
        cuts = [i for i, r in rec if int(r[0]) > cut_limit]
        t = {k: int(sum(int(r[j]) for i, r in rec if int(r[0]) <= cut_limit)) for j, k in enumerate(FLICKER_FIELDS)}
        pairs = [dict(frame=int(i), cut=int(r[0]) > cut_limit, **{k: int(v) for k, v in zip(FLICKER_FIELDS, r)}) for i, r in rec]
        mean = None if t["n_still"] == 0 else t["flicker"] / t["n_still"] / 16
        return dict(pairs=len(rec), cuts=len(cuts), cut_frames=cuts, totals=t, mean_px_per_frame=mean,
                    jump_share=None if t["n_still"] == 0 else t["n_jump"] / t["n_still"]), pairs


class QualityMonitor:
    """--quality-report of the depth CLI and the one-pass pipeline.  The driver (HybridStereoDepthExtractor.iter_depth_u16) calls
    note_pass() right after a disparity pass, while the pass's planes are valid; with --temporal-radius the stabiliser's `observe`
    hook calls note_stabilised() with the filtered depth.  Nothing here waits for the device before finish().  The backend supplies
    left_gray(n), temporal_concat(held, new), quality_reproj(n, bad_thr), quality_flicker(depth, gray, still, jump16),
    quality_fetch(records) and read_quality(handle, wait)."""

    def __init__(self, backend, bad_threshold: int = DEFAULT_BAD, still: int = DEFAULT_STILL, jump: float = DEFAULT_JUMP,
                 cut_threshold: int = DEFAULT_CUT, consecutive: bool = True, reproj_stage: str = "matcher", flicker_stage: str = "matcher",
                 owned: Optional[range] = None, min_disparity: int = 0):
        """consecutive: the frames arrive in clip order without gaps (one process); False switches flicker off (a sharded run).
        owned: the clip frames whose reprojection records count (a rank's block without its halo); None = all
        min_disparity m != 0 (--min-disparity): the pass's disparity is rebiased by -16 m; the backend's quality_reproj is told, and
        the "disparity 0" figures of the record are the hypothesis d = m (reported as baseline_disparity)"""
        self.min_disparity = int(min_disparity)
        self.bad_threshold, self.still, self.jump16, self.cut_threshold = check_parameters(bad_threshold, still, jump, cut_threshold)
        self.backend, self.consecutive = backend, bool(consecutive)
        self.reproj_stage, self.flicker_stage, self.owned = reproj_stage, flicker_stage, owned
        self.frames: List = []               # (clip frame, int64 [8])
        self.matched = _FlickerSeries(self, "matched")
        self.stabilised = None               # created by the first note_stabilised()
        self._stab_next = None
        self._pending = deque()
        self.shape = None
        self.summary = self.report_data = None

    # ---- fed by the driver ----
    def _enqueue(self, records, sink, indices):
        self._pending.append((self.backend.quality_fetch(records), sink, indices))

    def _drain(self, wait):
        while self._pending:
            handle, sink, indices = self._pending[0]
            rec = self.backend.read_quality(handle, wait)
            if rec is None:
                return
            self._pending.popleft()
            sink.extend((i, np.asarray(r, np.int64)) for i, r in zip(indices, rec) if sink is not self.frames or self.owned is None or i in self.owned)

    def note_pass(self, indices, n, depth):
        """indices: the clip frames of the pass, n of them; depth: what the pass hands on, [n,H,W]"""
        self._drain(False)                   # earlier passes: their events fired with the consumer's own synchronise
        be = self.backend
        self.shape = tuple(int(v) for v in depth.shape[1:])
        window = {"min_disparity": self.min_disparity} if self.min_disparity else {}
        self._enqueue(be.quality_reproj(n, self.bad_threshold, **window), self.frames, list(indices))
        if self.consecutive:
            self.matched.push(indices[0], depth[:n], be.left_gray(n))

    def note_stabilised(self, depth, gray):
        """the temporal stabiliser's observe hook: the filtered depth of the next targets and their left gray, in clip order"""
        if not self.consecutive:
            return
        if self.stabilised is None:
            self.stabilised, self._stab_next = _FlickerSeries(self, "stabilised"), (self.owned[0] if self.owned else 0)
        self.stabilised.push(self._stab_next, depth, gray)
        self._stab_next += len(depth)

    # ---- the report ----
    def finish(self, total=lambda v: v) -> Dict:
        """the summary (also kept in .summary; .report_data holds the whole quality.json): reprojection totals summed over the
        ranks by `total`, flicker this process's (None with a reason in a sharded run)"""
        self._drain(True)
        frames = sorted(self.frames, key=lambda r: r[0])
        tot = {k: int(total(int(sum(int(r[j]) for _, r in frames)))) for j, k in enumerate(REPROJ_FIELDS)}
        n_frames = int(total(len(frames)))
        H, W = self.shape if self.shape else (0, 0)
        params = dict(bad_threshold=self.bad_threshold, still=self.still, jump=self.jump16 / 16, jump16=self.jump16, cut_threshold=self.cut_threshold)
        reproj = dict(frames=n_frames, totals=tot, **reproj_summary(tot, n_frames * W * H))
        self.summary = dict(parameters=params, reproj_stage=self.reproj_stage, flicker_stage=self.flicker_stage, reproj=reproj)
        if self.min_disparity:
            self.summary["baseline_disparity"] = self.min_disparity
        data = dict(self.summary, width=W, height=H, units=dict(error="1/16 gray level", flicker="1/16 px"),
                    frames=[dict(frame=int(i), **{k: int(v) for k, v in zip(REPROJ_FIELDS, r)}) for i, r in frames])
        if not self.consecutive:
            self.summary["flicker"] = data["flicker"] = None
            self.summary["flicker_reason"] = data["flicker_reason"] = SHARDED_REASON
        else:
            limit, fl, pairs = self.cut_threshold * W * H, {}, {}
            for s in (self.matched, self.stabilised):
                if s is not None:
                    fl[s.name], pairs[s.name] = s.totals(limit)
            self.summary["flicker"] = data["flicker"] = fl
            data["pairs"] = pairs
        self.report_data = data
        return self.summary

    def report(self):
        s, r = self.summary, self.summary["reproj"]
        pct = lambda v: "n/a" if v is None else f"{100 * v:.2f} %"
        num = lambda v: "n/a" if v is None else f"{v:.3f}"
        print(f"Quality report ({r['frames']} frames, disparity of the {s['reproj_stage']}):")
        if self.min_disparity:
            print(f"  search window [{self.min_disparity}, {self.min_disparity + 64}): \"disparity 0\" below reads disparity {self.min_disparity} "
                  f"(baseline_disparity), compared over the {-self.min_disparity} columns narrower left view")
        print(f"  valid {pct(r['valid_share'])} of the pixels, compared {pct(r['compared_share'])}")
        print(f"  reprojection error: mean abs {num(r['mean_abs_error'])} levels (disparity 0: {num(r['mean_abs_error_d0'])}), "
              f"RMS {num(r['rms_error'])} (disparity 0: {num(r['rms_error_d0'])}), above {self.bad_threshold} levels {pct(r['bad_share'])} "
              f"(disparity 0: {pct(r['bad_share_d0'])})")
        if s["flicker"] is None:
            print(f"  flicker: not reported ({s['flicker_reason']})")
            return
        for name, f in s["flicker"].items():
            print(f"  flicker, {name}: {num(f['mean_px_per_frame'])} px/frame over {f['totals']['n_still']} still pixels of {f['pairs'] - f['cuts']} pairs "
                  f"(jumps above {self.jump16 / 16:g} px: {pct(f['jump_share'])}), {f['cuts']} scene cuts skipped")

    def write(self, path) -> Path:
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(self.report_data, indent=1))
        return path


def add_quality_arguments(parser):
    """the CLI surface shared by the depth CLI and the one-pass pipeline"""
    parser.add_argument('--quality-report', nargs='?', const=True, default=None, metavar='PATH',
                        help='Measure the depth of this run on the GPU without ground truth -- reprojection error of the disparity '
                             'against disparity 0, depth flicker of still pixels -- print a summary and write quality.json next to the '
                             'depth maps (or to PATH).  No output changes')
    parser.add_argument('--quality-bad-threshold', type=int, default=DEFAULT_BAD,
                        help=f'Reprojection error (gray levels) above which a pixel counts as bad (default {DEFAULT_BAD})')
    parser.add_argument('--quality-still', type=int, default=DEFAULT_STILL,
                        help=f'Largest luma change (gray levels) between two frames at which a pixel counts as still (default {DEFAULT_STILL})')
    parser.add_argument('--quality-jump', type=float, default=DEFAULT_JUMP,
                        help=f'Depth change (pixels of disparity, a multiple of 1/16) of a still pixel that counts as a jump (default {DEFAULT_JUMP:g})')


def quality_options(args) -> dict:
    """parsed arguments -> the constructors' keyword arguments"""
    return dict(quality_report=args.quality_report, quality_bad_threshold=args.quality_bad_threshold, quality_still=args.quality_still,
                quality_jump=args.quality_jump)
