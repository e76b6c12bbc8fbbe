"""Rendered-eye fidelity report (opt-in: `convert --fidelity-report [PATH]`): how close a run's rendered eyes are to the film's own.

Every stage between the depth and the right eye is optional and has knobs (`--parallax-gain`, `--min-disparity`, `--temporal-radius`,
`--subpixel`, `--match-colour`, `--verify-source TAU`, ...), and `--quality-report` only judges the depth.  A `--fill-from-source`
run has the ground truth for the picture on the device anyway: the stored eyes of the SBS frame.  This module measures against them,
per frame, three series:

  * warp:    the right eye rendered with background fill only (no source samples, no verification), into a scratch output -- the
             honest figure for depth + DIBR, since fill and verification copy the truth into the picture;
  * final:   the right eye as written (it contains source samples wherever the fill or the verification put them);
  * ceiling: the output's left eye against the stored LEFT eye, when the left eye is the 4K frame itself (left gain 0): how far
             the two releases differ in resolution, grading, compression and registration.  No render can be expected to beat it.

A record is six integers with a bit-exact contract (include/v3d_hip.h, v3d_eye_fidelity_batch; tests/fidelity_ref.py restates it):
error sums of the cell means (a cell: the targets one stored sample spans -- the comparison happens at the stored eye's resolution,
which is all the information that eye holds) and the sum of the SSIM of 8 x 8-cell windows of the cells' luma in Q20.  The report
changes no output byte, adds no cache suffix and no synchronisation point: records are enqueued with the render, copied to pinned
memory without blocking and read once their event has fired (the batch's own copy back sees to that), the rest at the end.
"""
import json
import math
from collections import deque
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from .verify import VERIFY_LAYOUTS as LAYOUTS, SourceStep, check_source_rules

FIELDS = ("n_cells", "sad", "ssd", "n_bad", "n_win", "ssim_q20")
SERIES = ("warp", "final", "ceiling")
DEFAULT_BAD, BAD_MAX = 48, 765               # a convention (--verify-source's default threshold), not a measurement: levels, B + G + R
SSIM_ONE = 1 << 20
WORST_FRAMES = 10
SHARDED_REASON = "the records are a rank's own; a sharded run (world > 1) gives no rank the whole clip"
CEILING_REASON = "the left eye is rendered (left gain != 0): it is not the 4K frame, so it says nothing about the two releases"
CACHED_NOTE = "Fidelity report: none was made, the existing output was used; --force recomputes"


def check_parameters(bad_threshold=DEFAULT_BAD):
    """validated bad threshold: the sum over the three channels of a cell's mean differences above which it counts as bad"""
    v = bad_threshold
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or not 0 <= v <= BAD_MAX:
        raise ValueError(f"fidelity bad threshold must be an integer in [0, {BAD_MAX}], got {v!r}")
    return int(v)


def check_fidelity_report(layout, fill_from_source, clip: bool = True):
    """--fidelity-report against the flags it depends on; ValueError otherwise"""
    check_source_rules(fill_from_source, layout=layout, fidelity_report=True, clip=clip)


def figures(t: Dict[str, int]) -> Dict:
    """the six sums of a frame or of a clip -> mean_abs (levels per channel), psnr (dB of the cell means: inf when no cell
    differs), bad_share, ssim (the mean over the windows); None where there is nothing to divide by"""
    n, nw = t["n_cells"], t["n_win"]
    if n == 0:
        return dict(mean_abs=None, psnr=None, bad_share=None, ssim=None)
    mse = t["ssd"] / (3 * n)
    return dict(mean_abs=t["sad"] / (3 * n), psnr=math.inf if t["ssd"] == 0 else 10 * math.log10(255 * 255 / mse),
                bad_share=t["n_bad"] / n, ssim=None if nw == 0 else t["ssim_q20"] / SSIM_ONE / nw)


def series_summary(records) -> Dict:
    """[(frame, int64 [6])] of one series -> its clip-level block: totals, their figures, the ten worst frames by SSIM"""
    rec = sorted(records, key=lambda r: r[0])
    tot = {k: int(sum(int(r[j]) for _, r in rec)) for j, k in enumerate(FIELDS)}
    per = [(int(i), figures(dict(zip(FIELDS, (int(v) for v in r))))) for i, r in rec]
    worst = sorted((f for f in per if f[1]["ssim"] is not None), key=lambda f: (f[1]["ssim"], f[0]))[:WORST_FRAMES]
    return dict(frames=len(rec), totals=tot, **figures(tot), worst_frames=[dict(frame=i, ssim=f["ssim"], psnr=f["psnr"]) for i, f in worst])


def summary(records: Dict[str, Optional[List]]) -> Dict:
    """{series: [(frame, int64 [6])] or None} -> {"series": clip-level blocks, "frames": per-frame sums and figures}"""
    out, frames = {}, {}
    for name in SERIES:
        rec = records.get(name)
        if rec is None:
            out[name] = None
            continue
        out[name] = series_summary(rec)
        for i, r in rec:
            t = dict(zip(FIELDS, (int(v) for v in r)))
            frames.setdefault(int(i), {"frame": int(i)})[name] = dict(t, **figures(t))
    if out.get("final") is not None:
        out["final"]["contains_source_samples"] = True
    return dict(series=out, frames=[frames[i] for i in sorted(frames)])


def _jsonable(v):
    """inf (the PSNR of identical cell means) has no JSON spelling: it is written as the string "inf" """
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    return "inf" if isinstance(v, float) and math.isinf(v) else v


class FidelityMonitor(SourceStep):
    """--fidelity-report of the convert CLI.  Nothing here waits for the device before finish().  The backend supplies
    fidelity_handle() (the records of its last render_batch, on their way to pinned memory) and read_fidelity(handle, wait)."""
    key, cached_note = "fidelity", CACHED_NOTE

    def __init__(self, bad_threshold: int = DEFAULT_BAD, ceiling: bool = True, path=True):
        self.bad_threshold, self.ceiling, self.path = check_parameters(bad_threshold), bool(ceiling), path
        self.records, self._pending = {}, deque()        # {series: [(frame, int64 [6])]}, the ceiling's only when it is measured
        self.shape = self.cell = self.data = None

    def prepare(self, backend, plan, video_4k_path, guide_start, count, frame_size):
        check_fidelity_report(plan.params["layout"], plan.fill_from_source)      # a run over clips: now the SBS clip has to be there
        # a run's own records; the ceiling series only when the left eye is the 4K frame itself, known once the gains are
        self.ceiling, self.records, self._pending = plan.gains[0] == 0, {}, deque()

    def request(self) -> Dict:
        """the `fidelity` entry of a render call's source dict"""
        return dict(bad_thr=self.bad_threshold, ceiling=self.ceiling)

    def note(self, backend, indices, frame_size, q):
        """after a render call that carried request(): indices = the clip frames of the batch"""
        from ._native import verify_cell
        self._drain(False)                   # earlier batches: their events fired with the batch's own copy back
        handle = backend.fidelity_handle()
        if handle is None:
            raise RuntimeError("--fidelity-report: the backend rendered without measuring")
        self.shape, self.cell = tuple(int(v) for v in frame_size), verify_cell(q[0], q[2])
        self._pending.append((backend, handle, list(indices)))

    def _drain(self, wait):
        while self._pending:
            backend, handle, indices = self._pending[0]
            rec = backend.read_fidelity(handle, wait)
            if rec is None:
                return
            self._pending.popleft()
            for name, r in zip(SERIES, rec):
                self.records.setdefault(name, []).extend((i, np.asarray(row, np.int64)) for i, row in zip(indices, r))

    def finish(self, output_path, frames_dir, world):
        """-> the manifest's fidelity_report entry, the report next to the manifest or at its path (.data: its content, None when sharded)"""
        self._drain(True)
        if world != 1:
            self.report()
            return {"fidelity_report": dict(path=None, summary=None, reason=SHARDED_REASON)}, {}
        path = output_path.with_name(output_path.with_suffix("").name + "_fidelity.json") if self.path is True else Path(self.path)
        s = summary(self.records)
        W, H = self.shape if self.shape else (0, 0)
        params = dict(bad_threshold=self.bad_threshold, cell=list(self.cell or (None, None)), window="8 x 8 cells at stride 4",
                      reference="the stored eyes of the SBS clip, sampled through the render's own map")
        head = dict(parameters=params, width=W, height=H, series=s["series"])
        if not self.ceiling:
            head["ceiling_reason"] = CEILING_REASON
        self.data = dict(head, units=dict(mean_abs="levels per channel", psnr="dB over the cell means", ssim="mean over the windows"),
                         frames=s["frames"])
        self.report()
        entry = dict(path=str(path), **{k: v for k, v in head.items() if k != "series"},
                     summary={k: (None if v is None else {a: b for a, b in v.items() if a != "worst_frames"}) for k, v in s["series"].items()})
        return {"fidelity_report": _jsonable(entry)}, {path: json.dumps(_jsonable(self.data), indent=1)}

    def report(self):
        if self.data is None:
            print(f"Fidelity report: not made ({SHARDED_REASON})")
            return
        num = lambda v, f="{:.4f}": "n/a" if v is None else f.format(v)
        print(f"Fidelity report ({self.data['series']['final']['frames']} frames, cells of {self.cell[0]} x {self.cell[1]} pixels, against the SBS clip's stored eyes):")
        notes = dict(warp="right eye, depth + DIBR alone", final="right eye as written, contains source samples", ceiling="left eye = the 4K frame: the two releases")
        for name in SERIES:
            s = self.data["series"].get(name)
            if s is None:
                print(f"  {name}: not measured ({CEILING_REASON})")
                continue
            print(f"  {name} ({notes[name]}): SSIM {num(s['ssim'])}, PSNR {num(s['psnr'], '{:.2f}')} dB, mean abs {num(s['mean_abs'], '{:.2f}')} levels, "
                  f"cells above {self.bad_threshold}: {num(None if s['bad_share'] is None else 100 * s['bad_share'], '{:.2f}')} %")
