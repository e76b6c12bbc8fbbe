"""Frame-accurate matching of the SBS clip and the 4K clip (no counterpart in the reference, which trusts the rounded audio offset).

Every stage after the alignment pairs SBS frame i with 4K frame guide_start_frame + i.  Here that pairing is measured: the device
turns each luma plane -- the left view's gray plane and the 4K frame's luma -- into a signature of 64 x 36 cell means
(v3d_frame_signature_batch) and correlates signatures in exact integers (v3d_signature_scores); the host divides,

    Z = num / sqrt(float64(var_a) * float64(var_b)),

the zero-mean normalised correlation, which no gain or offset of either image changes (the two releases are graded differently).
A pair with a zero variance (a flat frame, a fade to black) is uninformative and has no Z (NaN here).

Two surfaces: refine() -- the align CLI's --refine-video / --video-only -- searches the shift of the guide start frame around a
seed, and GuideChecker -- the one-pass pipeline's --check-guide -- scores the pairing a run actually uses.  zncc() and decide() are
plain NumPy; bit-exact contract of the device part and restatement of the rule: tests/framematch_ref.py.
"""
from typing import Dict, List, Optional

import numpy as np

from .utils import get_video_info, iter_frames

DEFAULT_SEARCH, DEFAULT_WINDOW, DEFAULT_PROBES = 4, 24, 3
DEFAULT_MIN_SCORE, DEFAULT_MIN_MARGIN = 0.5, 0.01          # product conventions, not measurements
FPS_TOLERANCE = 0.1                                        # the reference's own (utils.py:248-249 validate_video_compatibility)
CHECK_SEARCH = 2                                           # --check-guide looks this far inside one guided batch
DEFAULT_CHECK_MIN = 0.5
ADVICE = "python -m video_3d_pipeline.align --refine-video"


def zncc(num, var_a, var_b) -> np.ndarray:
    """the integer scores of v3d_signature_scores -> Z float64 [na,nb]; NaN where a variance is 0 (uninformative pair)"""
    num = np.asarray(num, dtype=np.int64)
    va = np.asarray(var_a, dtype=np.int64).astype(np.float64).reshape(-1, 1)
    vb = np.asarray(var_b, dtype=np.int64).astype(np.float64).reshape(1, -1)
    prod = va * vb
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = num.astype(np.float64) / np.sqrt(prod)
    Z[~(prod > 0)] = np.nan
    return Z


def _best(values, search: int) -> Optional[int]:
    """the shift d in [-search, search] with the largest defined values[d + search]; ties go to the smaller |d|, then to the
    negative d; None if nothing is defined"""
    best = None
    for d in sorted(range(-search, search + 1), key=lambda d: (abs(d), d)):
        v = values[d + search]
        if not np.isnan(v) and (best is None or v > values[best + search]):
            best = d
    return best


def shift_means(Z: np.ndarray, col0: int, search: int) -> np.ndarray:
    """m(d), d = -search .. search: the mean of Z[a][col0 + a + d] over the rows a whose column exists and whose pair is
    informative; NaN unless they are at least half of the rows"""
    w, nb = Z.shape
    m = np.full(2 * search + 1, np.nan)
    rows = np.arange(w)
    for d in range(-search, search + 1):
        cols = col0 + rows + d
        ok = (cols >= 0) & (cols < nb)
        v = Z[rows[ok], cols[ok]]
        v = v[~np.isnan(v)]
        if v.size and 2 * v.size >= w:
            m[d + search] = v.sum() / v.size
    return m


def decide(probes, search: int = DEFAULT_SEARCH, min_score: float = DEFAULT_MIN_SCORE, min_margin: float = DEFAULT_MIN_MARGIN) -> Dict:
    """The decision rule.  probes: [(Z [w,nb], col0)] -- row a of a probe's window and shift d meet at column col0 + a + d.
    1. m_p(d) = shift_means of probe p;  2. the probe's shift = argmax_d m_p(d) (ties: smaller |d|, then negative);
    3. M(d) = mean of the defined m_p(d), d* = its argmax under the same ties, margin = M(d*) - the second best M;
    4. refined iff M(d*) >= min_score, margin >= min_margin and every probe that has a shift agrees with d*;
    5. otherwise inconsistent iff a probe disagrees (differing cuts, drift), else undetermined (static scene, low texture, too few
       informative frames); both keep the seed: shift = 0."""
    nd = 2 * search + 1
    m = np.full((len(probes), nd), np.nan)
    for p, (Z, col0) in enumerate(probes):
        m[p] = shift_means(np.asarray(Z, dtype=np.float64), int(col0), search)
    shifts = [_best(m[p], search) for p in range(len(probes))]
    scores = [None if s is None else float(m[p, s + search]) for p, s in enumerate(shifts)]
    M = np.full(nd, np.nan)
    for k in range(nd):
        col = m[:, k]
        col = col[~np.isnan(col)]
        if col.size:
            M[k] = col.sum() / col.size
    d = _best(M, search)
    out = dict(M=M, probe_shifts=shifts, probe_scores=scores)
    if d is None:
        out.update(status="undetermined", best_shift=0, shift=0, score=None, margin=None)
        return out
    rest = np.delete(M, d + search)
    rest = rest[~np.isnan(rest)]
    margin = float(M[d + search] - rest.max()) if rest.size else 0.0
    agree = all(s == d for s in shifts if s is not None)
    if M[d + search] >= min_score and margin >= min_margin and agree:
        status = "refined"
    else:
        status = "undetermined" if agree else "inconsistent"
    out.update(status=status, best_shift=d, shift=d if status == "refined" else 0, score=float(M[d + search]), margin=margin)
    return out


def probe_starts(count: int, window: int, probes: int):
    """(first frames of the probe windows relative to the start frame, window length): `probes` windows of `window` frames spread
    evenly over `count` frames; a short clip gives fewer or shorter ones"""
    w = min(window, count)
    if probes <= 1 or count - w <= 0:
        return [0], w
    return sorted({(count - w) * p // (probes - 1) for p in range(probes)}), w


def check_parameters(search, window, probes, min_score, min_margin):
    for name, v, lo, hi in (("search", search, 1, 64), ("window", window, 2, 1024), ("probes", probes, 1, 64)):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError(f"refine {name} must be an integer in [{lo}, {hi}], got {v!r}")
    if window + 2 * search > 4096:
        raise ValueError(f"refine window + 2 * search = {window + 2 * search} exceeds 4096 signatures per call")
    for name, v in (("min_score", min_score), ("min_margin", min_margin)):
        if not np.isfinite(v):
            raise ValueError(f"refine {name} must be finite, got {v!r}")
    return int(search), int(window), int(probes), float(min_score), float(min_margin)


def _clip_frames(info, start_frame=0, max_frames=None) -> int:
    total = info.get("frames", 0) or int(info["duration"] * info["fps"])
    n = total - start_frame
    return n if max_frames is None else min(max_frames, n)


def refine(sbs_video: str, video_4k: str, guide_start_frame: int, start_frame: int = 0, search: int = DEFAULT_SEARCH,
           window: int = DEFAULT_WINDOW, probes: int = DEFAULT_PROBES, unsqueeze: bool = True, max_frames: Optional[int] = None,
           min_score: float = DEFAULT_MIN_SCORE, min_margin: float = DEFAULT_MIN_MARGIN, backend=None, input_layout: str = "sbs") -> Dict:
    """Refine the 4K frame that belongs to SBS frame start_frame, seeded with guide_start_frame (g0).  Decodes `probes` windows of
    `window` consecutive SBS frames spread over the clip (or over max_frames) and, per window starting at frame s, the 4K frames
    g0 + s - search .. g0 + s + window - 1 + search; the left eye (the backend's SBS staging and v3d_sbs_to_gray_batch) and the 4K
    luma (its guide staging and v3d_bgr_to_gray) give signatures on the device, one v3d_signature_scores call per probe gives the
    integers, decide() the answer.  Returns decide()'s result plus guide_start_frame (g0 + shift), guide_start_frame_seed, the
    parameters and `ints`, the probes' integer scores.  input_layout "tb": the left eye is the top half of the frame (the backend's
    calls and the recorded parameters gain the keyword; an SBS run's are what they were).  ValueError: unreadable clips, unequal
    frame rates, bad parameters."""
    search, window, probes, min_score, min_margin = check_parameters(search, window, probes, min_score, min_margin)
    info_s, info_g = get_video_info(sbs_video), get_video_info(video_4k)
    if not info_s or not info_g:
        raise ValueError(f"Could not read video info: {sbs_video if not info_s else video_4k}")
    if abs(float(info_s["fps"]) - float(info_g["fps"])) > FPS_TOLERANCE:
        raise ValueError(f"video refinement refused: frame rates differ ({info_s['fps']:.3f} vs {info_g['fps']:.3f} fps); frames can "
                         f"only be matched one to one between clips of equal rate")
    from .depth import check_frame_halves, check_input_layout
    layout = {"input_layout": check_input_layout(input_layout)} if input_layout != "sbs" else {}
    check_frame_halves(info_s["width"], info_s["height"], input_layout)
    count, n4k = _clip_frames(info_s, start_frame, max_frames), _clip_frames(info_g)
    if count < 1:
        raise ValueError("No frames extracted from video")
    if backend is None:
        from .pipeline import HipPipelineBackend
        backend = HipPipelineBackend("cuda")
    g0 = int(guide_start_frame)
    starts, w = probe_starts(count, window, probes)
    plist, ints, used = [], [], []
    for s in starts:
        lo, hi = max(0, g0 + s - search), min(n4k, g0 + s + w + search)
        if hi <= lo:
            continue                                             # the whole probe lies outside the 4K clip
        sbs = list(iter_frames(sbs_video, start_frame + s, w))
        guides = list(iter_frames(video_4k, lo, hi - lo))
        if not sbs or not guides:
            continue
        sig_a = backend.sbs_left_signatures(sbs, unsqueeze, **layout)
        sig_b = backend.guide_signatures(guides, info_g["height"], info_g["width"])
        num, va, vb = backend.read_scores(backend.signature_scores(sig_a, sig_b))
        ints.append((num, va, vb))
        plist.append((zncc(num, va, vb), g0 + s - lo))
        used.append(s)
    out = decide(plist, search, min_score, min_margin)
    out.update(guide_start_frame_seed=g0, guide_start_frame=g0 + out["shift"], probe_starts=used, ints=ints,
               parameters=dict(search=search, window=w, probes=probes, min_score=min_score, min_margin=min_margin,
                               unsqueeze=bool(unsqueeze), start_frame=int(start_frame), max_frames=max_frames, **layout))
    return out


def alignment_keys(res: Dict, seed_audio: Optional[int]) -> Dict:
    """what a refine() result adds to alignment_data.json"""
    f = lambda v: None if v is None else float(v)
    return {
        "guide_start_frame_audio": seed_audio,
        "guide_start_frame": int(res["guide_start_frame"]),
        "visual_status": res["status"],
        "visual_shift_frames": int(res["shift"]),
        "visual_score": f(res["score"]),
        "visual_margin": f(res["margin"]),
        "visual_probe_shifts": res["probe_shifts"],
        "visual_probe_scores": [f(v) for v in res["probe_scores"]],
        "visual_parameters": res["parameters"],
    }


def add_refine_arguments(parser):
    parser.add_argument('--refine-video', action='store_true',
                        help='After the audio alignment, refine the guide start frame by matching frames on the GPU')
    parser.add_argument('--video-only', action='store_true',
                        help='Skip the audio step (clips without usable audio) and match frames around --guide-start-frame')
    parser.add_argument('--guide-start-frame', type=int, default=0, help='Seed of --video-only: 4K frame of the first SBS frame (default 0)')
    parser.add_argument('--refine-search', type=int, default=DEFAULT_SEARCH, help=f'Search +-K frames around the seed (default {DEFAULT_SEARCH})')
    parser.add_argument('--refine-window', type=int, default=DEFAULT_WINDOW, help=f'Consecutive frames per probe (default {DEFAULT_WINDOW})')
    parser.add_argument('--refine-probes', type=int, default=DEFAULT_PROBES, help=f'Probe windows spread over the clip (default {DEFAULT_PROBES})')
    parser.add_argument('--refine-min-score', type=float, default=DEFAULT_MIN_SCORE, help=f'Least mean correlation to accept (default {DEFAULT_MIN_SCORE})')
    parser.add_argument('--refine-min-margin', type=float, default=DEFAULT_MIN_MARGIN,
                        help=f'Least lead over the second-best shift (default {DEFAULT_MIN_MARGIN})')
    parser.add_argument('--start-frame', type=int, default=0, help='First SBS frame of the refinement (default 0)')
    parser.add_argument('--max-frames', type=int, default=None, help='Spread the probes over this many SBS frames (default: the clip)')
    parser.add_argument('--no-unsqueeze', action='store_true', help='Match the squeezed left eye (as the depth CLI with --no-unsqueeze)')
    from .depth import add_input_layout_argument
    add_input_layout_argument(parser)


def refine_options(args) -> Dict:
    from .depth import input_layout_options
    return dict(start_frame=args.start_frame, search=args.refine_search, window=args.refine_window, probes=args.refine_probes,
                unsqueeze=not args.no_unsqueeze, max_frames=args.max_frames, min_score=args.refine_min_score,
                min_margin=args.refine_min_margin, **input_layout_options(args))


class GuideChecker:
    """--check-guide of the one-pass pipeline: scores the pairing of the left views with the 4K frames a run filters against.
    The driver calls note_left() while a pass's left gray planes are valid (the matched frame and the emitted frame differ under
    --temporal-radius, so signatures are kept on the device by clip frame index), emit() enqueues the batch's luma signatures,
    ONE scores call and the copy of the three small arrays, and collect() reads them after the batch's own synchronise.  The
    backend supplies frame_signatures(gray), signature_scores(rows, sig), guide_scores(rows, luma) and read_scores(handle)."""

    def __init__(self, backend, threshold: float = DEFAULT_CHECK_MIN, consecutive: bool = True):
        if not np.isfinite(threshold):
            raise ValueError(f"--check-guide-min must be finite, got {threshold!r}")
        self.backend, self.threshold, self.consecutive = backend, float(threshold), bool(consecutive)
        self._sigs = {}
        self.scores: List = []                 # (clip frame, Z)
        self.skipped = 0
        self.batch_shifts: List[int] = []
        self.summary = None

    def note_left(self, indices, gray):
        sig = self.backend.frame_signatures(gray)
        for k, i in enumerate(indices):
            self._sigs[i] = sig[k]

    def emit(self, idx, frames, luma):
        """-> a handle for collect(); nothing here waits for the device"""
        rows = [self._sigs.pop(i) for i in idx]
        for i in [i for i in self._sigs if i < idx[0]]:          # halo frames that are matched but never emitted
            del self._sigs[i]
        return list(idx), [f is not None for f in frames], self.backend.guide_scores(rows, luma)

    def collect(self, pending):
        idx, has_guide, handle = pending
        Z = zncc(*self.backend.read_scores(handle))
        Z[:, ~np.asarray(has_guide)] = np.nan                    # flat guides (beyond the 4K clip) are not 4K frames
        for k, i in enumerate(idx):
            if np.isnan(Z[k, k]):
                self.skipped += 1
            else:
                self.scores.append((int(i), float(Z[k, k])))
        n = len(idx)
        if self.consecutive and n >= 2 and all(b - a == 1 for a, b in zip(idx, idx[1:])):
            d = _best(shift_means(Z, 0, CHECK_SEARCH), CHECK_SEARCH)
            if d is not None:
                self.batch_shifts.append(d)

    def finish(self, total=lambda v: v) -> Dict:
        """the summary (also kept in .summary): counts summed over the ranks by `total`, the rest this rank's"""
        z = np.array([s for _, s in self.scores], dtype=np.float64)
        below = int((z < self.threshold).sum())
        votes = {d: self.batch_shifts.count(d) for d in set(self.batch_shifts)}
        suspected = min(votes, key=lambda d: (-votes[d], abs(d), d)) if votes else 0
        nonzero = sum(1 for d in self.batch_shifts if d != 0)
        worst = min(self.scores, key=lambda t: (t[1], t[0]))[0] if self.scores else None
        self.summary = dict(frames_checked=int(total(len(self.scores))), frames_below=int(total(below)), skipped=int(total(self.skipped)),
                            median=float(np.median(z)) if z.size else None, min=float(z.min()) if z.size else None,
                            worst_frame=worst, suspected_shift=int(suspected), threshold=self.threshold)
        self.warn = bool((z.size and np.median(z) < self.threshold) or (self.batch_shifts and 2 * nonzero > len(self.batch_shifts)))
        return self.summary

    def report(self):
        s = self.summary
        med = "n/a" if s["median"] is None else f"{s['median']:.4f}"
        low = "n/a" if s["min"] is None else f"{s['min']:.4f} (frame {s['worst_frame']})"
        print(f"Guide check: {s['frames_checked']} frames checked, {s['frames_below']} below {self.threshold:g}, {s['skipped']} skipped; "
              f"median {med}, min {low}, suspected shift {s['suspected_shift']:+d}")
        if self.warn:
            print(f"Warning: the 4K guide frames do not match the SBS frames (median {med}, suspected shift "
                  f"{s['suspected_shift']:+d} frames); re-align the clips with `{ADVICE}`")
