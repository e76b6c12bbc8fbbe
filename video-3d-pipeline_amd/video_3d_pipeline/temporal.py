"""Temporal stabilisation of the depth sequence (opt-in: `--temporal-radius R`, R in 1..8).

Per frame the matcher's disparity jitters and the u16 normalisation takes the frame's own min and max, so static background
moves in the 3D video.  With a radius this stage sits on the device between `sbs_to_disparity` and the u16 samples:

  * scene cuts from the left gray (mean absolute luma difference above `cut_threshold` levels): frames on two sides of a cut
    never mix;
  * a cross-bilateral filter over the 2R+1 frames around a target: triangular weight in time, a weight that falls with the
    3x3 luma difference to the target (so moving objects are left alone), invalid pixels skipped (and, with `fill`, filled);
  * the u16 samples against the min / max of the whole window instead of the frame's own.

All of it is integer arithmetic with a bit-exact contract (include/v3d_hip.h; tests/temporal_ref.py restates it).

`--temporal-motion S` (opt-in, needs a radius; S in 1..32 pixels per frame step) compensates the window for motion: a block
matcher finds one vector per 16x16 luma block between adjacent frames, forward and backward; a neighbouring frame is read where
the target's block went (the vectors chained step by step), and a scene cut is what the matcher cannot explain (the compensated
residual above `cut_threshold` levels per pixel) rather than what moved.  A pan or a moving object then keeps its neighbours
(contract: include/v3d_hip.h, tests/temporal_mc_ref.py).

`--range-percentile P` (opt-in, with or without a radius) makes the white point of that normalisation robust: a frame's "max"
becomes the P-th percentile of its valid disparities, so a few mismatched pixels no longer set the scale of every sample
(contract: include/v3d_hip.h, tests/range_ref.py).  Everything after the per-frame (min, max) is unchanged.

`--fill-holes` (opt-in, per frame, combines with both) fills the matcher's invalid pixels from their scanline neighbours on the
int16 disparity, before anything above sees it (contract: include/v3d_hip.h, tests/fill_ref.py).

`TemporalStabilizer` is the streaming driver: a clip arrives in passes of any size, the output lags the input by R frames
and the last 2R frames of depth and gray stay on the device between passes.  The result does not depend on how the clip is
cut into passes.  Frames before the first pushed frame and after the last one do not exist for the window.
"""

MAX_RADIUS = 8
MAX_MOTION_SEARCH = 32
DEFAULT_TAU = 12
DEFAULT_CUT = 20
RANGE_Q_MIN, RANGE_Q_OFF = 5000, 10000      # the range percentile in parts per 10000; 10000 = the maximum = off


def check_parameters(radius: int, tau: int = DEFAULT_TAU, cut_threshold: int = DEFAULT_CUT, fill: bool = True):
    """validated (radius, tau, cut_threshold, fill) as plain ints / bool; radius 0 means the stage is off"""
    vals = {"temporal radius": (radius, 0, MAX_RADIUS), "temporal tau": (tau, 1, 255), "temporal cut threshold": (cut_threshold, 0, 256)}
    for name, (v, lo, hi) in vals.items():
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(radius), int(tau), int(cut_threshold), bool(fill)


def check_motion_search(motion_search, radius: int) -> int:
    """--temporal-motion S: an integer in [0, 32], 0 = off; S > 0 needs a radius"""
    if isinstance(motion_search, bool) or int(motion_search) != motion_search or not 0 <= motion_search <= MAX_MOTION_SEARCH:
        raise ValueError(f"temporal motion search must be an integer in [0, {MAX_MOTION_SEARCH}], got {motion_search!r}")
    if motion_search > 0 and radius < 1:
        raise ValueError("--temporal-motion needs --temporal-radius of at least 1")
    return int(motion_search)


def check_range_percentile(percentile) -> int:
    """--range-percentile P, a number in [50, 100] with at most two decimals -> q = P in parts per 10000; 100 means off"""
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float)):
        raise ValueError(f"range percentile must be a number in [50, 100], got {percentile!r}")
    if not 50 <= percentile <= 100:                          # NaN fails both comparisons
        raise ValueError(f"range percentile must lie in [50, 100], got {percentile!r}")
    q = round(percentile * 100)
    if abs(percentile * 100 - q) > 1e-6:
        raise ValueError(f"range percentile may have at most two decimals, got {percentile!r}")
    return int(q)


def cache_suffix(radius: int, tau: int, cut_threshold: int, fill: bool, range_quantile: int = RANGE_Q_OFF, motion_search: int = 0) -> str:
    """what the depth cache key gains when the stage or the robust range is on ('' when off: the reference's key unchanged)"""
    s = f"_temporal_r{radius}_t{tau}_c{cut_threshold}_f{int(bool(fill))}" if radius > 0 else ""
    if radius > 0 and motion_search > 0:
        s += f"_m{motion_search}"
    return s + (f"_rangeq{range_quantile}" if range_quantile < RANGE_Q_OFF else "")


def manifest_entry(radius: int, tau: int, cut_threshold: int, fill: bool, range_quantile: int = RANGE_Q_OFF, motion_search: int = 0) -> dict:
    entry = {"radius": radius, "tau": tau, "cut_threshold": cut_threshold, "fill": bool(fill)}
    if motion_search > 0:
        entry["motion_search"] = motion_search
    if range_quantile < RANGE_Q_OFF:
        entry["range_quantile"] = range_quantile
    return entry


class TemporalStabilizer:
    """push(depth [n,H,W], gray [n,H,W]) -> stabilised u16 samples of every frame whose window is complete (possibly none:
    then None); finish() -> the tail, with windows clipped at the end of the clip.  The arrays are whatever the backend's
    `sbs_to_disparity` / `left_gray` return (device tensors for the HIP backend); the driver touches them only through
    `backend.temporal_concat` and `backend.temporal_stabilize`."""

    def __init__(self, backend, radius: int, tau: int = DEFAULT_TAU, cut_threshold: int = DEFAULT_CUT, fill: bool = True,
                 range_quantile: int = RANGE_Q_OFF, observe=None, motion_search: int = 0, metric: bool = False):
        """observe (--quality-report): a callable the backend's temporal_stabilize calls with the filtered depth and the targets'
        gray; None (the default) adds no argument to that call.  motion_search (--temporal-motion): S > 0 adds the keyword
        `motion_search=S` to that call; 0 (the default) adds nothing.  metric (--depth-range metric): adds the keyword
        `metric=True`, the constant range (0, 64) in place of the window's; off adds nothing"""
        self.observe = observe
        self.metric = bool(metric)
        self.radius, self.tau, self.cut_threshold, self.fill = check_parameters(radius, tau, cut_threshold, fill)
        self.motion_search = check_motion_search(motion_search, self.radius)
        if isinstance(range_quantile, bool) or int(range_quantile) != range_quantile or not RANGE_Q_MIN <= range_quantile <= RANGE_Q_OFF:
            raise ValueError(f"range quantile must be an integer in [{RANGE_Q_MIN}, {RANGE_Q_OFF}], got {range_quantile!r}")
        self.range_quantile = int(range_quantile)
        if self.radius < 1:
            raise ValueError("TemporalStabilizer needs a radius of at least 1 (radius 0 is the per-frame path)")
        self.backend = backend
        self._depth = self._gray = None      # frames first .. first+len-1 of the clip
        self._first = 0
        self._next = 0                       # the next target to emit
        self._finished = False

    def _emit(self, upto: int):
        """targets self._next .. upto-1 out of the held buffer"""
        n = upto - self._next
        if n <= 0:
            return None
        args = (self._depth, self._gray, self._next - self._first, n, self.radius, self.tau, self.cut_threshold, self.fill)
        if self.range_quantile < RANGE_Q_OFF:                # off: the call a backend without the robust range knows
            args += (self.range_quantile,)
        kw = {} if self.observe is None else {"observe": self.observe}
        if self.motion_search > 0:                           # off: no keyword, the call every backend knows
            kw["motion_search"] = self.motion_search
        if self.metric:
            kw["metric"] = True
        out = self.backend.temporal_stabilize(*args, **kw)
        self._next = upto
        return out

    def push(self, depth, gray):
        if self._finished:
            raise RuntimeError("push() after finish()")
        if len(depth) != len(gray):
            raise ValueError(f"{len(depth)} depth frames and {len(gray)} gray frames")
        if len(depth) == 0:
            return None
        be = self.backend
        self._depth = be.temporal_concat(self._depth, depth)
        self._gray = be.temporal_concat(self._gray, gray)
        end = self._first + len(self._depth)
        out = self._emit(end - self.radius)
        keep = min(2 * self.radius, len(self._depth))          # the next target is end - R at the earliest; it reaches back R more
        self._first = end - keep
        self._depth, self._gray = self._depth[len(self._depth) - keep:], self._gray[len(self._gray) - keep:]
        return out

    def finish(self):
        if self._finished:
            raise RuntimeError("finish() called twice")
        self._finished = True
        out = None if self._depth is None else self._emit(self._first + len(self._depth))
        self._depth = self._gray = None
        return out

    def pending(self) -> int:
        """frames pushed but not yet returned"""
        return 0 if self._depth is None else self._first + len(self._depth) - self._next


class BlockStabilizer:
    """TemporalStabilizer for one rank's share of a clip (sharding.temporal_block): the rank pushes frames
    first - halo_before .. first + count + halo_after - 1 in order and gets back (frame indices, u16 samples) of the frames
    it owns; the halo frames only feed the windows."""

    def __init__(self, backend, params, first: int, count: int, halo_before: int, range_quantile: int = RANGE_Q_OFF, observe=None,
                 motion_search: int = 0, metric: bool = False):
        self.stab = TemporalStabilizer(backend, *params, range_quantile, observe, motion_search, **({"metric": True} if metric else {}))
        self.first, self.count = first, count
        self._at = first - halo_before           # clip index of the next frame the stabiliser returns

    def _owned(self, out):
        if out is None:
            return [], None
        a, b = self._at, self._at + len(out)
        self._at = b
        lo, hi = max(a, self.first), min(b, self.first + self.count)
        if hi <= lo:
            return [], None
        return list(range(lo, hi)), out[lo - a:hi - a]

    def push(self, depth, gray):
        return self._owned(self.stab.push(depth, gray))

    def finish(self):
        return self._owned(self.stab.finish())


def add_temporal_arguments(parser):
    """the CLI surface shared by the depth CLI and the one-pass pipeline"""
    parser.add_argument('--temporal-radius', type=int, default=0,
                        help=f'Temporal depth stabilisation over 2R+1 frames, R in 1..{MAX_RADIUS} (default 0: off, every frame on '
                             'its own).  Frames before --start-frame and after the last processed frame do not exist for the window')
    parser.add_argument('--temporal-tau', type=int, default=DEFAULT_TAU,
                        help=f'Luma difference (levels, 3x3 mean) at which a neighbouring frame stops contributing (default {DEFAULT_TAU})')
    parser.add_argument('--temporal-cut', type=int, default=DEFAULT_CUT,
                        help=f'Mean absolute luma difference (levels) between frames that counts as a scene cut (default {DEFAULT_CUT})')
    parser.add_argument('--no-temporal-fill', action='store_true',
                        help='Leave pixels that are invalid in a frame invalid instead of filling them from its neighbours')
    parser.add_argument('--temporal-motion', type=int, default=0,
                        help=f'Motion-compensate the temporal window: block-matching search radius in pixels per frame step, '
                             f'1..{MAX_MOTION_SEARCH} (default 0: off, a neighbouring frame is read at the same coordinates).  Needs '
                             '--temporal-radius; 16 covers a pan of 16 px per frame')


def add_range_arguments(parser):
    """--range-percentile, shared by the depth CLI and the one-pass pipeline"""
    parser.add_argument('--range-percentile', type=float, default=100.0,
                        help='White point of the 16-bit normalisation: this percentile of the valid disparities of a frame (of the '
                             'window, with --temporal-radius) instead of the maximum; 50..100, at most two decimals (default 100: '
                             'the maximum, off).  98 keeps a few mismatched pixels from setting the range')


def add_fill_arguments(parser):
    """--fill-holes, shared by the depth CLI and the one-pass pipeline"""
    parser.add_argument('--fill-holes', action='store_true',
                        help="Fill the matcher's invalid pixels (the 64 leftmost columns, occlusions, rejected matches) from their "
                             'scanline neighbours with the background value before the depth is normalised (default: off, they '
                             'stay depth 0)')


METRIC_LO, METRIC_HI = 0, 64                                   # --depth-range metric: the matcher's rebiased window, in pixels
DEPTH_RANGES = ("frame", "metric")


def add_depth_range_arguments(parser):
    """--depth-range, shared by the depth CLI and the one-pass pipeline"""
    parser.add_argument('--depth-range', choices=DEPTH_RANGES, default='frame',
                        help=f"Range of the 16-bit normalisation.  frame: every frame (window, with --temporal-radius) against its own "
                             f"minimum and maximum (default).  metric: the constant range [{METRIC_LO}, {METRIC_HI}], so a sample s is a "
                             f"rebiased disparity of {METRIC_HI} s / 65535 pixels whatever else is in the frame (what convert's --parallax "
                             f"source needs); use it with --fill-holes")


def check_depth_range(mode, range_quantile: int = RANGE_Q_OFF) -> str:
    if mode not in DEPTH_RANGES:
        raise ValueError(f"depth_range must be one of {DEPTH_RANGES}, got {mode!r}")
    if mode == "metric" and range_quantile < RANGE_Q_OFF:
        raise ValueError("--depth-range metric fixes the range: it cannot be combined with --range-percentile below 100")
    return mode


def depth_range_options(args) -> dict:
    """nothing at the default, so a constructor that predates the flag is called as before"""
    return {"depth_range": args.depth_range} if getattr(args, "depth_range", "frame") != "frame" else {}


def depth_range_suffix(mode: str) -> str:
    """what the depth cache key gains, after every other suffix, with --depth-range metric ('' at the default)"""
    return "_metric" if mode == "metric" else ""


def fill_options(args) -> dict:
    return dict(fill_holes=args.fill_holes)


def fill_suffix(fill_holes: bool) -> str:
    """what the depth cache key gains, after the temporal and range suffixes, with --fill-holes ('' when off)"""
    return "_fill1" if fill_holes else ""


def range_options(args) -> dict:
    return dict(range_percentile=args.range_percentile)


def temporal_options(args) -> dict:
    """parsed arguments -> the constructors' keyword arguments"""
    return dict(temporal_radius=args.temporal_radius, temporal_tau=args.temporal_tau, temporal_cut=args.temporal_cut,
                temporal_fill=not args.no_temporal_fill, temporal_motion=getattr(args, "temporal_motion", 0))
