"""Depth extraction from SBS stereoscopic video -- MI355X-native host side.

Mirror of reference src/video_3d_pipeline/depth.py (class, method names, argument meaning, error
behaviour, CLI flags) with the per-frame arithmetic moved from OpenCV-on-CPU to libv3d_hip.so:

    split_sbs_frame     depth.py:250-268  -> v3d_split_sbs / v3d_sbs_to_gray (input_layout "tb": v3d_split_tb / v3d_tb_to_gray)
    process_frame_batch depth.py:297-395  -> v3d_bgr_to_gray + v3d_sgbm_compute_batch + v3d_disp_to_depth
    save_depth_map      depth.py:397-406  -> v3d_depth_to_u16 + 16-bit PNG (Pillow)
    process_video_sbs   depth.py:408-476  -> streaming decode -> fused SBS batch path -> PNG cache
    main                depth.py:479-538  -> same argparse surface, exit code 0/1

There is no CPU compute path: without a GPU (or without libv3d_hip.so) construction fails loudly,
like the reference's `RuntimeError("CUDA not available but requested")` (depth.py:43-44).
Neural guidance (the reference's DPT blend, depth.py:344-371): the blend itself -- resize of the monocular map,
min-max to the disparity range, 0.7 / 0.3 mix, clamp -- runs on the GPU (v3d_mono_blend).  The monocular map comes
from a provider: `DPTForDepthEstimation` loaded from a LOCAL directory (or an already populated HF cache; nothing is
ever downloaded), or any callable handed to the constructor (`mono_provider`).  When neither is available the loader
falls back to stereo-only exactly like the reference does when loading fails (depth.py:107-114).
"""
import argparse
import hashlib
from collections import defaultdict
from itertools import islice
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .backend import HipBackend, require_hip_device
from .utils import PngWriterPool, create_work_directory, get_video_info, iter_frames, write_png16


# --min-disparity: the matcher's search window is [m, m + 64), m in [-64, 0] ("minDisparity"); 0 = the reference's
MIN_DISPARITY_CANDIDATES = (0, -16, -32, -48, -64)       # what `auto` tries
MIN_DISPARITY_CALIBRATION_FRAMES = 8
MIN_DISPARITY_BAD = 16                                   # the quality report's default bad threshold: auto scores with it


def check_min_disparity(value, allow_auto: bool = True):
    """validated --min-disparity: an integer in [-64, 0], or "auto" where a clip is at hand"""
    if isinstance(value, str) and value == "auto":
        if not allow_auto:
            raise ValueError('min_disparity="auto" needs a clip to calibrate on: give an integer here')
        return "auto"
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not -64 <= value <= 0:
        raise ValueError(f'min_disparity must be an integer in [-64, 0] or "auto", got {value!r}')
    return int(value)


def min_disparity_argument(text: str):
    """argparse type of --min-disparity"""
    try:
        return check_min_disparity(text if text == "auto" else int(text))
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def choose_min_disparity(scores: Dict[int, int]) -> int:
    """the rule of --min-disparity auto: scores[m] = pixels of the calibration frames whose reprojection error stays within the
    bad threshold.  The candidate nearest 0 within 2 % of the best wins (integers: 100 * score >= 98 * best), so the reference's
    window stays where it is as good; 0 when nothing scored"""
    best = max(scores.values())
    if best <= 0:
        return 0
    return max(m for m, s in scores.items() if 100 * s >= 98 * best)


def calibration_frames(start_frame: int, frame_count: int) -> List[int]:
    """the clip frames `auto` calibrates on: K = min(8, N) of the N the run will process, spread evenly"""
    k = min(MIN_DISPARITY_CALIBRATION_FRAMES, frame_count)
    stride = max(frame_count // k, 1) if k else 1
    return [start_frame + stride // 2 + j * stride for j in range(k)]


INPUT_LAYOUTS = ("sbs", "tb")                            # --input-layout: the eyes side by side, or the left eye on top


def check_input_layout(value) -> str:
    if value not in INPUT_LAYOUTS:
        raise ValueError(f"input_layout must be one of {INPUT_LAYOUTS}, got {value!r}")
    return value


def add_input_layout_argument(parser):
    """--input-layout, declared once for the depth, pipeline and align CLIs"""
    parser.add_argument('--input-layout', choices=INPUT_LAYOUTS, default='sbs',
                        help='How the stereoscopic clip packs its eyes: sbs = side by side, left eye first (default); tb = top-bottom '
                             '(over-under), left eye on top.  Squeezed eyes are stretched back along the packed axis unless '
                             '--no-unsqueeze says they are stored at full size')


def input_layout_options(args) -> dict:
    """the keyword only when the layout is not the default: an SBS run calls everything as before (and so does a caller whose
    arguments predate the flag)"""
    layout = getattr(args, "input_layout", "sbs")
    return {"input_layout": layout} if layout != "sbs" else {}


def input_layout_suffix(input_layout: str) -> str:
    """what the depth cache key gains, last, for a top-bottom clip"""
    return f"_{input_layout}" if input_layout != "sbs" else ""


def check_frame_halves(width: int, height: int, input_layout: str = "sbs"):
    """a frame of two eyes has an even width (side by side) or an even height (top-bottom)"""
    if input_layout == "tb":
        if height % 2 != 0:
            raise ValueError("top-bottom frame height must be even")
    elif width % 2 != 0:
        raise ValueError("SBS frame width must be even")


def min_disparity_suffix(m: int) -> str:
    """what the depth cache key gains, after the temporal, range and fill suffixes, with a window other than [0, 64)"""
    return f"_mind{m}" if m != 0 else ""


class HipStereoBackend(HipBackend):
    """The product compute backend: PyTorch-ROCm buffers + libv3d_hip.so kernels."""

    def __init__(self, device: str = "cuda", sgbm_params: Optional[Dict] = None):
        super().__init__(device)
        self.sgbm_params = dict(sgbm_params or {})
        self._matcher = None
        self._geom = None

    def _get_matcher(self, W, H, n, min_disparity=0):
        g = self._geom
        if self._matcher is None or g[0] < W or g[1] < H or g[2] < n or g[3] != min_disparity:
            if self._matcher is not None:
                self._matcher.close()
            window = {"minDisparity": min_disparity} if min_disparity else {}
            self._matcher = self.native.StereoSGBM(W, H, n, device=self.device, **dict(self.sgbm_params, **window))
            self._geom = (W, H, n, min_disparity)
        return self._matcher

    def close_matcher(self):
        """destroy the matcher and its workspace (the next pass creates one): --min-disparity auto's calibration"""
        if self._matcher is not None:
            self._matcher.close()
        self._matcher = self._geom = None

    @staticmethod
    def _lockstep_ok(matcher) -> bool:
        """The lock-step SGM kernel needs all its workgroups resident at once; if another process is hogging the GPU
        its bounded spins give up and raise a flag.  Then the batch is recomputed with one launch per direction
        (still on the GPU, ~2x the SGM time, same bits) and the handle stays in that mode -- never a wrong disparity,
        never a CPU path."""
        n = matcher.sync_errors()
        if n == 0:
            return True
        print(f"warning: SGM lock-step kernel timed out waiting for neighbour strips ({n} workgroups): the GPU is "
              "over-subscribed; recomputing this batch and continuing with one launch per direction")
        matcher.set_lockstep(False)
        return False

    def _match(self, lg, rg, out=None, min_disparity=0):
        """gray [n,H,W] pairs -> int16 disparity x16 [n,H,W]; a pass whose lock-step kernel timed out is computed again.
        min_disparity m != 0: the matcher searches [m, m + 64) and its output is rebiased in place by -16 m, so valid values lie
        in [0, 1023] and invalid ones are -16 -- the form everything after the matcher reads"""
        n, H, W = lg.shape
        matcher = self._get_matcher(W, H, n, min_disparity)
        disp = matcher.compute(lg, rg, out)
        if not self._lockstep_ok(matcher):
            disp = matcher.compute(lg, rg, out)
            if matcher.sync_errors():
                raise RuntimeError("SGM kernels report time-outs with the lock-step pass off: device fault")
        if min_disparity:
            disp.sub_(16 * min_disparity)
        return disp

    def compute_batch_size(self, W: int, H: int, requested: int) -> int:
        """frames per device pass of the streaming path (process_video_sbs).  The caller's batch_size is list chunking
        in the reference (depth.py:448-461); here a pass should fill one lock-step SGM launch -- two workgroup slots per
        CU over the 128-column strips of a frame, 34 frames at 1080p -- because a smaller pass leaves CUs idle (batch 8:
        0.58 ms per frame, batch 34: 0.36).  Bounded by free HBM: the matcher's workspace is ~290 B per pixel."""
        torch = self.torch
        props = torch.cuda.get_device_properties(self.device)
        strips = max(1, -(-(W - 64) // 128))
        fill = max(1, (2 * props.multi_processor_count) // strips)
        free, _ = torch.cuda.mem_get_info(self.device)
        per_frame = 290 * W * H + 16 * W * H                     # workspace + staging / result tensors of this class
        fit = max(1, int(0.5 * free) // per_frame)
        if self._matcher is not None:                            # the workspace already allocated is not "free"
            fit = max(fit, self._geom[2])
        n = min(fill, fit)
        if requested > n:                                        # a caller asking for more gets whole launches
            n = min((requested // fill) * fill or requested, fit)
        return max(1, n)

    def split_sbs(self, sbs_frame: np.ndarray, unsqueeze: bool, input_layout: str = "sbs"):
        d = self.native.to_device(sbs_frame, self.device)
        L, R = (self.native.split_tb if input_layout == "tb" else self.native.split_sbs)(d, unsqueeze)
        return L.cpu().numpy(), R.cpu().numpy()

    def _depth_from(self, disp, monos, out=None):
        """disp16 [n,H,W] -> float32 depth: /16 + clamp (depth.py:341, 374), or, with monocular maps, the hybrid blend
        of depth.py:344-374 (maps of one shape go through one batched launch set)"""
        torch, nat = self.torch, self.native
        if monos is None:
            return nat.disp_to_depth(disp, out)
        if len(monos) != disp.shape[0]:
            raise ValueError(f"{len(monos)} monocular maps for {disp.shape[0]} frames")
        ms = [m if torch.is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)) for m in monos]
        ms = [m.to(self.device, torch.float32).contiguous() for m in ms]
        if any(m.dim() != 2 for m in ms):
            raise ValueError("monocular depth maps must be 2-D")
        if out is None:
            out = torch.empty(disp.shape, dtype=torch.float32, device=self.device)
        if len({tuple(m.shape) for m in ms}) == 1:
            nat.mono_blend(disp, torch.stack(ms), 0.7, 0.3, out)
        else:
            for i, m in enumerate(ms):
                nat.mono_blend(disp[i], m, 0.7, 0.3, out[i])
        return out

    def fill_holes(self, disp):
        """--fill-holes: the int16 disparity [n,H,W] of a pass, filled in place (v3d_fill_holes_disp16_batch); the row flags
        live in a staging buffer"""
        nat = self.native
        n, H, _ = disp.shape
        ws = self._staging("fill_ws", (max(16, nat.lib().v3d_fill_holes_ws_bytes(n, H)),), self.torch.uint8, False)
        return nat.fill_holes_disp16_batch(disp, out=disp, ws=ws)

    def pairs_to_disparity(self, pairs: List[Tuple[np.ndarray, np.ndarray]], monos=None, fill_holes: bool = False,
                           min_disparity: int = 0) -> List[np.ndarray]:
        """BGR (left, right) pairs -> float32 disparity maps (>= 0), depth.py:337-341 + 374 (+ 344-371 with `monos`);
        fill_holes: the matcher's invalid pixels are filled first (per frame, so this surface has it too)"""
        torch, nat = self.torch, self.native
        n = len(pairs)
        H, W = pairs[0][0].shape[:2]
        lg = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
        rg = torch.empty_like(lg)
        for i, (l, r) in enumerate(pairs):
            lg[i] = nat.bgr_to_gray(nat.to_device(l, self.device))
            rg[i] = nat.bgr_to_gray(nat.to_device(r, self.device))
        disp = self._match(lg, rg, min_disparity=min_disparity)
        if fill_holes:
            disp = self.fill_holes(disp)
        depth = self._depth_from(disp, monos)
        out = depth.cpu().numpy()
        return [out[i] for i in range(n)]

    def _sbs_to_gray(self, frames: List[np.ndarray], unsqueeze: bool, input_layout: str = "sbs"):
        """stereoscopic BGR frames -> (device frames [n,H,W,3], left gray, right gray [n,oh,ow]): the frames are gathered into one
        pinned buffer and cross PCIe in a single asynchronous copy, then one v3d_sbs_to_gray_batch launch -- v3d_tb_to_gray_batch
        for input_layout "tb", whose eyes are W x H unsqueezed and W x H/2 as stored.  The grays stay in the staging buffers
        `lg` / `rg` (left_gray, right_gray) until the next pass."""
        torch = self.torch
        n = len(frames)
        H, W = frames[0].shape[:2]
        check_frame_halves(W, H, check_input_layout(input_layout))
        ow, oh = sbs_eye_size({"width": W, "height": H}, unsqueeze, input_layout)
        dev = self._upload("sbs", frames, (H, W, 3), torch.uint8)
        lg = self._staging("lg", (n, oh, ow), torch.uint8, False)
        rg = self._staging("rg", (n, oh, ow), torch.uint8, False)
        (self.native.tb_to_gray_batch if input_layout == "tb" else self.native.sbs_to_gray_batch)(dev, unsqueeze, (lg, rg))
        return dev, lg, rg

    def sbs_to_disparity(self, frames: List[np.ndarray], unsqueeze: bool, mono_provider=None, fill_holes: bool = False,
                         min_disparity: int = 0, input_layout: str = "sbs"):
        """fused path: SBS BGR frames -> device float32 disparity [n,H,W] (no BGR halves materialised).
        Frames are gathered into one pinned buffer and cross PCIe in a single asynchronous copy (_sbs_to_gray).
        mono_provider (neural guidance on): called with the left views as RGB arrays, its maps are blended in.
        fill_holes: the int16 disparity is filled in place after the matcher (and its lock-step recompute), before /16 and the
        blend.
        min_disparity: the matcher's window [m, m + 64); the disparity is rebiased to [0, 64) right after it (_match).
        input_layout: "tb" reads top-bottom frames (the left eye on top); everything after the gray split is the same."""
        torch, nat = self.torch, self.native
        n = len(frames)
        dev, lg, rg = self._sbs_to_gray(frames, unsqueeze, input_layout)
        split = nat.split_tb if input_layout == "tb" else nat.split_sbs
        disp = self._match(lg, rg, self._staging("disp", tuple(lg.shape), torch.int16, False), min_disparity)
        if fill_holes:
            disp = self.fill_holes(disp)
        monos = None
        out = self._staging("depth", tuple(lg.shape), torch.float32, False)
        if mono_provider is not None:
            # a failing provider (DPT forward out of memory, bad shape ...) must not abort the clip -- nor, in a sharded run,
            # leave the other ranks waiting in the final barrier: warn and continue stereo-only like depth.py:367-369
            try:
                lefts = [split(dev[i], unsqueeze)[0].flip(-1).cpu().numpy() for i in range(n)]     # left view, RGB (depth.py:274)
                monos = mono_provider(lefts)
                return self._depth_from(disp, monos, out)
            except Exception as e:
                print(f"    Warning: Neural guidance failed, using stereo only: {e}")
        return self._depth_from(disp, None, out)

    # ---- frame matching (framematch.py; only called by --check-guide and the align CLI's video refinement) ----
    def frame_signatures(self, gray):
        """device luma planes u8 [n,H,W] -> their signatures [n,2304] on the device (v3d_frame_signature_batch)"""
        return self.native.frame_signature_batch(gray)

    def sbs_left_signatures(self, frames: List[np.ndarray], unsqueeze: bool, input_layout: str = "sbs"):
        """SBS (or top-bottom) BGR frames -> the signatures of their left views: the staging and the gray split of sbs_to_disparity,
        no matcher"""
        return self.native.frame_signature_batch(self._sbs_to_gray(frames, unsqueeze, input_layout)[1])

    def sbs_left_profiles(self, frames: List[np.ndarray], unsqueeze: bool, input_layout: str = "sbs"):
        """SBS (or top-bottom) BGR frames -> the column and row sums of their left views on the device (register.estimate): the
        staging and the gray split of sbs_left_signatures, then v3d_plane_profiles_batch"""
        return self.native.plane_profiles_batch(self._sbs_to_gray(frames, unsqueeze, input_layout)[1])

    def match_scores(self, prof_a, prof_b, cand, bins):
        """profiles [K,na] and [K,nb] on the device, a host-side candidate list int64 [C,2] -> the records int64 [K,C,6] as NumPy
        (one v3d_profile_match_scores call; the copy back synchronises: the search picks its next candidates from them)"""
        return self.native.profile_match_scores(prof_a, prof_b, cand, bins).cpu().numpy()

    def signature_scores(self, sig_a, sig_b):
        """signatures [na,2304] x [nb,2304] on the device -> a handle for read_scores: one v3d_signature_scores call, then the
        three small integer arrays go to pinned memory without blocking; an event marks the end of the copies"""
        return self._fetch_async(self.native.signature_scores(sig_a, sig_b))

    def guide_scores(self, rows, luma):
        """--check-guide: the kept signature rows of a batch's left views x the signatures of its 4K luma -> a read_scores handle"""
        return self.signature_scores(self.torch.stack(list(rows)), self.native.frame_signature_batch(luma))

    def read_scores(self, handle):
        """-> (num [na,nb], var_a [na], var_b [nb]) int64 NumPy.  After the stream's next synchronise the event has fired and
        nothing waits here"""
        return tuple(self._read(handle))

    # ---- quality report (quality.py; only called with --quality-report) ----
    def right_gray(self, n: int):
        """the right gray [n,H,W] of the latest sbs_to_disparity pass: a view of its staging buffer, like left_gray"""
        return self._bufs["rg"][:n]

    def last_disp16(self, n: int):
        """the int16 disparity [n,H,W] of the latest sbs_to_disparity pass, after --fill-holes when that is on (it fills in
        place): a view of the staging buffer the next pass overwrites"""
        return self._bufs["disp"][:n]

    def quality_reproj(self, n: int, bad_thr: int, min_disparity: int = 0):
        """reprojection records int64 [n,8] of the latest pass's planes, on the device (v3d_quality_reproj_batch); the partial
        records live in a staging buffer.  min_disparity m != 0: the pass's disparity is rebiased, so the entry sees the columns
        [0, W + m) of the left view against the right view moved by -m columns: the true match, and the baseline d = m"""
        nat = self.native
        lg = self.left_gray(n)
        ws = self._staging("quality_reproj_ws", (max(16, nat.lib().v3d_quality_reproj_ws_bytes(n, lg.shape[2] + min_disparity, lg.shape[1])),), self.torch.uint8, False)
        shift = {"right_shift": -min_disparity} if min_disparity else {}
        return nat.quality_reproj_batch(lg, self.right_gray(n), self.last_disp16(n), bad_thr, ws=ws, **shift)

    def min_disparity_score(self, frames: List[np.ndarray], unsqueeze: bool, min_disparity: int, input_layout: str = "sbs") -> int:
        """--min-disparity auto: the calibration frames through a matcher of their own at window m -> the number of pixels whose
        reprojection error stays within the report's default threshold, sum over frames of n_cmp - n_bad"""
        self.close_matcher()
        self.sbs_to_disparity(frames, unsqueeze, **({"min_disparity": min_disparity} if min_disparity else {}),
                              **({"input_layout": input_layout} if input_layout != "sbs" else {}))
        rec = self.quality_reproj(len(frames), MIN_DISPARITY_BAD, **({"min_disparity": min_disparity} if min_disparity else {})).cpu().numpy()
        self.close_matcher()
        return int((rec[:, 1] - rec[:, 4]).sum())

    def quality_flicker(self, depth, gray, still: int, jump16: int):
        """flicker records int64 [T-1,4] of the consecutive frames depth f32 / gray u8 [T,H,W], on the device
        (v3d_quality_flicker_batch)"""
        return self.native.quality_flicker_batch(depth, gray, still, jump16)

    def quality_fetch(self, records):
        """device records -> a handle for read_quality: the small integer array goes to pinned memory without blocking, an event
        marks the end of the copy (as signature_scores does)"""
        return self._fetch_async([records])

    def read_quality(self, handle, wait: bool = True):
        """-> int64 NumPy records, or None when the copy has not finished and wait is False.  After the stream's next
        synchronise the event has fired and nothing waits here"""
        got = self._read(handle, wait)
        return None if got is None else got[0]

    def depth_to_host(self, depth) -> np.ndarray:
        """device float32 [n,H,W] -> NumPy through a pinned block of its own (_fetch)"""
        return self._fetch(depth)

    def normalise_u16(self, depth) -> np.ndarray:
        nat = self.native
        d = depth if self.torch.is_tensor(depth) else nat.to_device(np.asarray(depth, np.float32), self.device)
        return nat.depth_to_u16(d.contiguous()).cpu().numpy().view(np.uint16)

    # ---- temporal stabilisation (temporal.py; only called with --temporal-radius > 0) ----
    def left_gray(self, n: int):
        """the left gray [n,H,W] of the latest sbs_to_disparity pass: a view of its staging buffer, which the next pass
        overwrites (temporal_concat copies it)"""
        return self._bufs["lg"][:n]

    def temporal_concat(self, held, new):
        """frames carried from earlier passes (or None) + the frames of this pass -> one private device buffer"""
        return new.clone() if held is None else self.torch.cat([held, new])

    def metric_lohi(self, n):
        """--depth-range metric: the constant range (0, 64) of n frames, a [n,2] device tensor written once per n"""
        from .temporal import METRIC_HI, METRIC_LO
        bufs = self.__dict__.setdefault("_bufs", {})
        lohi = bufs.get(("metric_lohi", n))
        if lohi is None:
            lohi = bufs[("metric_lohi", n)] = self.torch.tensor([[METRIC_LO, METRIC_HI]] * n, dtype=self.torch.float32, device=self.device)
        return lohi

    def depth_to_u16_metric(self, depth):
        """--depth-range metric without a radius: device float32 depth [n,H,W] -> device u16 samples (int16-viewed) [n,H,W] against
        the constant range (0, 64): one launch, no reduction"""
        return self.native.depth_to_u16_range_batch(depth, self.metric_lohi(len(depth)))

    def temporal_stabilize(self, depth, gray, t0, n, radius, tau, cut_threshold, fill, range_quantile=10000, observe=None,
                           motion_search=0, metric=False):
        """buffer of T frames (device depth f32 and left gray u8 [T,H,W]) -> device u16 samples (int16-viewed) [n,H,W] of
        targets t0 .. t0+n-1: cuts, per-frame min/max, clip-stable range, filter, normalisation -- nine launches on the
        current stream, nothing comes back to the host.  range_quantile < 10000: the per-frame max is the robust white point
        (three launches in place of the min/max's three).  observe (--quality-report): called with the filtered depth and the
        targets' gray before the normalisation.  motion_search > 0 (--temporal-motion): the block matcher's fields and the cuts
        of its residual (three launches in place of the cuts' three) and the compensated filter in place of the filter.  metric
        (--depth-range metric): the constant range (0, 64) in place of the min/max and the window's range (four launches fewer)"""
        nat = self.native
        if motion_search > 0:
            fwd, bwd, _, cut = nat.temporal_motion(gray, motion_search, cut_threshold)
        else:
            cut = nat.temporal_cuts(gray, cut_threshold)
        if metric:
            lohi = self.metric_lohi(n)
        else:
            mm = nat.depth_robust_minmax_batch(depth, range_quantile) if range_quantile < 10000 else nat.depth_minmax_batch(depth)
            lohi = nat.temporal_range(mm, cut, radius, t0, n)
        if motion_search > 0:
            filt = nat.temporal_filter_mc_batch(depth, gray, radius, tau, cut, fwd, bwd, fill, t0, n)
        else:
            filt = nat.temporal_filter_batch(depth, gray, radius, tau, cut, fill, t0, n)
        if observe is not None:
            observe(filt, gray[t0:t0 + n])
        return nat.depth_to_u16_range_batch(filt, lohi)

    def depth_to_u16_batch(self, depth):
        """device float32 depth [n,H,W] -> device u16 samples (int16-viewed) [n,H,W], every frame against its own min and max:
        frame f is what normalise_u16 gives for it alone"""
        return self.native.depth_to_u16_batch(depth)

    def depth_to_u16_robust(self, depth, range_quantile):
        """--range-percentile without a radius: device float32 depth [n,H,W] -> device u16 samples (int16-viewed) [n,H,W], every
        frame against its own (min, robust white point)"""
        nat = self.native
        return nat.depth_to_u16_range_batch(depth, nat.depth_robust_minmax_batch(depth, range_quantile))

    def to_host_u16(self, u16):
        """device u16 [n,H,W] -> NumPy uint16 [n,H,W] through pinned memory.  The pinned block comes from torch's caching host
        allocator and goes back to it once the writers drop the last frame of it: no allocation in the steady state, and no
        buffer is overwritten while a writer thread still encodes from it."""
        return self._fetch(u16).view(np.uint16)

    def png_streams_u16(self, u16):
        """--png-encoder gpu: device u16 samples (int16-viewed) [n,H,W] -> the zlib streams of their 16-bit PNGs, deflated on
        the device (png_gpu.DevicePngEncoder); only the streams cross PCIe"""
        return self._png_encoder().encode(u16)


def sbs_eye_size(video_info, unsqueeze: bool, input_layout: str = "sbs") -> Tuple[int, int]:
    """(width, height) of one eye as the matcher sees it (HybridStereoDepthExtractor.eye_size, for a caller without an extractor):
    the frame's own size once the eyes are unsqueezed, else half of it along the packed axis"""
    if input_layout == "tb":
        return video_info['width'], video_info['height'] if unsqueeze else video_info['height'] // 2
    return video_info['width'] if unsqueeze else video_info['width'] // 2, video_info['height']


class HybridStereoDepthExtractor:
    """ GPU-accelerated depth extraction from SBS video using hybrid stereo matching + neural guidance """

    # where the 16-bit maps of process_video_sbs go: anything with PngWriterPool's submit(path, uint16 image) / context-
    # manager surface (bench.py swaps in a raw sink to time the path without zlib)
    writer_pool_factory = PngWriterPool

    def __init__(self,
                 model_checkpoint: str = "Intel/dpt-large",
                 work_dir: str = "temp_depth",
                 cache_dir: str = "temp_depth",
                 device: str = "cuda",
                 batch_size: int = 8,
                 use_neural_guidance: bool = True,
                 stereo_only: bool = False,
                 unsqueeze_sbs: bool = True,
                 backend=None,
                 mono_provider=None,
                 temporal_radius: int = 0,
                 temporal_tau: int = 12,
                 temporal_cut: int = 20,
                 temporal_fill: bool = True,
                 range_percentile: float = 100.0,
                 fill_holes: bool = False,
                 png_encoder: str = "zlib",
                 quality_report=None,
                 quality_bad_threshold: int = 16,
                 quality_still: int = 4,
                 quality_jump: float = 1.0,
                 temporal_motion: int = 0,
                 min_disparity=0,
                 depth_range: str = "frame",
                 input_layout: str = "sbs"):
        """ mono_provider: optional callable(list of HxWx3 uint8 RGB left views) -> list of 2-D float32 monocular
        depth maps (NumPy arrays or device tensors, any size); takes the place of the DPT forward of depth.py:348-350.
        temporal_radius > 0 (process_video_sbs only): temporal stabilisation over 2R+1 frames (temporal.py); 0 = every frame
        on its own, the reference's behaviour.  temporal_motion > 0 (needs a radius): the window follows the motion a block
        matcher finds, search radius in pixels per frame step.  process_frame_batch / save_depth_map stay per-frame: a list of pairs is not a clip.
        range_percentile < 100 (process_video_sbs only): the white point of the 16-bit normalisation is that percentile of the
        valid disparities instead of the maximum; 100 = the reference's min-max.
        fill_holes (every surface, process_frame_batch included: it is per frame): the matcher's invalid pixels are filled from
        their scanline neighbours on the int16 disparity, before /16 and everything after it; off = they stay depth 0
        png_encoder (process_video_sbs only): "gpu" deflates the 16-bit maps on the device (png_gpu.py); "zlib" = on the writer
        threads, as ever
        quality_report (process_video_sbs and the one-pass pipeline): True or a path measures the run's depth on the device without
        ground truth (quality.py) and writes quality.json next to the depth maps or to the path; quality_*: its thresholds.  No
        output and no cache key changes
        min_disparity (every surface): m in [-64, 0], the matcher searches disparities [m, m + 64) -- content behind the screen
        plane has d < 0 -- and the result is rebiased to [0, 64): larger still means nearer, and the far end of the window
        (rel = 0) is dropped like d = 0 is at m = 0 (depth.py:374).  "auto" (process_video_sbs and the one-pass pipeline)
        calibrates m on frames of the clip (resolve_min_disparity).  0 = the reference's window: no call, key or byte changes
        depth_range (process_video_sbs and the one-pass pipeline): "metric" normalises every frame against the constant range
        (0, 64) instead of its own (or its window's) minimum and maximum: a sample s is a rebiased disparity of 64 s / 65535 pixels
        of the matcher's eye.  "frame" = the reference's min-max: no call, key or byte changes
        input_layout (every surface that takes a packed frame): "tb" reads a top-bottom clip, the left eye on top; unsqueeze_sbs then
        stretches the eyes vertically.  "sbs" = the reference's layout: no call, key or byte changes """
        self.input_layout = check_input_layout(input_layout)
        self.min_disparity = check_min_disparity(min_disparity)
        self.min_disparity_scores = None         # {candidate: score} of an `auto` run, once resolved
        from .png_gpu import check_png_encoder
        self.png_encoder = check_png_encoder(png_encoder)
        from .temporal import check_motion_search, check_parameters, check_range_percentile
        self.temporal = check_parameters(temporal_radius, temporal_tau, temporal_cut, temporal_fill)
        self.motion_search = check_motion_search(temporal_motion, self.temporal[0])
        self.range_quantile = check_range_percentile(range_percentile)
        from .temporal import check_depth_range
        self.depth_range = check_depth_range(depth_range, self.range_quantile)
        self.eye_width = None                    # the matcher's image width of the run in progress (--depth-range metric)
        if self.depth_range == "metric" and not fill_holes:
            print("Warning: --depth-range metric without --fill-holes: invalid pixels sit at the far end of the search window")
        if not isinstance(fill_holes, (bool, np.bool_)):
            raise ValueError(f"fill_holes must be a bool, got {fill_holes!r}")
        self.fill_holes = bool(fill_holes)
        from .quality import check_parameters as check_quality
        if quality_report is not None and not isinstance(quality_report, (bool, np.bool_, str, Path)):
            raise ValueError(f"quality_report must be None, a bool or a path, got {quality_report!r}")
        self.quality_report = quality_report if quality_report else None
        self.quality_params = check_quality(quality_bad_threshold, quality_still, quality_jump, self.temporal[2])
        self.quality_jump = float(quality_jump)
        self.quality = None                      # quality.QualityMonitor of the run in progress (--quality-report)

        self.device = device
        self.work_dir = create_work_directory(work_dir)
        self.cache_dir = create_work_directory(cache_dir)
        self.batch_size = batch_size
        self.model_checkpoint = model_checkpoint
        self.use_neural_guidance = use_neural_guidance
        self.stereo_only = stereo_only
        self.unsqueeze_sbs = unsqueeze_sbs

        # `backend` exists so host-logic tests can run without a GPU; the product always builds the HIP one
        if backend is None:
            require_hip_device(device)
            backend = HipStereoBackend(device)
        self.backend = backend

        print(f"Initializing Hybrid Stereo depth extractor...")
        print(f"Device: {self.device}")
        print(f"Model: {self.model_checkpoint if not self.stereo_only else 'Stereo-only mode'}")
        print(f"Batch size: {self.batch_size}")
        print(f"Neural guidance: {self.use_neural_guidance and not self.stereo_only}")

        self.model = None
        self.processor = None
        self.mono_provider = mono_provider
        self.guide_check = None                  # framematch.GuideChecker of the one-pass pipeline's --check-guide
        self.model_loaded = False
        self.max_vram_usage = 0.9
        self.memory_stats = defaultdict(float)

    def load_model(self):
        """ Load depth estimation model (depth.py:60-114).  Offline by construction: a local directory, a model already in
        the HF cache, or a provider handed to the constructor; anything else falls back like depth.py:107-114 """
        if self.model_loaded:
            return
        if self.stereo_only:
            print("Using stereo-only mode (no neural network)")
            self.model_loaded = True
            return
        if self.mono_provider is not None:
            print("Using the supplied monocular depth provider for neural guidance")
            self.model_loaded = True
            return
        print(f"Loading depth model: {self.model_checkpoint}")
        try:
            from transformers import DPTForDepthEstimation, DPTImageProcessor
            print("Loading DPT model for neural depth guidance")
            self.processor = DPTImageProcessor.from_pretrained(self.model_checkpoint, local_files_only=True)
            self.model = DPTForDepthEstimation.from_pretrained(self.model_checkpoint, local_files_only=True)
            dev = getattr(self.backend, "device", self.device)
            self.model = self.model.to(dev)
            self.model.eval()
            self.mono_provider = self._dpt_provider
            self.model_loaded = True
            print("✓ Model loaded successfully")
        except ImportError:
            print("Warning: transformers library not available, falling back to stereo-only mode")
            self.stereo_only = True
            self.model_loaded = True
        except Exception as e:
            print(f"Warning: Failed to load neural model, falling back to stereo-only mode: {e}")
            self.stereo_only = True
            self.model_loaded = True

    def _dpt_provider(self, left_rgb_frames):
        """ depth.py:283-293 + 346-350: DPT forward on the left view; the predicted depth stays on the device """
        import torch
        dev = next(self.model.parameters()).device
        out = []
        with torch.no_grad():
            for rgb in left_rgb_frames:
                inputs = self.processor(images=rgb, return_tensors="pt")
                inputs = {k: v.to(dev) for k, v in inputs.items()}
                out.append(self.model(**inputs).predicted_depth[0].float())
        return out

    def _disparity_pass(self, call, *args, guidance=None, packed=False):
        """the one way a disparity pass of the backend (sbs_to_disparity, pairs_to_disparity) is called: an option that is off
        adds no argument -- no provider / monocular maps without guidance, no `fill_holes` keyword without --fill-holes -- so
        it stays the call every backend knows.  packed: the pass takes packed frames (sbs_to_disparity), so a top-bottom clip adds
        its `input_layout`"""
        if guidance is not None:
            args += (guidance,)
        window = {"min_disparity": self.min_disparity} if self.min_disparity != 0 else {}
        return call(*args, **({"fill_holes": True} if self.fill_holes else {}), **window, **(self._layout_keyword() if packed else {}))

    def _layout_keyword(self) -> dict:
        """what a backend call that takes packed frames gains with a top-bottom clip: nothing with an SBS one"""
        return {"input_layout": self.input_layout} if self.input_layout != "sbs" else {}

    def resolve_min_disparity(self, video_path: str, start_frame: int, frame_count: int) -> int:
        """--min-disparity auto -> its integer, before anything is keyed by it: every candidate window scores the calibration
        frames by reprojection (backend.min_disparity_score), choose_min_disparity picks.  Under torchrun every rank decodes
        the same frames and reaches the same integer: no collective"""
        if self.min_disparity != "auto":
            return self.min_disparity
        if frame_count < 1:
            self.min_disparity = 0
            return 0
        picks = calibration_frames(start_frame, frame_count)
        stride = picks[1] - picks[0] if len(picks) > 1 else 1
        frames = list(iter_frames(video_path, picks[0], (len(picks) - 1) * stride + 1, stride=stride))
        scores = {m: int(self.backend.min_disparity_score(frames, self.unsqueeze_sbs, m, **self._layout_keyword())) for m in MIN_DISPARITY_CANDIDATES} if frames else \
                 {m: 0 for m in MIN_DISPARITY_CANDIDATES}
        self.min_disparity = choose_min_disparity(scores)
        self.min_disparity_scores = {str(m): s for m, s in scores.items()}
        print(f"--min-disparity auto: calibrated on frames {picks}")
        print("  " + "  ".join(f"m={m}: {s}" for m, s in scores.items()) + f"  -> {self.min_disparity}")
        return self.min_disparity

    def manifest_extra(self) -> dict:
        """what the options that are on add to the one-pass pipeline's manifest (none: nothing); write_side_files puts the
        same entries next to the depth maps"""
        from .temporal import manifest_entry
        extra = {}
        if self.temporal[0] > 0 or self.range_quantile < 10000:
            extra["temporal"] = manifest_entry(*self.temporal, self.range_quantile, self.motion_search)
        if self.fill_holes:
            extra["fill_holes"] = True
        if self.input_layout != "sbs":
            extra["input_layout"] = self.input_layout
        if self.min_disparity != 0 or self.min_disparity_scores is not None:
            extra["min_disparity"] = self.min_disparity
        if self.min_disparity_scores is not None:
            extra["min_disparity_scores"] = self.min_disparity_scores
        if self.depth_range == "metric":
            from .temporal import METRIC_HI, METRIC_LO
            extra["depth_range"] = {"mode": "metric", "lo": METRIC_LO, "hi": METRIC_HI, "min_disparity": self.min_disparity,
                                    "eye_width": self.eye_width}
        if self.guide_check is not None and self.guide_check.summary is not None:
            extra["guide_match"] = self.guide_check.summary
        if self.quality is not None and self.quality.summary is not None:
            extra["quality"] = self.quality.summary
        return extra

    def start_quality(self, world: int, owned=None):
        """--quality-report: the monitor of one run, created by the driver (None when the flag is off)"""
        self.quality = None
        if self.quality_report is not None:
            from .quality import QualityMonitor
            stage = "matcher+fill" if self.fill_holes else "matcher"
            bad, still, _, cut = self.quality_params
            window = {"min_disparity": self.min_disparity} if self.min_disparity != 0 else {}
            self.quality = QualityMonitor(self.backend, bad, still, self.quality_jump, cut, consecutive=world == 1, reproj_stage=stage,
                                          flicker_stage="hybrid blend" if self._guidance_provider() is not None else stage, owned=owned,
                                          **window)
        return self.quality

    def finish_quality(self, default_dir, rank: int = 0):
        """after the last pass: totals over the ranks, the printed summary and quality.json (rank 0) in default_dir or at the
        flag's path; the manifest entry is ready afterwards"""
        from . import sharding
        if self.quality is None:
            return None
        self.quality.finish(sharding.total)
        if rank != 0:
            return None
        self.quality.report()
        path = Path(default_dir) / "quality.json" if isinstance(self.quality_report, (bool, np.bool_)) else Path(self.quality_report)
        print(f"✓ Quality report: {self.quality.write(path)}")
        return path

    def quality_skipped(self):
        """a run that reuses existing output measures nothing: say so"""
        if self.quality_report is not None:
            from .quality import CACHED_NOTE
            print(CACHED_NOTE)

    def write_side_files(self, cache_path: Path):
        """temporal.json (a radius or the robust range is on), fill.json (--fill-holes), min_disparity.json (--min-disparity),
        depth_range.json (--depth-range metric) and input_layout.json (--input-layout tb) of a depth map directory"""
        import json
        extra = self.manifest_extra()
        if "temporal" in extra:
            (cache_path / "temporal.json").write_text(json.dumps(extra["temporal"]))
        if "fill_holes" in extra:
            (cache_path / "fill.json").write_text(json.dumps({"fill_holes": True}))
        if "min_disparity" in extra:
            (cache_path / "min_disparity.json").write_text(json.dumps({k: extra[k] for k in ("min_disparity", "min_disparity_scores") if k in extra}))
        if "depth_range" in extra:
            (cache_path / "depth_range.json").write_text(json.dumps(extra["depth_range"]))
        if "input_layout" in extra:
            (cache_path / "input_layout.json").write_text(json.dumps({"input_layout": extra["input_layout"]}))

    def _guidance_provider(self):
        """ the provider when neural guidance is active (depth.py:344-345), else None """
        if self.use_neural_guidance and not self.stereo_only and self.mono_provider is not None:
            return self.mono_provider
        return None

    def get_cache_path(self, video_path: str, frame_start: int, frame_count: int) -> Path:
        """ Generate cache path for depth maps (key format identical to depth.py:119-120; with temporal stabilisation or the
        robust range on, the key also carries their parameters, so such maps and the reference's never share a directory; so
        does a search window other than [0, 64): the resolved integer, which an `auto` run and an explicit one share; a top-bottom
        clip appends its layout last: the key of an SBS run is byte for byte what it was) """
        if self.min_disparity == "auto":
            raise ValueError('min_disparity="auto" is resolved from the clip first (resolve_min_disparity)')
        from .temporal import cache_suffix, depth_range_suffix, fill_suffix
        cache_key = f"{video_path}_{frame_start}_{frame_count}_{self.model_checkpoint}_{self.unsqueeze_sbs}"
        cache_key += cache_suffix(*self.temporal, self.range_quantile, self.motion_search) + fill_suffix(self.fill_holes)
        cache_key += min_disparity_suffix(self.min_disparity) + depth_range_suffix(self.depth_range) + input_layout_suffix(self.input_layout)
        cache_hash = hashlib.md5(cache_key.encode()).hexdigest()[:16]
        cache_subdir = self.cache_dir / f"depth_{cache_hash}"
        cache_subdir.mkdir(exist_ok=True)
        return cache_subdir

    def is_cached(self, cache_path: Path, frame_count: int) -> bool:
        """ Check if depth maps are already cached """
        if not cache_path.exists():
            return False
        expected_files = [cache_path / f"depth_{i:06d}.png" for i in range(frame_count)]
        all_exist = all(f.exists() for f in expected_files)
        if all_exist:
            print(f"✓ Found cached depth maps: {cache_path}")
            return True
        return False

    def _frame_count(self, video_path, start_frame, max_frames):
        video_info = get_video_info(video_path)
        if not video_info:
            raise ValueError(f"Could not read video info: {video_path}")
        total_frames = video_info.get('frames', 0) or int(video_info['duration'] * video_info['fps'])
        if max_frames is None:
            n = total_frames - start_frame
        else:
            n = min(max_frames, total_frames - start_frame)
        return video_info, n

    def extract_frames_opencv(self, video_path: str, start_frame: int = 0, max_frames: int = None) -> List[np.ndarray]:
        """ Extract video frames (kept for API compatibility; process_video_sbs streams instead) """
        print(f"Extracting frames from {video_path}...")
        _, max_frames = self._frame_count(video_path, start_frame, max_frames)
        print(f"Extracting {max_frames} frames starting from frame {start_frame}")
        try:
            frames = list(iter_frames(video_path, start_frame, max_frames))
        except ValueError:
            raise
        except Exception as e:
            raise RuntimeError(f"Frame extraction failed: {e}")
        print(f"✓ Extracted {len(frames)} frames")
        return frames

    extract_frames_ffmpeg = extract_frames_opencv

    def split_sbs_frame(self, sbs_frame: np.ndarray, unsqueeze: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """ Split side-by-side (input_layout "tb": top-bottom) frame into left and right images """
        height, width = sbs_frame.shape[:2]
        check_frame_halves(width, height, self.input_layout)
        return self.backend.split_sbs(np.ascontiguousarray(sbs_frame), unsqueeze, **self._layout_keyword())

    def preprocess_frame_pair(self, left_frame: np.ndarray, right_frame: np.ndarray) -> Dict:
        """ Preprocess frame pair for depth estimation (BGR -> RGB views; the provider does its own input processing) """
        if left_frame.shape[2] == 3:
            left_rgb, right_rgb = left_frame[..., ::-1], right_frame[..., ::-1]
        else:
            left_rgb, right_rgb = left_frame, right_frame
        return {'stereo_pair': {'left': left_rgb, 'right': right_rgb}}

    def process_frame_batch(self, frame_pairs: List[Tuple[np.ndarray, np.ndarray]]) -> List[np.ndarray]:
        """ Process batch of BGR frame pairs -> list of HxW float32 disparity maps (>= 0) """
        check_min_disparity(self.min_disparity, allow_auto=False)        # a list of pairs is not a clip
        if not self.model_loaded:
            self.load_model()
        batch_size = len(frame_pairs)
        print(f"Processing batch of {batch_size} frame pairs...")
        if batch_size == 0:
            return []
        try:
            monos = None
            provider = self._guidance_provider()
            if provider is not None:
                try:
                    monos = provider([np.ascontiguousarray(l[..., ::-1]) for l, _ in frame_pairs])     # left views as RGB (depth.py:274)
                except Exception as e:                       # depth.py:367-369
                    print(f"    Warning: Neural guidance failed, using stereo only: {e}")
            depth_maps = self._disparity_pass(self.backend.pairs_to_disparity, frame_pairs, guidance=monos)
        except Exception as e:
            print(f"Error processing frame batch: {e}")
            raise
        print(f"✓ Processed {len(depth_maps)} depth maps")
        return depth_maps

    def save_depth_map(self, depth_map: np.ndarray, output_path: Path):
        """ Save depth map as 16-bit PNG (per-frame min-max normalisation, depth.py:399-403) """
        write_png16(output_path, self.backend.normalise_u16(depth_map))

    def process_video_sbs(self,
                          video_path: str,
                          start_frame: int = 0,
                          max_frames: int = None,
                          force_reprocess: bool = False) -> Path:
        """ Process entire SBS video to extract depth maps """
        from . import sharding

        print(f"Processing SBS video: {video_path}")
        video_info, frame_count = self._frame_count(video_path, start_frame, max_frames)
        print(f"Video info: {video_info['width']}x{video_info['height']} @ {video_info['fps']:.1f}fps")
        print(f"Processing {frame_count} frames starting from frame {start_frame}")

        self.resolve_min_disparity(video_path, start_frame, frame_count)
        cache_path = self.get_cache_path(video_path, start_frame, frame_count)
        if not force_reprocess and self.is_cached(cache_path, frame_count):
            print("✓ Using cached depth maps")
            self.quality_skipped()
            return cache_path
        check_frame_halves(video_info['width'], video_info['height'], self.input_layout)
        if not self.model_loaded:
            self.load_model()

        rank, world = sharding.rank_world()
        sharding.require_initialized(world)                  # WORLD_SIZE > 1 without a process group would race the cache dir
        written = 0
        # PNG compression (zlib) costs ~20 ms per 1080p map on one core, the GPU path 0.5 ms: the maps of a pass go to
        # a bounded pool of writer threads and compress while the next pass is decoded and computed
        with self.writer_pool_factory() as writers:
            for idx, u16 in self.iter_depth_u16(video_path, start_frame, frame_count, video_info, rank, world):
                self.submit_depth_maps(writers, cache_path, idx, u16)
                written += len(idx)
                print(f"✓ Queued batch depth maps ({written} on rank {rank})")
        if sharding.total(written) == 0:
            raise ValueError("No frames extracted from video")
        self.finish_quality(cache_path, rank)
        if rank == 0:
            self.write_side_files(cache_path)
        sharding.barrier()

        print(f"✓ Depth extraction complete: {cache_path}")
        print(f"  Processed {written} frames")
        print(f"  Output directory: {cache_path}")
        return cache_path

    def submit_depth_maps(self, writers, cache_path: Path, idx, u16):
        """the u16 samples of frames idx -> depth_%06d.png through the writer pool.  Every map crosses in a pinned block of its
        own, which goes back to the allocator once that map is written; a whole pass in one block stays pinned until its last
        map is, and the next pass has to pin a second one (20 ms at 1080p)"""
        if self.png_encoder == "gpu":                 # the pass is deflated on the device; the writers wrap and write
            from .png_gpu import gray16_file
            wrap = gray16_file(u16.shape[2], u16.shape[1])
            for frame_idx, stream in zip(idx, self.backend.png_streams_u16(u16)):
                writers.submit(cache_path / f"depth_{frame_idx:06d}.png", stream, encode=wrap)
            return
        to_host = getattr(self.backend, "to_host_u16", lambda planes: planes)     # per-frame surface only: they are NumPy already
        for j, frame_idx in enumerate(idx):
            writers.submit(cache_path / f"depth_{frame_idx:06d}.png", to_host(u16[j:j + 1])[0])

    def eye_size(self, video_info) -> Tuple[int, int]:
        """(width, height) of the matcher's eye: the packed frame's own size once the eyes are unsqueezed, else half of it along the
        packed axis"""
        return sbs_eye_size(video_info, self.unsqueeze_sbs, **self._layout_keyword())

    def pass_frames(self, video_info) -> int:
        """frames per device pass: decoupled from batch_size (which the reference only uses to chunk its frame list,
        depth.py:448-461) -- a pass fills one lock-step SGM launch whatever the caller's chunk size is"""
        sizer = getattr(self.backend, "compute_batch_size", None)
        return sizer(*self.eye_size(video_info), self.batch_size) if sizer else self.batch_size

    def frame_plan(self, frame_count: int, rank: int, world: int):
        """(decoded, owned, block) of one rank: `decoded` is the iter_frames range (first, count, stride, offset), relative to
        start_frame, that the rank decodes and matches, `owned` the range in the same form of the frames it writes.
        Per frame, frame i goes to rank i mod world: every rank seeks to and decodes ONLY its own frames, so the decode (the
        scaling limiter once the kernels are fast) is divided by the world size, not replicated; block is None.
        With --temporal-radius round-robin frames have no neighbours: a rank owns a contiguous block and also decodes a halo of
        `radius` frames on each side (sharding.temporal_block); block is BlockStabilizer's (first, count, halo_before)."""
        from . import sharding
        if self.temporal[0] == 0:
            share = (0, frame_count, world, rank)
            return share, share, None
        first, count, hb, ha = sharding.temporal_block(frame_count, rank, world, self.temporal[0])
        return (first - hb, hb + count + ha, 1, 0), (first, count, 1, 0), (first, count, hb)

    def iter_depth_u16(self, video_path, start_frame, frame_count, video_info, rank, world):
        """The streaming driver of the depth CLI and the one-pass pipeline: decodes this rank's frames of the clip (frame_plan),
        matches them a device pass at a time and yields (clip frame indices, the backend's u16 samples [n,H,W]) of the frames
        the rank owns: per pass, or -- with --temporal-radius -- `radius` frames behind the matcher with the tail at the end."""
        be = self.backend
        self.last_pass_frames = pass_frames = self.pass_frames(video_info)
        self.eye_width = self.eye_size(video_info)[0]
        metric = self.depth_range == "metric"
        (first, count, stride, offset), _, block = self.frame_plan(frame_count, rank, world)
        # --quality-report: a rank's halo frames are matched twice in a block-sharded run; only the owner's records count
        quality = self.start_quality(world, None if block is None else range(block[0], block[0] + block[1]))
        stab = None
        if block is not None:
            from .temporal import BlockStabilizer
            observe = {"observe": quality.note_stabilised} if quality is not None and world == 1 else {}
            motion = {"motion_search": self.motion_search} if self.motion_search > 0 else {}
            stab = BlockStabilizer(be, self.temporal, *block, self.range_quantile, **observe, **motion, **({"metric": True} if metric else {}))
        frames = iter_frames(video_path, start_frame + first, count, stride=stride, offset=offset) if count else iter(())
        provider = self._guidance_provider()
        self.last_decoded_frames = 0

        def staged():
            """(indices, u16 samples) of what each pass completes; ([], None) when the stabiliser's window is not full yet"""
            for batch in iter(lambda: list(islice(frames, pass_frames)), []):
                k0 = self.last_decoded_frames
                self.last_decoded_frames += len(batch)
                idx = [first + offset + k * stride for k in range(k0, k0 + len(batch))]       # the pass's clip indices
                depth = self._disparity_pass(be.sbs_to_disparity, batch, self.unsqueeze_sbs, guidance=provider, packed=True)
                if quality is not None:                  # --quality-report: the pass's planes are valid until the next pass
                    quality.note_pass(idx, len(batch), depth)
                if self.guide_check is not None:         # --check-guide: the pass's left gray planes are valid until the next pass
                    self.guide_check.note_left(idx, be.left_gray(len(batch)))
                if stab is not None:
                    yield stab.push(depth, be.left_gray(len(batch)))
                    continue
                if metric:                               # --depth-range metric: the constant range, no reduction
                    yield idx, be.depth_to_u16_metric(depth)
                elif self.range_quantile < 10000:        # --range-percentile: every frame against its own robust white point
                    yield idx, be.depth_to_u16_robust(depth, self.range_quantile)
                elif hasattr(be, "depth_to_u16_batch"):
                    yield idx, be.depth_to_u16_batch(depth)
                else:                                    # a backend with the per-frame surface only: the same samples, on the host
                    yield idx, np.stack([be.normalise_u16(d) for d in depth])
            if stab is not None:
                yield stab.finish()

        for idx, u16 in staged():
            if idx:
                yield idx, u16


# run_pipeline.py:12,63 and reference __init__.py:6 import this name
IGEVStereoDepthExtractor = HybridStereoDepthExtractor


def add_depth_arguments(parser, force_help: str):
    """the options of the depth path, shared by the depth CLI and the one-pass pipeline (--force means something else in each)"""
    from .png_gpu import add_png_arguments
    from .quality import add_quality_arguments
    from .temporal import add_depth_range_arguments, add_fill_arguments, add_range_arguments, add_temporal_arguments
    parser.add_argument('--start-frame', type=int, default=0, help='Starting frame number (default: 0)')
    parser.add_argument('--max-frames', type=int, default=None, help='Maximum number of frames to process (default: all)')
    parser.add_argument('--batch-size', type=int, default=8, help='Batch size for GPU processing (default: 8)')
    parser.add_argument('--model', default="Intel/dpt-large", help='Neural model checkpoint (default: Intel/dpt-large)')
    parser.add_argument('--work-dir', default='temp_depth', help='Working directory for output (default: temp_depth)')
    parser.add_argument('--force', action='store_true', help=force_help)
    parser.add_argument('--device', default='cuda', help='Processing device (default: cuda)')
    parser.add_argument('--stereo-only', action='store_true', help='Use stereo matching only (no neural guidance)')
    parser.add_argument('--no-neural', action='store_true', help='Disable neural guidance (same as --stereo-only)')
    parser.add_argument('--no-unsqueeze', action='store_true', help='Skip SBS unsqueezing (keep squeezed aspect ratio)')
    add_input_layout_argument(parser)
    add_temporal_arguments(parser)
    add_range_arguments(parser)
    add_depth_range_arguments(parser)
    add_fill_arguments(parser)
    parser.add_argument('--min-disparity', type=min_disparity_argument, default=0, metavar='M|auto',
                        help='Search disparities [M, M + 64) instead of [0, 64), M in [-64, 0]: content behind the screen plane of '
                             'a stereoscopic film has negative disparity.  The result is rebiased to [0, 64), so larger still means '
                             'nearer.  auto: calibrate M on up to 8 frames of the clip by reprojection error (default: 0)')
    add_png_arguments(parser)
    add_quality_arguments(parser)


def depth_options(args) -> dict:
    """parsed add_depth_arguments -> the keyword arguments HybridStereoDepthExtractor and SbsTo4kDepthPipeline share"""
    from .png_gpu import png_options
    from .quality import quality_options
    from .temporal import depth_range_options, fill_options, range_options, temporal_options
    stereo_only = args.stereo_only or args.no_neural
    return dict(model_checkpoint=args.model, work_dir=args.work_dir, device=args.device, batch_size=args.batch_size,
                use_neural_guidance=not stereo_only, stereo_only=stereo_only, unsqueeze_sbs=not args.no_unsqueeze,
                **temporal_options(args), **range_options(args), **fill_options(args), **png_options(args),
                **quality_options(args), **({"min_disparity": args.min_disparity} if args.min_disparity != 0 else {}),
                **depth_range_options(args), **input_layout_options(args))


def main(argv=None):
    """ Command line interface for depth extraction """
    parser = argparse.ArgumentParser(description='Extract depth maps from SBS stereoscopic video')
    parser.add_argument('video', help='Path to SBS video file')
    add_depth_arguments(parser, 'Force reprocessing even if cached results exist')
    args = parser.parse_args(argv)

    try:
        from . import sharding
        sharding.init_process_group()            # no-op for one process; under torchrun: one rank per GPU (sets the device)
        extractor = HybridStereoDepthExtractor(cache_dir=args.work_dir, **depth_options(args))
        output_path = extractor.process_video_sbs(video_path=args.video, start_frame=args.start_frame,
                                                  max_frames=args.max_frames, force_reprocess=args.force)
        print(f"\n✓ Success! Depth maps saved to: {output_path}")
    except Exception as e:
        print(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    exit(main())
