"""Step 4 of the pipeline: the 4K frame and its 4K depth -> side-by-side 3D (`python -m video_3d_pipeline.convert`).

The reference declares this step as the console script `video-3d-convert = "video_3d_pipeline.convert:main"` and hands the
work to an outside tool (VisionDepth3D, "Optimized DIBR rendering").  Here it is depth-image-based rendering on the device,
v3d_render_stereo_batch: every source pixel moves horizontally by g/256 * (D - conv)/65536 pixels per eye, the nearest
source wins, disocclusions take the farther neighbour (background extension), and the two eyes are packed as full or half
side-by-side.  The bit-exact contract is tests/stereo_ref.py.  --subpixel renders with v3d_render_stereo_subpixel_batch instead:
positions in 1/16 pixel and colours interpolated along the spans between neighbouring sources, so that a smooth depth surface
no longer comes out as a staircase of duplicated and dropped pixels (contract: tests/stereo_sub_ref.py).  --layout packs the two
eyes for the display: side by side, top-bottom, row-interleaved or as a red-cyan anaglyph; every layout but the two side-by-side
ones is v3d_render_stereo_packed_batch, which packs in the launch that renders (contract: tests/stereo_pack_ref.py).  The parameters:

    max_shift    parallax in pixels between depth 65535 (nearest) and depth 0 (default 48 = 1.25 % of a 3840 frame)
    convergence  the depth at the screen plane, in [0, 1] (default 0.5): nearer moves right in the left eye, left in the right
    eye_split    the left eye's share of the shift, in [0, 1] (default 0.5; 0 keeps the 4K frame itself as the left eye)

--parallax source replaces the three invented parameters by the film's own parallax: a depth run made with --depth-range metric
stores the matcher's disparity itself (64 s / 65535 pixels of its eye), and source_parallax() maps it back to 4K pixels, so the right
eye's target of a pixel is x - round(K s d): the left eye is the 4K frame, the right eye sits where the SBS release had it.
--fill-from-source SBS_CLIP then takes the disocclusions of that right eye from the SBS clip's stored right eye
(v3d_render_stereo_source_batch; contract: tests/stereo_source_ref.py) instead of stretching the background into them.
--match-colour clip|frame first fits that eye's colours to the 4K frame's (colour.py: the SBS clip is another release, another grading);
--verify-source [TAU] then checks the rendered right eye against that stored eye, cell by cell, and replaces the cells whose mean
colour is off by more than TAU with the stored eye's own samples (verify.py; only where the right eye lies unpacked in the output:
full-sbs and full-tb); --fidelity-report [PATH] measures what came of it against the SBS frame's stored eyes (fidelity.py), and changes
no output byte and no cache key.  --fuse-source, between the two, takes the right eye's low band from the stored eye and keeps only
the render's detail above the stored eye's resolution (verify.SourceFuser).  These four are the plan's steps (verify.SourceStep):
the conversion only iterates them.

Data flow: depth PNGs are decoded ahead on reader threads, 4K frames stream from the decoder, CONVERT_BATCH frames at a time
cross PCIe in one pinned copy, render in one launch and come back in one copy; 8-bit RGB PNGs are compressed on the writer
pool.  The output directory `<output without suffix>_frames` is itself a clip (frame_%06d.png + info.json).
"""
import argparse
import functools
import json
from pathlib import Path

import numpy as np

from . import sharding
from .backend import HipBackend, require_hip_device
from .colour import DEFAULT_PROBES, ColourMatcher
from .fidelity import FidelityMonitor, check_fidelity_report
from .utils import (PngWriterPool, encode_png8, finish_sequence, get_video_info, iter_frames, prefetch_map, read_png16,
                    sibling_frames_dir)      # sibling_frames_dir is importable from here too
from .verify import DEFAULT_VERIFY_TAU, VERIFY_LAYOUTS, VERIFY_TAU_MAX, SourceFuser, SourceVerifier, check_fuse_source, check_source_rules, check_verify_source  # noqa: F401

# V3D_PACK_*: codes 0 / 1 are V3D_STEREO_FULL_SBS / V3D_STEREO_HALF_SBS of v3d_render_stereo[_subpixel]_batch, codes >= 2 go to
# v3d_render_stereo_packed_batch
LAYOUTS = {"full-sbs": 0, "half-sbs": 1, "full-tb": 2, "half-tb": 3, "interlaced": 4, "anaglyph-colour": 5, "anaglyph-dubois": 6}
DEFAULT_MAX_SHIFT, DEFAULT_CONVERGENCE, DEFAULT_EYE_SPLIT = 48.0, 0.5, 0.5
PARALLAX = ("invented", "source")
FILL_RIGHT_EYE = 2                  # --fill-from-source: fill_eyes of v3d_render_stereo_source_batch (the left eye has gain 0, no holes)
# frames per launch: 4 x (25 MB BGR + 17 MB depth) of pinned input staging and 4 x 50 MB of pinned output (full SBS at 4K)
CONVERT_BATCH = 4

png_rgb_from_bgr = functools.partial(encode_png8, bgr=True)     # the writer pool's encoder of the stereo frames


def add_stereo_arguments(parser):
    """--layout / --max-shift / --convergence / --eye-split / --subpixel: shared by the convert CLI and the pipeline's
    --stereo-output"""
    parser.add_argument('--layout', choices=list(LAYOUTS), default='full-sbs',
                        help='full-sbs: two full-width eyes side by side (2W x H); half-sbs: each eye squeezed to W/2 (W x H); '
                             'full-tb: the left eye above the right (W x 2H); half-tb: each eye squeezed to H/2, left on top '
                             '(W x H, most 3D TVs and VR players); interlaced: left eye in even rows, right eye in odd rows '
                             '(W x H, passive line-polarised displays); anaglyph-colour: red from the left eye, green and blue '
                             'from the right (W x H, red-cyan glasses); anaglyph-dubois: red-cyan by the Dubois least-squares '
                             'matrices (W x H, less ghosting and retinal rivalry)')
    parser.add_argument('--max-shift', type=float, default=None,
                        help=f'parallax in pixels between the nearest and the farthest depth (default {DEFAULT_MAX_SHIFT:g})')
    parser.add_argument('--convergence', type=float, default=None,
                        help=f'depth at the screen plane, 0 (far) .. 1 (near) (default {DEFAULT_CONVERGENCE:g})')
    parser.add_argument('--eye-split', type=float, default=None,
                        help=f"left eye's share of the shift, 0 .. 1; 0 keeps the 4K frame as the left eye (default {DEFAULT_EYE_SPLIT:g})")
    parser.add_argument('--subpixel', action='store_true',
                        help='sub-pixel DIBR: positions in 1/16 px, colours interpolated between neighbouring sources '
                             '(smooth surfaces render without one-pixel tears; default: whole-pixel shifts)')
    parser.add_argument('--parallax', choices=PARALLAX, default='invented',
                        help="invented: --max-shift / --convergence / --eye-split map the depth to a parallax (default).  source: the "
                             "film's own parallax, from a depth run made with --depth-range metric: the left eye is the 4K frame, the "
                             "right eye sits where the SBS release had it; not with --max-shift, --convergence or --eye-split.  The depth "
                             "must be the 16-bit PNG sequence with its JSON manifest: an H.264 depth file carries neither the metric "
                             "samples nor the depth_range block")
    parser.add_argument('--parallax-gain', type=float, default=None, metavar='K',
                        help='with --parallax source: scale the film\'s parallax by K (default 1.0)')


def stereo_options(args):
    """the parsed stereo flags as keyword arguments; `subpixel` and the parallax keys appear only when their flag is on"""
    explicit = [f"--{k.replace('_', '-')}" for k in ("max_shift", "convergence", "eye_split") if getattr(args, k) is not None]
    source = getattr(args, "parallax", "invented") == "source"
    if source and explicit:
        raise ValueError(f"--parallax source takes the film's parallax: it cannot be combined with {', '.join(explicit)}")
    if not source and getattr(args, "parallax_gain", None) is not None:
        raise ValueError("--parallax-gain needs --parallax source")
    opts = dict(max_shift=DEFAULT_MAX_SHIFT if args.max_shift is None else args.max_shift,
                convergence=DEFAULT_CONVERGENCE if args.convergence is None else args.convergence,
                eye_split=DEFAULT_EYE_SPLIT if args.eye_split is None else args.eye_split, layout=args.layout)
    if getattr(args, "subpixel", False):
        opts["subpixel"] = True
    if source:
        opts.update(parallax="source", parallax_gain=1.0 if args.parallax_gain is None else args.parallax_gain)
    return opts


def source_parallax(depth_range, Whi: int, spatial_map=None, gain: float = 1.0, flag: str = "--depth-range metric"):
    """--parallax source: the `depth_range` block of a metric depth run + the 4K width -> dict(max_shift, convergence, eye_split,
    scale, gain), the parameters stereo_settings turns into gains.  A u16 sample v is a rebiased disparity of 64 v / 65535 pixels
    of the matcher's eye (W_eye wide); s = Whi / (Ax W_eye) 4K pixels per matcher pixel (Ax: the applied spatial map's x scale, or
    1); with eye_split 0, max_shift = K s 64 65536 / 65535 and convergence = -m / 64 (m: the search window's first disparity) the
    right eye's target is x - round(K s d), d the matcher's own disparity: the film's parallax at 4K."""
    import math
    if not isinstance(depth_range, dict) or depth_range.get("mode") != "metric":
        raise ValueError(f"--parallax source needs a depth run made with {flag}, given as its JSON manifest of 16-bit PNGs (a manifest "
                         f"with a depth_range block whose mode is metric; an .mp4 depth file carries none)")
    W_eye, m, hi = depth_range.get("eye_width"), depth_range.get("min_disparity", 0), depth_range.get("hi", 64)
    if not isinstance(W_eye, int) or W_eye < 1 or not isinstance(m, int) or not -hi <= m <= 0:
        raise ValueError(f"--parallax source: the depth_range block {depth_range} lacks a usable eye_width / min_disparity")
    if isinstance(gain, bool) or not isinstance(gain, (int, float, np.integer, np.floating)) or not math.isfinite(gain) or gain < 0:
        raise ValueError(f"--parallax-gain must be a finite number >= 0, got {gain!r}")
    Ax = float(spatial_map[0]) if spatial_map is not None else 1.0
    if not Ax > 0:
        raise ValueError(f"--parallax source: spatial map {spatial_map} has no positive x scale")
    s = Whi / (Ax * W_eye)
    max_shift = gain * s * hi * 65536 / 65535
    if math.floor(max_shift * 256 + 0.5) >= 1 << 24:           # |gain_right| < 2^24 is what the render entries take
        raise ValueError(f"--parallax source: scale {s:g} x gain {gain:g} gives a render gain beyond 2^24")
    return dict(max_shift=max_shift, convergence=-m / hi, eye_split=0.0, scale=s, gain=float(gain))


def fill_map_q16(spatial_map, eye_size, frame_size):
    """--fill-from-source: the Q16 map (ax, bx, ay, by) from a 4K target to the stored eye's sample grid, for the applied spatial
    map (normalised plane coordinates, so the stored half-width eye needs no special case) or the identity"""
    from .register import map_to_q16
    Ax, Bx, Ay, By = spatial_map if spatial_map is not None else (1, 0, 1, 0)
    (We, Hs), (Whi, Hhi) = eye_size, frame_size
    q = map_to_q16(Ax, Bx, We, Whi) + map_to_q16(Ay, By, Hs, Hhi)
    if not (1 << 12 <= q[0] <= 1 << 20 and 1 << 12 <= q[2] <= 1 << 20 and abs(q[1]) <= 1 << 40 and abs(q[3]) <= 1 << 40):
        raise ValueError(f"--fill-from-source: a {We}x{Hs} eye under a {Whi}x{Hhi} frame leaves the sampler's range (1/16 .. 16 samples per pixel)")
    return q


def right_eye_view(out, layout, W, H):
    """the right eye [n,H,W,3] of packed full-sbs / full-tb frames [n,outH,outW,3] as a view (NumPy array or tensor alike)"""
    return out[:, :, W:] if layout == LAYOUTS["full-sbs"] else out[:, H:]


def left_eye_view(out, layout, W, H):
    """the left eye of the same frames"""
    return out[:, :, :W] if layout == LAYOUTS["full-sbs"] else out[:, :H]


def depth_manifest(depth_path):
    """the JSON manifest of a 4K depth run at depth_path, or {} (a directory, a video, anything else)"""
    p = Path(depth_path)
    if not p.is_file():
        return {}
    with open(p, "rb") as f:
        if f.read(1) != b"{":
            return {}
    try:
        man = json.loads(p.read_text())
    except (UnicodeDecodeError, ValueError):
        return {}
    return man if isinstance(man, dict) else {}


def stereo_settings(max_shift=DEFAULT_MAX_SHIFT, convergence=DEFAULT_CONVERGENCE, eye_split=DEFAULT_EYE_SPLIT, layout="full-sbs",
                    subpixel=False):
    """validated user parameters -> (layout code, (gain_left, gain_right, conv)); ValueError for anything out of range"""
    from ._native import stereo_gains
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {sorted(LAYOUTS)}, got {layout!r}")
    if not isinstance(subpixel, (bool, np.bool_)):
        raise ValueError(f"subpixel must be True or False, got {subpixel!r}")
    return LAYOUTS[layout], stereo_gains(max_shift, convergence, eye_split)


def output_size(layout, W, H):
    """(outW, outH) of the packed frame of layout code `layout` (_native.stereo_output_size): ValueError for half-sbs on an odd
    width and half-tb on an odd height"""
    from ._native import stereo_output_size
    return stereo_output_size(layout, W, H)


def render_stereo(native, frames, depths, gain_left, gain_right, conv, layout, out, subpixel=False):
    """the native call of a layout code: the two side-by-side layouts go where they always went, the others to the packed entry"""
    if layout >= 2:
        return native.render_stereo_packed_batch(frames, depths, gain_left, gain_right, conv, layout, out, subpixel=subpixel)
    return native.render_stereo_batch(frames, depths, gain_left, gain_right, conv, layout, out, subpixel=subpixel)


def finish_stereo_output(frames_dir: Path, output_path, count: int, width: int, height: int, fps: float, params: dict, gains, entries=()):
    """one process, after every frame is written: the manifest of the PNG sequence (entries: what the plan's steps add to it), through
    finish_sequence (as encode_depth4k)"""
    man = {
        "format": "png8-rgb-sequence", "frames_dir": str(frames_dir), "pattern": "frame_%06d.png",
        "count": count, "width": width, "height": height, "fps": fps, "layout": params["layout"],
        "max_shift": params["max_shift"], "convergence": params["convergence"], "eye_split": params["eye_split"],
        "gain_left": gains[0], "gain_right": gains[1], "conv": gains[2],
        "note": "no ffmpeg binary on this host: side-by-side frames kept as 8-bit RGB PNGs"}
    if params.get("subpixel"):
        man["subpixel"] = True
    if params.get("parallax") == "source":
        man.update(parallax="source", parallax_scale=params["parallax_scale"], parallax_gain=params["parallax_gain"])
    if params.get("fill_from_source"):
        man.update(fill_from_source=params["fill_from_source"], source_start_frame=params.get("source_start_frame", 0))
    man.update(entries)
    finish_sequence(frames_dir, "frame_%06d.png", output_path, fps, man)


def depth_frame_files(depth_path):
    """the 4K depth maps of a depth run: a directory of depth4k_%06d.png, the JSON manifest the upscale CLI / the pipeline
    write at their output path (whatever its suffix), or a file whose sibling `<path without suffix>_frames` directory holds
    them (the upscale CLI keeps it next to its .mp4)"""
    p = Path(depth_path)

    def listing(d):
        return sorted(Path(d).glob("depth4k_*.png"))

    files = []
    if p.is_dir():
        files = listing(p)
    elif p.is_file():
        man = depth_manifest(p)
        if "frames_dir" in man:
            d = Path(man["frames_dir"])
            if not d.is_dir() and not d.is_absolute():
                d = p.parent / d
            files = listing(d)[:int(man.get("count", 1 << 62))]
        if not files:
            files = listing(sibling_frames_dir(p))
    if not files:
        raise ValueError(f"No depth maps found in {depth_path}")
    return files


class HipRenderBackend(HipBackend):
    """the device side of the convert step: pinned staging, one H2D, one v3d_render_stereo_batch launch, one D2H per batch"""

    def render_batch(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, png=False, subpixel=False, source=None):
        """NumPy BGR frames [H,W,3] + u16 depth maps [H,W] -> NumPy u8 [n,H,outW,3].  The input staging holds `capacity`
        frames and is reused (the synchronise at the end of the previous call made that safe); the output block comes from
        torch's caching host allocator and returns to it once the writers drop the last frame of it.
        source (--fill-from-source): dict(frames: the SBS BGR frames [Hs,Ws,3] of this batch, fill_eyes, q: (ax, bx, ay, by)) -- the
        render is v3d_render_stereo_source_batch, one launch all the same.  With a `match` entry (--match-colour: ColourMatcher.
        request) the right-eye half of the uploaded SBS frames is colour-matched in place before that launch: with the clip's
        table, or with one table per frame fitted to this batch (two histograms, the tables, the apply); nothing synchronises.
        With a `verify` entry (--verify-source: dict(tau)) the right eye of the staged output is checked in place against the
        (colour-matched) stored right eye right after the render, v3d_verify_eye_source_batch with the render's own map; its
        counters start their way to pinned memory before the frames' copy and are read after it (verify_counts).
        With a `fuse` entry (--fuse-source) that right eye, verified or not, is then fused in place with the same stored eye under
        the same map, v3d_fuse_eye_source_batch on a workspace of this backend's staging.
        With a `fidelity` entry (--fidelity-report: dict(bad_thr, ceiling)) the frames are rendered once more with fill_eyes 0 into
        a scratch output of this backend, and v3d_eye_fidelity_batch measures that right eye, the right eye of the staged output
        and, with `ceiling`, its left eye against the stored eyes; the staged output is only read.  With `ceiling` and a `match`
        entry the colour table goes over the whole SBS frame, after the histograms: the render and the verification read the
        right half alone.  The records travel as the counters do (fidelity_handle)"""
        torch, nat = self.torch, self.native
        n = len(frames)
        H, W = depths[0].shape
        cap = max(n, capacity or n)
        oW, oH = nat.stereo_output_size(layout, W, H)
        od = self._staging("out_dev", (cap, oH, oW, 3), torch.uint8, False)
        with torch.cuda.device(self.device):
            fd = self._upload("frames", frames, (H, W, 3), torch.uint8, cap)
            dd = self._upload("depth", [np.asarray(d, np.uint16).view(np.int16) for d in depths[:n]], (H, W), torch.int16, cap)
            if source is not None:
                sd = self._upload("sbs", source["frames"], tuple(source["frames"][0].shape), torch.uint8, cap)
                fid = source.get("fidelity")
                if source.get("match") is not None:
                    self._match_colour(sd, fd, source["match"], whole=fid is not None and fid["ceiling"])
                nat.render_stereo_source_batch(fd, dd, gain_left, gain_right, conv, layout, sd, source["fill_eyes"], *source["q"],
                                               out=od[:n], subpixel=subpixel)
                if source.get("verify") is not None:
                    counts = self._staging("verify_dev", (cap,), torch.int32, False)
                    nat.verify_eye_source_batch(right_eye_view(od[:n], layout, W, H), sd, 1, *source["q"], source["verify"]["tau"],
                                                out=counts[:n])
                    self._verify = self._fetch_async([counts[:n]])
                if source.get("fuse") is not None:
                    ws = self._staging("fuse_ws_dev", (nat.fuse_eye_source_ws_bytes(cap, *sd.shape[2:0:-1]),), torch.uint8, False)
                    nat.fuse_eye_source_batch(right_eye_view(od[:n], layout, W, H), sd, 1, *source["q"], ws=ws)
                if fid is not None:
                    self._fidelity = self._measure_fidelity(fd, dd, sd, od[:n], (gain_left, gain_right, conv), layout, subpixel,
                                                            source["q"], fid, cap)
            else:
                render_stereo(nat, fd, dd, gain_left, gain_right, conv, layout, od[:n], subpixel)
            return od[:n] if png else self._fetch(od[:n])

    def verify_counts(self):
        """--verify-source: the replaced cells per frame of the last render_batch (uint32 [n]) once its frames are on the host, or
        None when that call verified nothing.  The copy was enqueued before the frames' own, whose wait covered it"""
        handle, self._verify = getattr(self, "_verify", None), None
        return None if handle is None else self._read(handle)[0].view(np.uint32)

    def _measure_fidelity(self, fd, dd, sd, od, gains, layout, subpixel, q, fid, cap):
        """--fidelity-report: the warp series from a render with fill_eyes 0 into the scratch output, the final series from the
        right eye of od, the ceiling series from its left eye -> the handle of their records ([n,6] each) on the way to the host"""
        torch, nat = self.torch, self.native
        n, H, W = dd.shape
        scratch = self._staging("fidelity_out_dev", (cap,) + tuple(od.shape[1:]), torch.uint8, False)
        rec = self._staging("fidelity_dev", (3, cap, nat.FIDELITY_FIELDS), torch.int64, False)
        nat.render_stereo_source_batch(fd, dd, *gains, layout, sd, 0, *q, out=scratch[:n], subpixel=subpixel)
        nat.eye_fidelity_batch(right_eye_view(scratch[:n], layout, W, H), sd, 1, *q, fid["bad_thr"], out=rec[0, :n])
        nat.eye_fidelity_batch(right_eye_view(od, layout, W, H), sd, 1, *q, fid["bad_thr"], out=rec[1, :n])
        if fid["ceiling"]:
            nat.eye_fidelity_batch(left_eye_view(od, layout, W, H), sd, 0, *q, fid["bad_thr"], out=rec[2, :n])
        return self._fetch_async([rec[k, :n] for k in range(3 if fid["ceiling"] else 2)])

    def fidelity_handle(self):
        """--fidelity-report: the records of the last render_batch as a handle for read_fidelity, or None when that call measured
        nothing.  Their copies were enqueued before the frames' own"""
        handle, self._fidelity = getattr(self, "_fidelity", None), None
        return handle

    def read_fidelity(self, handle, wait: bool = True):
        """-> [warp, final(, ceiling)] int64 [n,6] each, or None while the copies run and wait is False"""
        return self._read(handle, wait)

    def _match_colour(self, sd, fd, match, whole=False):
        """the right eye of the staged SBS frames sd [n,Hs,Ws,3] through the clip's table, or through the tables of these frames'
        own left eyes against the staged 4K frames fd.  whole: the table goes over both eyes (after the histograms were taken)"""
        torch, nat = self.torch, self.native
        _, Hs, Ws, _ = sd.shape
        table = match["table"]
        if match["mode"] == "frame":
            table = nat.colour_lut_batch(nat.bgr_hist_batch(sd, match["eye_rect"]), nat.bgr_hist_batch(fd, match["frame_rect"]), 1)
        elif not isinstance(table, torch.Tensor):              # the NumPy surface hands the table over as an array
            table = torch.from_numpy(np.ascontiguousarray(table, np.uint8).reshape(3, 256)).to(self.device)
        nat.bgr_lut_batch(sd, table, (0 if whole else Ws // 2, 0, Ws, Hs), out=sd)

    def colour_probe(self, sbs_frames, frames, eye_rect, frame_rect):
        """--match-colour clip, before the render loop: probe pairs -> (left-eye histograms, 4K histograms), int32 [n,3,256] each on
        the device.  Uses the render loop's staging, so it waits for its launches before it returns"""
        torch, nat = self.torch, self.native
        with torch.cuda.device(self.device):
            cap = max(len(frames), CONVERT_BATCH)              # the staging the render loop is about to use
            sd = self._upload("sbs", sbs_frames, tuple(sbs_frames[0].shape), torch.uint8, cap)
            fd = self._upload("frames", frames, tuple(frames[0].shape), torch.uint8, cap)
            pair = nat.bgr_hist_batch(sd, eye_rect), nat.bgr_hist_batch(fd, frame_rect)
            self._synchronize()
        return pair

    def colour_table(self, hists):
        """the probe passes' histograms -> (the one table of all of them, u8 [1,3,256] on the device, its NumPy copy [3,256])"""
        torch, nat = self.torch, self.native
        with torch.cuda.device(self.device):
            hs, hd = (torch.cat([h[k] for h in hists]) for k in (0, 1))
            table = nat.colour_lut_batch(hs, hd, hs.shape[0])
            return table, np.array(self._fetch(table)[0])

    def render_batch_png(self, frames, depths, gain_left, gain_right, conv, layout, capacity=None, subpixel=False, source=None):
        """--png-encoder gpu: render_batch whose frames stay on the device and come back as the zlib streams of their PNGs"""
        return self._png_encoder().encode(self.render_batch(frames, depths, gain_left, gain_right, conv, layout, capacity, png=True,
                                                            subpixel=subpixel, **({} if source is None else {"source": source})))


class StereoPlan:
    """What stereo_options(args) (+ the fill-from-source keys) mean for a run, for the convert CLI and the pipeline's --stereo-output
    alike: validated once, then the render calls' layout code, gains and optional keywords, the packed frame's size, the writers'
    encoder and the files that finish the clip.
    subpixel: sub-pixel DIBR (the backend's render calls then carry subpixel=True; with it off they are unchanged);
    parallax: "source" takes the parallax from the depth run's depth_range block (resolve_source) and ignores max_shift /
    convergence / eye_split, parallax_gain scales it;
    fill_from_source: the SBS clip whose stored right eye fills the right eye's disocclusions (needs parallax="source": the holes
    of an invented parallax do not line up with the real eye); source_start_frame: its frame that depth frame 0 was made from;
    match_colour and match_probes, verify_source (the threshold), fuse_source, fidelity_report (True: next to the manifest, or its path): the
    source-eye options, which make self.steps (verify.SourceStep) in the order of their entries in the render calls' source dict"""

    def __init__(self, max_shift: float = DEFAULT_MAX_SHIFT, convergence: float = DEFAULT_CONVERGENCE,
                 eye_split: float = DEFAULT_EYE_SPLIT, layout: str = "full-sbs", subpixel: bool = False, parallax: str = "invented",
                 parallax_gain: float = 1.0, fill_from_source: str = None, source_start_frame: int = 0, match_colour: str = None,
                 match_probes: int = None, verify_source: int = None, fidelity_report=None, fuse_source: bool = False):
        if parallax not in PARALLAX:
            raise ValueError(f"parallax must be one of {PARALLAX}, got {parallax!r}")
        check_source_rules(fill_from_source, parallax=parallax)
        if isinstance(source_start_frame, bool) or not isinstance(source_start_frame, (int, np.integer)) or source_start_frame < 0:
            raise ValueError(f"--source-start-frame must be an integer >= 0, got {source_start_frame!r}")
        check_source_rules(fill_from_source, match_colour=match_colour, match_probes=match_probes)
        self.steps = []
        if match_colour is not None:
            self.steps.append(ColourMatcher(match_colour, DEFAULT_PROBES if match_probes is None else match_probes))   # checks both values
            match_probes = self.steps[-1].probes
        self.match_colour, self.match_probes = match_colour, match_probes
        self.verify_source = None if verify_source is None else check_verify_source(verify_source, layout, parallax == "source", False)
        if self.verify_source is not None:
            self.steps.append(SourceVerifier(self.verify_source))
        self.fuse_source = bool(fuse_source)
        if self.fuse_source:
            check_fuse_source(layout, parallax == "source", False)
            self.steps.append(SourceFuser())
        self.fidelity_report = None if fidelity_report is None or fidelity_report is False else fidelity_report
        if self.fidelity_report is not None:
            check_fidelity_report(layout, parallax == "source", False)
            self.steps.append(FidelityMonitor(path=self.fidelity_report))
        self.parallax, self.parallax_gain = parallax, parallax_gain
        self.fill_from_source, self.source_start_frame = fill_from_source, int(source_start_frame)
        self.layout_code, self.gains = stereo_settings(max_shift, convergence, eye_split, layout, subpixel)
        self.subpixel = bool(subpixel)
        self.params = dict(max_shift=max_shift, convergence=convergence, eye_split=eye_split, layout=layout)   # the manifest's entries
        if self.subpixel:
            self.params["subpixel"] = True
        self.spatial_map = None                      # the spatial map the depth run applied (resolve_source)
        self.size = None                             # (outW, outH) of the packed frame (check_frame)
        if parallax == "source":
            source_parallax({"mode": "metric", "eye_width": 1, "min_disparity": 0}, 1, None, parallax_gain)     # the gain's own checks, now
            self.gains = None                        # until resolve_source, and so are the three parameters it derives
            self.params.update(max_shift=None, convergence=None, eye_split=None)

    def check_frame(self, W: int, H: int):
        """the 4K frame's size -> self.size = (outW, outH); ValueError for a half layout on an odd size"""
        if self.layout_code == LAYOUTS["half-sbs"] and W % 2:
            raise ValueError(f"half SBS needs an even frame width, the 4K clip is {W} wide")
        if self.layout_code == LAYOUTS["half-tb"] and H % 2:
            raise ValueError(f"half top-bottom needs an even frame height, the 4K clip is {H} high")
        self.size = output_size(self.layout_code, W, H)

    def resolve_source(self, depth_range, Whi: int, spatial_map=None, announce: bool = True):
        """parallax="source": the depth run's depth_range block, the 4K width and the applied spatial map (or None) -> the gains"""
        p = source_parallax(depth_range, Whi, spatial_map, self.parallax_gain)
        _, self.gains = stereo_settings(p["max_shift"], p["convergence"], p["eye_split"], self.params["layout"], self.subpixel)
        self.params.update(max_shift=p["max_shift"], convergence=p["convergence"], eye_split=p["eye_split"], parallax="source",
                           parallax_scale=p["scale"], parallax_gain=p["gain"])
        self.spatial_map = None if spatial_map is None else tuple(float(v) for v in spatial_map)
        if announce:
            print(f"Source parallax: {p['scale']:g} 4K px per matcher px x gain {p['gain']:g} -> gains {self.gains}")
        return self.gains

    def render_kwargs(self):
        """what a backend's render call gains: nothing with --subpixel off, so a backend that predates it is called as before"""
        return {"subpixel": True} if self.subpixel else {}

    def source_kwargs(self, sbs_frames, frame_size, surface: bool = False):
        """what a backend's render call gains with --fill-from-source: nothing without it (surface: on the NumPy surface, which prepares no step)"""
        if sbs_frames is None:
            return {}
        Hs, Ws = sbs_frames[0].shape[:2]
        if Ws % 2:
            raise ValueError(f"the SBS frames of --fill-from-source are {Ws} wide: not two eyes side by side")
        source = dict(frames=sbs_frames, fill_eyes=FILL_RIGHT_EYE, q=fill_map_q16(self.spatial_map, (Ws // 2, Hs), frame_size))
        for step in self.steps:
            if step.on_surface or not surface:
                step.check_map(source["q"])
                source[step.key] = step.request()
        return {"source": source}

    def note(self, backend, src, indices, frame_size):
        """after a render call that carried source_kwargs' src: every step whose request was in it takes note"""
        for step in self.steps:
            if step.key in src.get("source", ()):
                step.note(backend, indices, frame_size, src["source"]["q"])

    def encoder(self, gpu_png: bool):
        """the writer pool's encoder of a rendered frame: the wrapper of a device-deflated stream, or zlib on the writer threads"""
        from .png_gpu import rgb8_file
        return rgb8_file(*self.size) if gpu_png else png_rgb_from_bgr

    def finish(self, frames_dir: Path, output_path, count: int, fps: float, entries=()):
        """one process, after every frame is written: info.json makes frames_dir a clip, then the H.264 file or the manifest"""
        (frames_dir / "info.json").write_text(json.dumps({"fps": fps}))
        finish_stereo_output(frames_dir, output_path, count, *self.size, fps, self.params, self.gains, entries)


def _of_plan(name):
    return property(lambda self: getattr(self.plan, name))


class DepthTo3DConverter:
    """4K frames + 4K depth maps -> side-by-side 3D frames (DIBR on the GPU)"""

    writer_pool_factory = PngWriterPool       # sink of the 8-bit RGB frames (the CLIs' hook)

    def __init__(self, device: str = "cuda", backend=None, batch_size: int = CONVERT_BATCH, png_encoder: str = "zlib", **stereo):
        """backend: HipRenderBackend (built when None) or a stand-in with its render_batch (host-logic tests);
        png_encoder: "gpu" deflates the rendered frames on the device (png_gpu.py); "zlib" = on the writer threads;
        every other keyword is StereoPlan's (parallax="source": set_source_parallax, or process_conversion from the depth manifest)"""
        from .png_gpu import check_png_encoder
        self.png_encoder = check_png_encoder(png_encoder)
        self.plan = StereoPlan(**stereo)
        if backend is None:
            require_hip_device(device)
            backend = HipRenderBackend(device)
        self.backend = backend
        self.batch_size = max(1, int(batch_size))

    # the plan's state and steps under the converter's own names
    params, gains, layout_code = _of_plan("params"), _of_plan("gains"), _of_plan("layout_code")
    subpixel, parallax, parallax_gain = _of_plan("subpixel"), _of_plan("parallax"), _of_plan("parallax_gain")
    spatial_map, fill_from_source, source_start_frame = _of_plan("spatial_map"), _of_plan("fill_from_source"), _of_plan("source_start_frame")

    def set_source_parallax(self, depth_range, Whi: int, spatial_map=None):
        """the plan's resolve_source, silently"""
        return self.plan.resolve_source(depth_range, Whi, spatial_map, announce=False)

    def render_frame(self, frame_bgr: np.ndarray, depth_u16: np.ndarray, source: np.ndarray = None, colour_table: np.ndarray = None) -> np.ndarray:
        """NumPy surface: HxWx3 uint8 BGR + HxW uint16 depth -> the side-by-side BGR image (synchronous).  source: the SBS BGR
        frame the depth was made from; the right eye's disocclusions are sampled from its stored right eye (parallax="source" only);
        colour_table: u8 [3,256] (BGR), applied to that eye first, as --match-colour clip applies its table.  With verify_source
        set and a source given, the right eye is verified against that stored eye as --verify-source does, and with fuse_source set it
        is then fused with it as --fuse-source does"""
        frame_bgr, depth_u16 = np.asarray(frame_bgr), np.asarray(depth_u16)
        if frame_bgr.shape[:2] != depth_u16.shape or frame_bgr.ndim != 3 or frame_bgr.shape[2] != 3:
            raise ValueError(f"frame {frame_bgr.shape} and depth {depth_u16.shape} disagree")
        if self.gains is None:
            raise ValueError("parallax='source': call set_source_parallax(depth_range, frame width) first")
        if source is not None and self.parallax != "source":
            raise ValueError("source= needs parallax='source'")
        if colour_table is not None and source is None:
            raise ValueError("colour_table= needs source=: it is applied to the SBS frame's right eye")
        src = self.plan.source_kwargs(None if source is None else [np.asarray(source, np.uint8)], frame_bgr.shape[1::-1], surface=True)
        if colour_table is not None:
            table = np.asarray(colour_table)
            if table.dtype != np.uint8 or table.shape != (3, 256):
                raise ValueError(f"colour_table must be uint8 [3,256], got {table.dtype} {table.shape}")
            src["source"]["match"] = dict(mode="clip", table=table, eye_rect=None, frame_rect=None)
        out = np.array(self.backend.render_batch([frame_bgr], [depth_u16], *self.gains, self.layout_code,
                                                 **self.plan.render_kwargs(), **src)[0])
        self.plan.note(self.backend, src, [0], frame_bgr.shape[1::-1])
        return out

    def process_conversion(self, video_4k_path: str, depth_path: str, output_path: str = None, force_reprocess: bool = False,
                           guide_start_frame: int = 0, max_frames: int = None) -> str:
        """depth frame i pairs with 4K frame guide_start_frame + i (the offset the upscale CLI used).  Returns the output
        path: an H.264 file when ffmpeg exists and it ends in .mp4, else a JSON manifest of the PNG sequence."""
        plan = self.plan
        print(f"4K + depth -> 3D ({self.params['layout']}{', sub-pixel' if self.subpixel else ''}"
              f"{', source parallax' if self.parallax == 'source' else ''}): {video_4k_path} + {depth_path}")
        depth_files = depth_frame_files(depth_path)
        info = get_video_info(video_4k_path)
        if not info:
            raise ValueError(f"Could not read video info: {video_4k_path}")
        W, H = info['width'], info['height']
        if output_path is None:
            # _subpx: a run with --subpixel never reuses a file rendered without it
            tag = ("_subpx" if self.subpixel else "") + ("_srcpx" if self.parallax == "source" else "") + \
                  ("_srcfill" if self.fill_from_source else "") + "".join(step.output_tag for step in plan.steps)
            output_path = f"3d_{self.params['layout']}{tag}_{Path(depth_path).with_suffix('').name}.mp4"
        output_path = Path(output_path)
        if output_path.exists() and not force_reprocess:
            print(f"✓ Using existing 3D video: {output_path}")
            for note in filter(None, (step.cached_note for step in plan.steps)):
                print(note)
            return str(output_path)
        plan.check_frame(W, H)
        if self.parallax == "source":                           # the film's parallax: from the depth run's own record
            man = depth_manifest(depth_path)
            plan.resolve_source(man.get("depth_range"), W, man.get("spatial_map"))
            if self.fill_from_source is not None and man.get("input_layout", "sbs") != "sbs":
                raise ValueError(f"--fill-from-source cannot read a top-bottom source (the depth run's input_layout is "
                                 f"{man['input_layout']}): the fill samples the stored right eye at column We + i of a side-by-side "
                                 f"frame, and a top-bottom clip keeps that eye in rows, not columns.  --parallax source alone works "
                                 f"for both layouts")
        if self.fill_from_source is not None:
            if not get_video_info(self.fill_from_source):
                raise ValueError(f"Could not read video info: {self.fill_from_source}")
            self.params.update(fill_from_source=str(self.fill_from_source), source_start_frame=self.source_start_frame)
        n = len(depth_files) if max_frames is None else min(len(depth_files), max(int(max_frames), 0))
        g0, frames_dir = max(int(guide_start_frame), 0), sibling_frames_dir(output_path)
        for step in plan.steps:                                 # on every rank, before the ranks part: all prepare the same
            step.prepare(self.backend, plan, video_4k_path, g0, n, (W, H))
        self._render(video_4k_path, g0, n, depth_files, frames_dir, (W, H))
        self._finish(output_path, frames_dir, info['fps'])
        print(f"✓ 3D video saved: {output_path}")
        return str(output_path)

    def _render(self, video_4k_path, g0, n, depth_files, frames_dir, size):
        """the streaming loop: this rank's frames, batch_size at a time, through the backend and on to the writers"""
        plan = self.plan
        rank, world = sharding.rank_world()
        sharding.require_initialized(world)
        frames_dir.mkdir(parents=True, exist_ok=True)
        mine = list(range(rank, n, world))                       # frame i -> rank i mod world; both inputs decoded per rank
        depths = prefetch_map(read_png16, [depth_files[i] for i in mine])
        frames4k = iter_frames(video_4k_path, g0, n, stride=world, offset=rank)
        sbs_frames = iter_frames(self.fill_from_source, self.source_start_frame, n, stride=world, offset=rank) if self.fill_from_source else None
        batch_f, batch_d, batch_i, batch_s = [], [], [], []
        rendered = 0
        gpu_png = self.png_encoder == "gpu"
        encode = plan.encoder(gpu_png)

        def flush(writers):
            nonlocal rendered
            if not batch_f:
                return
            # --png-encoder gpu: deflated on the device, only the streams cross PCIe
            render = self.backend.render_batch_png if gpu_png else self.backend.render_batch
            src = plan.source_kwargs(batch_s if sbs_frames is not None else None, size)
            out = render(batch_f, batch_d, *plan.gains, plan.layout_code, capacity=self.batch_size, **plan.render_kwargs(), **src)
            plan.note(self.backend, src, batch_i, size)
            for j, i in enumerate(batch_i):
                writers.submit(frames_dir / f"frame_{i:06d}.png", out[j], encode=encode)
            rendered += len(batch_i)
            for b in (batch_f, batch_d, batch_i, batch_s):
                b.clear()

        try:
            with self.writer_pool_factory() as writers:
                for k, i in enumerate(mine):
                    f = next(frames4k, None)
                    if f is None:
                        print(f"Warning: 4K video ended after {k} of this rank's frames; rendering stops at depth frame {i}")
                        break
                    if sbs_frames is not None:
                        s = next(sbs_frames, None)
                        if s is None:
                            print(f"Warning: the SBS clip ended after {k} of this rank's frames; rendering stops at depth frame {i}")
                            break
                        batch_s.append(s)
                    d = next(depths)
                    if d.shape != f.shape[:2] or f.ndim != 3:
                        raise ValueError(f"depth map {depth_files[i].name} is {d.shape[1]}x{d.shape[0]}, "
                                         f"the 4K frame {f.shape[1]}x{f.shape[0]}")
                    batch_f.append(f)
                    batch_d.append(d)
                    batch_i.append(i)
                    if len(batch_f) == self.batch_size:
                        flush(writers)
                flush(writers)
        finally:
            depths.close()
        self.last_rendered_frames = rendered

    def _finish(self, output_path, frames_dir, fps):
        """every rank: the steps' summaries; rank 0: their side files and the clip's manifest"""
        rank, world = sharding.rank_world()
        total = sharding.total(self.last_rendered_frames)
        if total == 0:
            raise ValueError("No frames rendered")
        sharding.barrier()
        entries, files = {}, {}
        for step in self.plan.steps:
            more, named = step.finish(output_path, frames_dir, world)
            entries, files = {**entries, **more}, {**named, **files}     # the files in the order they were always written: the last step's first
        if rank == 0:
            for path, text in files.items():
                path.parent.mkdir(parents=True, exist_ok=True)
                path.write_text(text)
            self.plan.finish(frames_dir, output_path, total, fps, entries)
        sharding.barrier()


def main(argv=None, backend=None):
    """ Command line interface: 4K video + 4K depth -> side-by-side 3D (backend: a stand-in for host tests) """
    parser = argparse.ArgumentParser(description='4K video + its 4K depth maps -> side-by-side 3D (DIBR on the GPU)')
    parser.add_argument('video_4k', help='Path to the 4K 2D video')
    parser.add_argument('depth_4k', help='4K depth: a depth4k_%%06d.png directory, the manifest the upscale CLI or the pipeline '
                                         'wrote, or their output path next to its _frames directory')
    parser.add_argument('--output', help='Output path for the 3D video')
    add_stereo_arguments(parser)
    parser.add_argument('--max-frames', type=int, default=None, help='Maximum number of frames to render (default: all)')
    parser.add_argument('--force', action='store_true', help='Force reprocessing even if the output exists')
    parser.add_argument('--device', default='cuda', help='Processing device (default: cuda)')
    from .png_gpu import add_png_arguments, png_options
    add_png_arguments(parser)
    parser.add_argument('--fill-from-source', default=None, metavar='SBS_CLIP',
                        help="with --parallax source: take the right eye's disocclusions from the stored right eye of this SBS clip "
                             '(the clip the depth was computed from) instead of stretching the background into them')
    parser.add_argument('--source-start-frame', type=int, default=0, metavar='N',
                        help='the SBS frame that depth frame 0 was made from (default 0)')
    parser.add_argument('--match-colour', choices=['clip', 'frame'], default=None,
                        help="with --fill-from-source: fit the SBS clip's colours to the 4K frame's before its right eye fills the holes "
                             "(the two are different releases: grading, tone mapping and black level differ, and an unmatched fill "
                             "shows as a patch along every depth edge).  clip: one transfer curve per channel for the whole run, from "
                             "--match-probes frame pairs; cannot flicker.  frame: every frame is fitted on its own, for clips whose "
                             "difference changes from scene to scene; the filled regions can flicker.  Default: off")
    parser.add_argument('--match-probes', type=int, default=None, metavar='P',
                        help='with --match-colour clip: frame pairs, spread over the frames to render, that the table is fitted to '
                             '(1 .. 64, default 16)')
    parser.add_argument('--verify-source', type=int, nargs='?', const=DEFAULT_VERIFY_TAU, default=None, metavar='TAU',
                        help="with --fill-from-source and --layout full-sbs or full-tb: check the rendered right eye against the SBS "
                             "clip's stored right eye, cell by cell (the 4K pixels one stored sample spans), and take the stored eye's "
                             "samples where a cell's mean colour differs by more than TAU (sum over the three channels, 0 .. "
                             f"{VERIFY_TAU_MAX}; default {DEFAULT_VERIFY_TAU}): a wrong disparity warps wrong picture content into "
                             "place, and the film's own right eye shows it.  Default: off")
    parser.add_argument('--fidelity-report', nargs='?', const=True, default=None, metavar='PATH',
                        help="with --fill-from-source and --layout full-sbs or full-tb: measure the rendered eyes against the SBS clip's "
                             "stored eyes on the GPU -- error sums and SSIM of the right eye before the fill (depth + DIBR alone), of the "
                             "right eye as written, and of the left eye (how far the two releases differ) -- print a summary and write "
                             "<output>_fidelity.json next to the manifest (or to PATH).  No output changes")
    parser.add_argument('--fuse-source', action='store_true',
                        help="with --fill-from-source and --layout full-sbs or full-tb: take the right eye's low band (everything up to "
                             "the SBS clip's resolution) from the clip's stored right eye and keep only the detail above it from the "
                             "render: out = E - LP(E) + P, after --verify-source where both are given.  Filled holes and replaced cells "
                             "gain the 4K frame's detail, and slightly wrong warps lose their wrong low frequencies.  Use it with "
                             "--match-colour: the low band carries the SBS release's grading otherwise.  Default: off")
    from .align import add_guide_arguments, resolve_guide_start
    add_guide_arguments(parser, 'depth frame 0', 'the offset the upscale CLI used')
    args = parser.parse_args(argv)
    if not resolve_guide_start(args):
        return 1
    try:
        sharding.init_process_group()            # no-op for one process; under torchrun: one rank per GPU (sets the device)
        check_source_rules(args.fill_from_source, source_start_frame=args.source_start_frame)
        if args.verify_source is not None:
            check_verify_source(args.verify_source, args.layout, args.fill_from_source)
        check_source_rules(args.fill_from_source, layout=args.layout, fidelity_report=args.fidelity_report, fuse_source=args.fuse_source)
        conv = DepthTo3DConverter(device=args.device, backend=backend, **stereo_options(args), **png_options(args),
                                  **{k: getattr(args, k) for k in ("fill_from_source", "source_start_frame", "match_colour", "match_probes",
                                                                     "verify_source", "fidelity_report", "fuse_source")})
        output_path = conv.process_conversion(args.video_4k, args.depth_4k, output_path=args.output,
                                              force_reprocess=args.force, guide_start_frame=args.guide_start_frame,
                                              max_frames=args.max_frames)
        print(f"\n✓ Success! 3D video: {output_path}")
    except Exception as e:
        print(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    exit(main())
