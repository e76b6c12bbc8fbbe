"""One pass from the SBS clip to the 4K depth sequence: `python -m video_3d_pipeline.pipeline sbs.npy 4k.npy`.

The two-step route -- `python -m video_3d_pipeline.depth` writes normalised 16-bit 1080p PNGs, `python -m
video_3d_pipeline.upscale` reads them back and filters them against the 4K clip -- sends every depth map over PCIe twice
and through zlib twice before the 4K filter sees it.  Here the depth stays on the device from the SBS frame to the final
16-bit 4K sample, B frames at a time:

    SBS frames -> HipStereoBackend.sbs_to_disparity (the depth CLI's own pass, neural guidance included)
               -> v3d_depth_to_u16_batch (per-frame min-max -> u16, the depth PNG's samples)
                  [--temporal-radius R: the temporal stabiliser's u16 samples instead (temporal.py), R frames behind the matcher]
                  [--range-percentile P: the white point of either is the P-th percentile of the valid disparities, not the maximum]
                  [--fill-holes: the matcher's invalid pixels are filled inside sbs_to_disparity, before any of the above]
                  [--quality-report: reprojection error and flicker of the pass's planes are measured on the side (quality.py); no byte changes]
               -> [--keep-depth-maps: depth_%06d.png into the depth CLI's cache directory]
               -> v3d_guided_upscale_u16_batch against the matching 4K frames' luma -> u16 4K samples -> writer pool

Everything up to the u16 samples is the depth CLI's own driver (HybridStereoDepthExtractor.iter_depth_u16), so the depth maps
of the two are the same by construction.  The only lossy step between the two CLIs is the u16 quantisation of the normalised depth; it happens here on the device and
the filter reads the same u16 samples `read_png16(...).astype(float32)` gives the upscale CLI, so every output PNG is
byte-for-byte what the two CLIs write.  The two-step route stays the reference for this one.
"""
import argparse
from pathlib import Path

from .backend import require_hip_device
from .depth import HipStereoBackend, HybridStereoDepthExtractor, add_depth_arguments, check_frame_halves, depth_options, input_layout_options, sbs_eye_size
from .upscale import GUIDED_EPS, GUIDED_RADIUS, encode_depth4k
from .utils import PngWriterPool, get_video_info, iter_frames, sibling_frames_dir

# 4K frames per guided launch.  A frame costs ~25 MB of pinned BGR staging + 25 MB of device BGR + 17 MB of u16 output on
# each side, and the filter's workspace (used by its two-sweep routes) 133 MB of device memory: 8 frames keep the pinned
# host memory near 0.4 GB whatever the SGM pass size is.  A frame's bits do not depend on the batch it is filtered in.
GUIDE_BATCH = 8


class HipPipelineBackend(HipStereoBackend):
    """HipStereoBackend (which has the u16 samples and their copy to the host: the depth CLI needs them too) plus the device
    steps after them: guide luma, guided filter, stereo rendering."""

    def guide_luma(self, frames, height, width, capacity):
        """4K BGR frames (None = beyond the clip: flat 128) -> device luma [n,height,width].  The frames are gathered in one
        pinned buffer of `capacity` frames and cross PCIe in one copy; the buffer is reused by the next call, which
        to_host_u16's synchronise has made safe."""
        torch = self.torch
        n = len(frames)
        for f in frames:
            if f is not None and f.shape[:2] != (height, width):
                raise ValueError(f"4K frame of shape {f.shape}, expected {height}x{width}")
        bgr = [f if f is None or f.ndim == 3 else f[..., None] for f in frames]      # a luma frame: gray of (g, g, g) is g exactly
        dev = self._upload("guide", bgr, (height, width, 3), torch.uint8, capacity)
        luma = self._staging("guide_luma", (max(n, capacity), height, width), torch.uint8, False)
        self.native.bgr_to_gray(dev, luma[:n])
        for i, f in enumerate(frames):
            if f is None:
                luma[i].fill_(128)                              # beyond the 4K clip: flat guide, as upscale.py does
        return luma[:n]

    def guide_signatures(self, frames, height, width):
        """4K BGR frames -> their luma signatures [n,2304] on the device (the align CLI's video refinement): guide_luma's staging,
        GUIDE_BATCH frames at a time; the pinned buffer is free again once a chunk's copy has finished"""
        torch = self.torch
        out = torch.empty((len(frames), self.native.SIG_CELLS), dtype=torch.int16, device=self.device)
        for j0 in range(0, len(frames), GUIDE_BATCH):
            chunk = frames[j0:j0 + GUIDE_BATCH]
            self.native.frame_signature_batch(self.guide_luma(chunk, height, width, GUIDE_BATCH), out[j0:j0 + len(chunk)])
            self._synchronize()
        return out

    def guide_profiles(self, frames, height, width):
        """4K BGR frames -> the column and row sums of their luma on the device (register.estimate): guide_luma's staging,
        GUIDE_BATCH frames at a time, as guide_signatures"""
        torch = self.torch
        cols, rows = [], []
        for j0 in range(0, len(frames), GUIDE_BATCH):
            chunk = frames[j0:j0 + GUIDE_BATCH]
            c, r = self.native.plane_profiles_batch(self.guide_luma(chunk, height, width, GUIDE_BATCH))
            self._synchronize()
            cols.append(c)
            rows.append(r)
        return torch.cat(cols), torch.cat(rows)

    def warp_u16(self, u16, q, size):
        """device u16 depth samples [n,H,W] -> the same samples in the 4K frame's framing [n,size[1],size[0]] (v3d_warp_u16_batch
        through the Q16 map q = (ax, bx, ay, by); outside the source: 0, the far plane)"""
        return self.native.warp_u16_batch(u16, *q, size[0], size[1], 0)

    def guided_upscale_u16(self, u16, luma, r, eps):
        """device u16 depth samples [n,H,W] + device luma [n,Hhi,Whi] -> device u16 4K samples [n,Hhi,Whi]"""
        return self.native.guided_upscale_u16_batch(u16, luma, r, eps)

    def render_stereo(self, u16_4k, gains, layout, subpixel=False):
        """--stereo-output: the 4K BGR frames guide_luma left in its device staging + their u16 4K depth [n,Hhi,Whi] (device)
        -> NumPy packed frames [n,outH,outW,3] (convert.output_size): one launch, one D2H, no second H2D of the 4K frames.  Slots of frames
        that had no 4K frame hold stale data; the caller drops them.  subpixel: the sub-pixel renderer (--subpixel)."""
        return self._fetch(self._render_stereo_dev(u16_4k, gains, layout, subpixel))

    def _render_stereo_dev(self, u16_4k, gains, layout, subpixel=False):
        torch, nat = self.torch, self.native
        n, H, W = u16_4k.shape
        dev = self._bufs["guide_dev"]
        from .convert import render_stereo
        oW, oH = nat.stereo_output_size(layout, W, H)
        out = self._staging("stereo_dev", (dev.shape[0], oH, oW, 3), torch.uint8, False)
        render_stereo(nat, dev[:n], u16_4k.contiguous(), *gains, layout, out[:n], subpixel)
        return out[:n]

    def render_stereo_png(self, u16_4k, gains, layout, subpixel=False):
        """--png-encoder gpu: render_stereo whose frames stay on the device and come back as the zlib streams of their PNGs"""
        return self._png_encoder().encode(self._render_stereo_dev(u16_4k, gains, layout, subpixel))


class SbsTo4kDepthPipeline:
    """SBS clip + 4K clip -> 4K 16-bit depth sequence in one pass (same files as the depth CLI followed by the upscale CLI)"""

    writer_pool_factory = PngWriterPool       # sink of the 4K 16-bit maps (and of --keep-depth-maps): the CLIs' hook

    def __init__(self,
                 model_checkpoint: str = "Intel/dpt-large",
                 work_dir: str = "temp_depth",
                 device: str = "cuda",
                 batch_size: int = 8,
                 use_neural_guidance: bool = True,
                 stereo_only: bool = False,
                 unsqueeze_sbs: bool = True,
                 radius: int = GUIDED_RADIUS,
                 eps: float = GUIDED_EPS,
                 guide_batch: int = GUIDE_BATCH,
                 backend=None,
                 mono_provider=None,
                 temporal_radius: int = 0,
                 temporal_tau: int = 12,
                 temporal_cut: int = 20,
                 temporal_fill: bool = True,
                 range_percentile: float = 100.0,
                 fill_holes: bool = False,
                 png_encoder: str = "zlib",
                 check_guide: bool = False,
                 check_guide_min: float = 0.5,
                 quality_report=None,
                 quality_bad_threshold: int = 16,
                 quality_still: int = 4,
                 quality_jump: float = 1.0,
                 temporal_motion: int = 0,
                 min_disparity=0,
                 depth_range: str = "frame",
                 input_layout: str = "sbs"):
        """backend: HipPipelineBackend (built when None) or a stand-in with its methods (host-logic tests);
        temporal_*: the depth CLI's temporal stabilisation (radius 0 = off: every frame on its own; temporal_motion > 0: the
        window follows the block matcher's motion);
        range_percentile: the depth CLI's robust white point (100 = off: the maximum);
        fill_holes: the depth CLI's hole filling of the int16 disparity (off: invalid pixels stay depth 0);
        png_encoder: "gpu" deflates every PNG this run writes on the device (png_gpu.py); "zlib" = on the writer threads;
        check_guide: score every (left view, 4K frame) pair the run uses (framematch.GuideChecker); no output PNG changes;
        quality_*: the depth CLI's --quality-report (quality.py): quality.json goes next to the kept depth maps, else next to the
        4K frames, or to the given path; no output PNG changes;
        min_disparity: the depth CLI's --min-disparity (an integer in [-64, 0] or "auto"; 0 = off: the window [0, 64));
        depth_range: the depth CLI's --depth-range ("metric": the constant range (0, 64); "frame" = off: per-frame min-max);
        input_layout: the depth CLI's --input-layout ("tb": a top-bottom clip, the left eye on top; "sbs" = side by side)"""
        if backend is None:
            require_hip_device(device)
            backend = HipPipelineBackend(device)
        self.backend = backend
        # the depth CLI's extractor supplies the model loading, the guidance provider, the cache path and the frame count
        self.extractor = HybridStereoDepthExtractor(
            model_checkpoint=model_checkpoint, work_dir=work_dir, cache_dir=work_dir, device=device, batch_size=batch_size,
            use_neural_guidance=use_neural_guidance, stereo_only=stereo_only, unsqueeze_sbs=unsqueeze_sbs, backend=backend,
            mono_provider=mono_provider, temporal_radius=temporal_radius, temporal_tau=temporal_tau, temporal_cut=temporal_cut,
            temporal_fill=temporal_fill, range_percentile=range_percentile, fill_holes=fill_holes,
            png_encoder=png_encoder, quality_report=quality_report, quality_bad_threshold=quality_bad_threshold,
            quality_still=quality_still, quality_jump=quality_jump, temporal_motion=temporal_motion, min_disparity=min_disparity,
            **({"depth_range": depth_range} if depth_range != "frame" else {}),
            **({"input_layout": input_layout} if input_layout != "sbs" else {}))
        self.radius, self.eps = radius, eps
        self.guide_batch = max(1, int(guide_batch))
        self.check_guide, self.check_guide_min = bool(check_guide), float(check_guide_min)

    def run(self, sbs_video: str, video_4k: str, output_path: str = None, start_frame: int = 0, max_frames: int = None,
            guide_start_frame: int = 0, force_reprocess: bool = False, keep_depth_maps: bool = False,
            stereo_output: str = None, stereo_options: dict = None, spatial: dict = None) -> str:
        """guide_start_frame: the 4K frame that belongs to SBS frame start_frame (as for the upscale CLI).  Returns the
        output path: an H.264 file when ffmpeg exists and it ends in .mp4, else a JSON manifest of the PNG sequence.
        stereo_output: also render every frame that has a 4K frame to side-by-side 3D from the device-resident 4K frame and
        depth (the files the convert CLI writes from this run's depth output); stereo_options: max_shift, convergence,
        eye_split, layout, subpixel (convert.py's defaults), or parallax="source" [, parallax_gain] with depth_range="metric": the
        film's own parallax (convert.source_parallax); spatial: register.resolve()'s result -- the low-res u16 depth is warped
        into the 4K frame's framing right before the guided filter (None: nothing changes)."""
        from . import sharding
        from .png_gpu import gray16_file
        ex, be = self.extractor, self.backend
        gpu_png = ex.png_encoder == "gpu"
        stereo, stereo_count = None, 0                               # convert.StereoPlan of --stereo-output, this rank's frames
        if stereo_output is not None:
            from .convert import StereoPlan
            if (stereo_options or {}).get("parallax") == "source" and ex.depth_range != "metric":
                raise ValueError("--parallax source needs --depth-range metric on the same command line: the depth must keep its scale")
            stereo = StereoPlan(**(stereo_options or {}))
            stereo_dir = sibling_frames_dir(stereo_output)
        print(f"SBS -> 4K depth: {sbs_video} + {video_4k}")
        video_info, frame_count = ex._frame_count(sbs_video, start_frame, max_frames)
        info4k = get_video_info(video_4k)
        if not info4k:
            raise ValueError(f"Could not read video info: {video_4k}")
        Whi, Hhi, fps = info4k['width'], info4k['height'], info4k['fps']
        reuse = output_path is not None and Path(output_path).exists() and not force_reprocess     # nothing will be computed
        if not reuse:
            ex.resolve_min_disparity(sbs_video, start_frame, frame_count)   # --min-disparity auto -> its integer, before anything is keyed by it
        cache_path = ex.get_cache_path(sbs_video, start_frame, frame_count) if (keep_depth_maps or output_path is None) and ex.min_disparity != "auto" else None
        if output_path is None:
            output_path = f"depth_4k_{cache_path.name}.mp4"          # what the upscale CLI names its output for that directory
        output_path = Path(output_path)
        if output_path.exists() and not force_reprocess:
            print(f"✓ Using existing depth video: {output_path}")
            ex.quality_skipped()
            return str(output_path)
        check_frame_halves(video_info['width'], video_info['height'], ex.input_layout)
        if stereo is not None:
            stereo.check_frame(Whi, Hhi)
            if stereo.parallax == "source":                          # the film's parallax: the window is resolved, the sizes are known
                stereo.resolve_source({"mode": "metric", "eye_width": ex.eye_size(video_info)[0], "min_disparity": ex.min_disparity}, Whi,
                                      None if spatial is None else spatial["map"])
            stereo_dir.mkdir(parents=True, exist_ok=True)
            stereo_encode = stereo.encoder(gpu_png)
        warp = None
        if spatial is not None:                                      # every rank applies the same map: nothing to exchange
            from .register import warp_q16
            warp = warp_q16(spatial["map"], ex.eye_size(video_info), (Whi, Hhi))
            print(f"Spatial map {tuple(spatial['map'])} from {spatial['source']}: depth warped to {warp['size'][0]}x{warp['size'][1]} before the guided filter")
        if not ex.model_loaded:
            ex.load_model()

        rank, world = sharding.rank_world()
        sharding.require_initialized(world)
        check = ex.guide_check = None
        if self.check_guide:
            from .framematch import GuideChecker
            # round-robin sharding leaves a rank every world-th frame: per-pair scores only, no in-batch shift
            check = ex.guide_check = GuideChecker(be, self.check_guide_min, consecutive=world == 1 or ex.temporal[0] > 0)
        frames_dir = sibling_frames_dir(output_path)
        frames_dir.mkdir(parents=True, exist_ok=True)
        # the extractor's frame plan: frame i -> rank i mod world, or -- with temporal stabilisation -- a contiguous block per
        # rank plus a halo of SBS frames that is decoded and matched but not written.  Each rank decodes only its own frames
        # of BOTH clips: the 4K guides are the frames it owns (4K frame g0 + i guides SBS frame i)
        g0 = max(int(guide_start_frame), 0)
        first, count, stride, offset = ex.frame_plan(frame_count, rank, world)[1]
        guides = iter_frames(video_4k, g0 + first, count, stride=stride, offset=offset) if count else iter(())
        guide_state = {"delivered": 0, "ended": False}
        flat = written = 0

        def next_guide():
            if guide_state["ended"]:
                return None
            f = next(guides, None)
            if f is None:
                guide_state["ended"] = True
                print(f"Warning: 4K guide video ended after {guide_state['delivered']} of this rank's frames; the "
                      f"remaining depth frames are upsampled with a flat guide")
                return None
            guide_state["delivered"] += 1
            return f

        def emit(writers, out_idx, u16):
            """the u16 depth samples of frames out_idx -> [depth PNGs,] guided filter, 4K PNGs [, stereo frames]"""
            nonlocal flat, written, stereo_count
            written += len(out_idx)
            gb = min(self.guide_batch, ex.last_pass_frames)         # the driver has sized the pass before its first yield
            if keep_depth_maps:
                ex.submit_depth_maps(writers, cache_path, out_idx, u16)
            for j0 in range(0, len(out_idx), gb):
                idx = out_idx[j0:j0 + gb]
                frames = [next_guide() for _ in idx]
                flat += sum(f is None for f in frames)
                luma = be.guide_luma(frames, Hhi, Whi, gb)
                lo = u16[j0:j0 + len(idx)]
                if warp is not None:
                    lo = be.warp_u16(lo, warp["q"], warp["size"])
                q_dev = be.guided_upscale_u16(lo, luma, self.radius, self.eps)
                pending = check.emit(idx, frames, luma) if check is not None else None
                if gpu_png:                                        # deflated on the device: only the streams cross PCIe
                    for i, s in zip(idx, be.png_streams_u16(q_dev)):
                        writers.submit(frames_dir / f"depth4k_{i:06d}.png", s, encode=gray16_file(Whi, Hhi))
                else:
                    q = be.to_host_u16(q_dev)
                    for j, i in enumerate(idx):
                        writers.submit(frames_dir / f"depth4k_{i:06d}.png", q[j])
                if pending is not None:                            # behind the batch's own synchronise: nothing waits here
                    check.collect(pending)
                if stereo is not None and any(f is not None for f in frames):
                    render = be.render_stereo_png if gpu_png else be.render_stereo
                    sbs3d = render(q_dev, stereo.gains, stereo.layout_code, **stereo.render_kwargs())
                    for j, i in enumerate(idx):
                        if frames[j] is not None:                   # no 4K frame: no stereo frame (its slot is stale)
                            writers.submit(stereo_dir / f"frame_{i:06d}.png", sbs3d[j], encode=stereo_encode)
                            stereo_count += 1
            print(f"✓ Queued {len(out_idx)} 4K depth maps (rank {rank})")

        with self.writer_pool_factory() as writers:
            for idx, u16 in ex.iter_depth_u16(sbs_video, start_frame, frame_count, video_info, rank, world):
                emit(writers, idx, u16)
        self.last_pass_frames, self.last_decoded_frames = ex.last_pass_frames, ex.last_decoded_frames
        self.last_flat_guides = flat
        n = sharding.total(written)
        if n == 0:
            raise ValueError("No frames extracted from video")
        n_stereo = sharding.total(stereo_count) if stereo is not None else 0
        if check is not None:
            check.finish(sharding.total)
            if rank == 0:
                check.report()
        ex.finish_quality(cache_path if keep_depth_maps else frames_dir, rank)
        sharding.barrier()
        if rank == 0:
            from .register import manifest_entries
            encode_depth4k(frames_dir, output_path, n, Whi, Hhi, fps, self.radius, self.eps,
                           {**(ex.manifest_extra() or {}), **manifest_entries(spatial)} or None)
            if keep_depth_maps:
                ex.write_side_files(cache_path)
            if stereo is not None and n_stereo:
                stereo.finish(stereo_dir, stereo_output, n_stereo, fps)
        sharding.barrier()
        print(f"✓ Depth video saved: {output_path}")
        if stereo is not None:
            print(f"✓ 3D video saved: {stereo_output} ({n_stereo} frames)")
        return str(output_path)


def _resolve_spatial(args, resolve):
    """--alignment-file's spatial block / --spatial-map / --no-spatial -> what the run applies (None: nothing); the clips' sizes are
    only read when there is something to compare them with"""
    if args.no_spatial or (args.alignment_file is None and args.spatial_map is None):
        return None
    unsqueeze = not args.no_unsqueeze
    layout = input_layout_options(args)

    def eye():
        info = get_video_info(args.video)
        return None if not info else list(sbs_eye_size(info, unsqueeze, **layout))

    def guide():
        info = get_video_info(args.video_4k)
        return None if not info else [info["width"], info["height"]]
    return resolve(args.alignment_file, False, args.spatial_map, eye, guide, unsqueeze, **layout)


def main(argv=None):
    """ Command line interface: SBS clip + 4K clip -> 4K depth sequence """
    parser = argparse.ArgumentParser(description='SBS stereoscopic video + 4K video -> 4K depth sequence in one pass')
    parser.add_argument('video', help='Path to SBS video file')
    parser.add_argument('video_4k', help='Path to 4K 2D video (dimensions and guide frames)')
    parser.add_argument('--output', help='Output path for 4K depth video')
    add_depth_arguments(parser, 'Force reprocessing even if the output exists')
    from .align import add_guide_arguments, resolve_guide_start
    add_guide_arguments(parser, 'the first SBS frame')
    parser.add_argument('--keep-depth-maps', action='store_true',
                        help="Also write the 1080p depth_%%06d.png maps into the depth CLI's cache directory")
    parser.add_argument('--stereo-output', default=None,
                        help='Also render side-by-side 3D to this path (what the convert CLI makes from the depth output)')
    parser.add_argument('--check-guide', action='store_true',
                        help='Score every SBS frame against the 4K frame it is filtered with (frame signatures on the GPU) and '
                             'warn when the guide looks misaligned; no output changes')
    parser.add_argument('--check-guide-min', type=float, default=0.5, help='Score below which a pair counts as bad (default 0.5)')
    from .convert import add_stereo_arguments, stereo_options
    add_stereo_arguments(parser)
    from .register import add_apply_arguments, resolve
    add_apply_arguments(parser)
    args = parser.parse_args(argv)
    if not resolve_guide_start(args):
        return 1
    try:
        stereo = stereo_options(args)            # refuses --parallax source beside an invented parallax before anything is opened
        spatial = _resolve_spatial(args, resolve)
        from . import sharding
        sharding.init_process_group()            # no-op for one process; under torchrun: one rank per GPU (sets the device)
        pipe = SbsTo4kDepthPipeline(check_guide=args.check_guide, check_guide_min=args.check_guide_min, **depth_options(args))
        output_path = pipe.run(args.video, args.video_4k, output_path=args.output, start_frame=args.start_frame,
                               max_frames=args.max_frames, guide_start_frame=args.guide_start_frame,
                               force_reprocess=args.force, keep_depth_maps=args.keep_depth_maps,
                               stereo_output=args.stereo_output, stereo_options=stereo, spatial=spatial)
        print(f"\n✓ Success! 4K depth video: {output_path}")
    except Exception as e:
        print(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    exit(main())
