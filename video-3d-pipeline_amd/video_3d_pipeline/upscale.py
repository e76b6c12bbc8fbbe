"""Depth upscaling to the 4K frame -- MI355X-native host side.

Mirror of reference src/video_3d_pipeline/upscale.py (class / method names, argument meaning, skip-if-
exists and error behaviour, CLI flags).  The reference shells out to ffmpeg's `scale` filter + H.264
(upscale.py:47-63) and never looks at the 4K pixels; BASELINE.json re-specifies the step as
guided-filter joint upsampling with the 4K frame as guide, which is what
v3d_guided_upscale computes here.  `use_nvenc` is accepted for signature compatibility (NVENC is an
NVIDIA encoder); H.264 encoding is used only if an ffmpeg binary exists at run time, otherwise the
4K depth frames are written as 16-bit PNGs and `output_path` becomes a small JSON manifest.
"""
import argparse
import glob
import json
import os
from pathlib import Path

import numpy as np

from .backend import HipBackend
from .utils import PngWriterPool, finish_sequence, get_video_info, iter_frames, prefetch_map, read_png16, sibling_frames_dir

GUIDED_RADIUS = 8       # at 4K; the reference specifies nothing
GUIDED_EPS = 1e-3       # on [0,1]-scaled guide


def encode_depth4k(frames_dir: Path, output_path, count: int, width: int, height: int, fps: float, radius: int, eps: float,
                   extra: dict = None):
    """the last step of a 4K depth run, on one process: the manifest of frames_dir/depth4k_%06d.png, through finish_sequence
    (`extra`: further entries of the manifest, e.g. the temporal stabilisation parameters of the run)"""
    finish_sequence(frames_dir, "depth4k_%06d.png", output_path, fps, {
        "format": "png16-sequence", "frames_dir": str(frames_dir), "pattern": "depth4k_%06d.png",
        "count": count, "width": width, "height": height, "fps": fps,
        "guided_radius": radius, "guided_eps": eps, **(extra or {}),
        "note": "no ffmpeg binary on this host: 4K depth frames kept as 16-bit PNGs"})


def depth_range_entry(depth_dir) -> dict:
    """the depth CLI's depth_range.json (--depth-range metric) as an entry of the 4K manifest: the guided filter keeps the samples'
    scale, so what a sample means travels with them to the convert CLI ({} without the file)"""
    side = Path(depth_dir) / "depth_range.json"
    if not side.is_file():
        return {}
    try:
        block = json.loads(side.read_text())
    except ValueError:
        return {}
    return {"depth_range": block} if isinstance(block, dict) else {}


def input_layout_entry(depth_dir) -> dict:
    """the depth CLI's input_layout.json (--input-layout tb) as an entry of the 4K manifest, where the convert CLI looks for it ({}
    without the file: side by side)"""
    side = Path(depth_dir) / "input_layout.json"
    if not side.is_file():
        return {}
    try:
        block = json.loads(side.read_text())
    except ValueError:
        return {}
    return {"input_layout": block["input_layout"]} if isinstance(block, dict) and isinstance(block.get("input_layout"), str) else {}


class HipUpscaleBackend(HipBackend):
    def to_luma(self, frame_bgr):
        d = frame_bgr if self.torch.is_tensor(frame_bgr) else self.native.to_device(frame_bgr, self.device)
        return d if d.dim() == 2 else self.native.bgr_to_gray(d.contiguous())

    def upscale(self, depth_lo, guide, r, eps):
        nat = self.native
        d = depth_lo if self.torch.is_tensor(depth_lo) else nat.to_device(np.asarray(depth_lo, np.float32), self.device)
        g = self.to_luma(guide)
        return nat.guided_upscale(d.contiguous(), g.contiguous(), r, eps)

    def upscale_u16(self, depth_lo, guide, r, eps) -> np.ndarray:
        """guided upscale, rounded and clamped to the 16-bit range of the PNG sink"""
        q = self.upscale(depth_lo, guide, r, eps)
        # v3d_round_to_u16: the uint16 bit pattern leaves the device as 2 bytes per pixel
        return self.native.round_to_u16(q.contiguous()).cpu().numpy().view(np.uint16)

    def upscale_png(self, depth_lo, guide, r, eps):
        """--png-encoder gpu: upscale_u16 whose samples stay on the device and come back as the zlib stream of their PNG"""
        q = self.upscale(depth_lo, guide, r, eps)
        return self._png_encoder().encode(self.native.round_to_u16(q.contiguous())[None])[0]

    def warp_u16(self, depth_u16: np.ndarray, q, size):
        """the u16 samples of a depth PNG -> the same samples in the 4K frame's framing as device float32 [size[1],size[0]]
        (v3d_warp_u16_batch through the Q16 map q = (ax, bx, ay, by); outside the source: 0, the far plane), what upscale() takes"""
        d = self.native.to_device(np.ascontiguousarray(depth_u16, dtype=np.uint16).view(np.int16)[None], self.device)
        w = self.native.warp_u16_batch(d, *q, size[0], size[1], 0)[0]
        return (w.to(self.torch.int32) & 0xFFFF).to(self.torch.float32)

    def flat_guide(self, h, w):
        return self.torch.full((h, w), 128, dtype=self.torch.uint8, device=self.device)


class SimpleDepthUpscaler:
    """ Depth upscaling to the 4K frame (guided filter on the GPU) """

    writer_pool_factory = PngWriterPool       # sink of the 4K 16-bit maps (see HybridStereoDepthExtractor.writer_pool_factory)

    def __init__(self, use_nvenc: bool = True, radius: int = GUIDED_RADIUS, eps: float = GUIDED_EPS,
                 device: str = "cuda", backend=None, png_encoder: str = "zlib", spatial: dict = None):
        """png_encoder: "gpu" deflates the 4K maps on the device (png_gpu.py); "zlib" = on the writer threads;
        spatial: register.resolve()'s result -- every low-res depth map is warped into the 4K frame's framing right before the
        guided filter (None: nothing changes)"""
        self.spatial = spatial
        from .png_gpu import check_png_encoder
        self.png_encoder = check_png_encoder(png_encoder)
        self.use_nvenc = use_nvenc
        self.radius, self.eps = radius, eps
        self.backend = backend if backend is not None else HipUpscaleBackend(device)
        print(f"Initializing Simple Depth Upscaler...")
        print(f"NVENC encoding: {self.use_nvenc}")

    def upscale_frame(self, depth_lo: np.ndarray, guide_4k: np.ndarray) -> np.ndarray:
        """NumPy surface: HxW float32 depth + 2Hx2W(x3) uint8 guide (BGR or luma) -> 2Hx2W float32"""
        return self.backend.upscale(depth_lo, guide_4k, self.radius, self.eps).cpu().numpy()

    def upscale_depth_maps_ffmpeg(self, depth_dir: str, target_width: int, target_height: int,
                                  output_path: str, fps: float = 23.976, video_4k_path: str = None,
                                  guide_start_frame: int = 0):
        """ Upscale the depth_%06d.png sequence to target_width x target_height (name kept from the reference).
        guide_start_frame: index of the 4K frame that belongs to depth_000000 -- the alignment offset that
        run_pipeline.py:45-50 computes and then drops; round(offset_seconds * fps), clamped at 0. """
        from . import sharding
        from .png_gpu import gray16_file

        print(f"Processing depth upscaling...")
        print(f"Input: {depth_dir}")
        print(f"Output: {output_path}")
        print(f"Target: {target_width}x{target_height} @ {fps}fps")

        depth_files = sorted(glob.glob(os.path.join(depth_dir, "depth_*.png")))
        if not depth_files:
            raise ValueError(f"No depth maps found in {depth_dir}")
        print(f"Found {len(depth_files)} depth maps")

        rank, world = sharding.rank_world()
        sharding.require_initialized(world)           # never a silent single-rank fallback under torchrun
        frames_dir = sibling_frames_dir(output_path)
        frames_dir.mkdir(parents=True, exist_ok=True)
        n = len(depth_files)
        g0 = max(int(guide_start_frame), 0)
        # The DECODER decides how many guide frames exist; the container's frame count is only a hint (cv2's
        # CAP_PROP_FRAME_COUNT and duration * fps are both unreliable).  A clip that ends early degrades the remaining
        # depth frames to a flat guide (plain smoothing upsample) with a warning; one that runs longer is simply used.
        n_hint = None
        if video_4k_path:
            info = get_video_info(video_4k_path)
            if info:
                total = info.get('frames', 0) or int(info['duration'] * info['fps'])
                n_hint = max(0, min(n, total - g0))
            else:
                print(f"Warning: could not read video info of {video_4k_path}; decoding it anyway")
        # the guide video is decoded ONCE, by rank 0 (one rank: directly into the filter; several: into the round exchange)
        guides = iter_frames(video_4k_path, g0, n) if (video_4k_path and rank == 0) else None
        decoded = [0, False]                                  # rank 0: guide frames delivered so far, decoder ended

        def next_luma():
            """rank 0: the next guide frame as a device luma tensor (the BGR frame crosses PCIe once, the luma stays on
            the device), or None once the decoder has ended"""
            if decoded[1]:
                return None
            f = next(guides, None)
            if f is None:
                decoded[1] = True
                if n_hint is not None and decoded[0] < n_hint:
                    print(f"Warning: 4K guide video ended after {decoded[0]} frames (container promised {n_hint}); "
                          f"depth frames from {decoded[0]} on are upsampled with a flat guide")
                return None
            decoded[0] += 1
            return self.backend.to_luma(f)

        exchange = None
        if world > 1 and video_4k_path:
            exchange = sharding.GuideRoundExchange((target_height, target_width), self.backend.device)

        def post_round(base):
            """rank 0 decodes the guide frames of depth frames base .. base+world-1 and posts the round (one collective).
            Every rank posts the same ceil(n / world) rounds -- the count depends on the depth files only, which all
            ranks see; what the decoder really delivered travels in the round's validity bitmap.  A decoder failure on
            rank 0 is posted as an aborted round first, so the other ranks raise instead of waiting in the collective."""
            if base >= n:
                return False
            if rank != 0:
                exchange.post()
                return True
            try:
                frames = [next_luma() if base + r < n else None for r in range(world)]
            except Exception:
                exchange.post(abort=True)
                raise
            exchange.post(frames)
            return True

        # this rank's depth maps, decoded a few files ahead on reader threads (PNG inflate is the slowest host step)
        my_depth = prefetch_map(read_png16, [depth_files[i] for i in range(rank, n, world)])
        flat, warp = 0, None                                          # warp: every rank applies the same map, nothing to exchange
        with self.writer_pool_factory() as writers:                  # 4K 16-bit PNGs: ~80 ms of zlib each, compressed off the main thread
            posted = post_round(0) if exchange is not None else False
            for base in range(0, n, world):
                # one round ahead: the collective of round base+world runs on the exchange's side stream while this
                # round's filter runs on the main stream
                posted_next = post_round(base + world) if exchange is not None else False
                i = base + rank
                guide = None
                if exchange is not None:
                    if posted:
                        guide = exchange.take()           # raises GuideExchangeAborted on every rank if rank 0's decoder failed
                elif guides is not None and i < n:        # one rank
                    guide = next_luma()
                posted = posted_next
                if i >= n:
                    continue
                if guide is None:
                    flat += 1
                    guide = self.backend.flat_guide(target_height, target_width)    # beyond the 4K clip: flat guide == plain smoothing upsample
                d16 = next(my_depth)
                if self.spatial is not None:
                    if warp is None:
                        from .register import check_block_size, warp_q16
                        check_block_size(self.spatial, d16.shape[1], d16.shape[0])
                        warp = warp_q16(self.spatial["map"], (d16.shape[1], d16.shape[0]), (target_width, target_height))
                    d16 = self.backend.warp_u16(d16, warp["q"], warp["size"])
                else:
                    d16 = d16.astype(np.float32)
                if self.png_encoder == "gpu":
                    writers.submit(frames_dir / f"depth4k_{i:06d}.png", self.backend.upscale_png(d16, guide, self.radius, self.eps),
                                   encode=gray16_file(target_width, target_height))
                    continue
                writers.submit(frames_dir / f"depth4k_{i:06d}.png", self.backend.upscale_u16(d16, guide, self.radius, self.eps))
        self.last_flat_guides = flat
        if rank == 0 and guides is not None and n_hint is not None and decoded[0] > n_hint:
            print(f"Note: the 4K video delivered {decoded[0]} guide frames, the container promised {n_hint}")
        sharding.barrier()

        if rank == 0:
            from .register import manifest_entries
            encode_depth4k(frames_dir, output_path, n, target_width, target_height, fps, self.radius, self.eps,
                           {**depth_range_entry(depth_dir), **input_layout_entry(depth_dir), **manifest_entries(self.spatial)} or None)
        sharding.barrier()
        print(f"✓ Depth video saved: {output_path}")
        return output_path

    def process_depth_upscaling(self, depth_dir: str, video_4k_path: str, output_path: str = None,
                                force_reprocess: bool = False, guide_start_frame: int = 0) -> str:
        """ Main pipeline for depth upscaling """
        print(f"Processing depth upscaling...")
        print(f"Depth maps: {depth_dir}")
        print(f"4K video: {video_4k_path}")

        video_info = get_video_info(video_4k_path)
        if not video_info:
            raise ValueError(f"Could not read video info: {video_4k_path}")
        target_width, target_height, fps = video_info['width'], video_info['height'], video_info['fps']
        print(f"Target resolution: {target_width}x{target_height} @ {fps}fps")

        if output_path is None:
            depth_dir_name = Path(depth_dir).name
            output_path = f"depth_4k_{depth_dir_name}.mp4"
        output_path = Path(output_path)

        if output_path.exists() and not force_reprocess:
            print(f"✓ Using existing depth video: {output_path}")
            return str(output_path)

        result = self.upscale_depth_maps_ffmpeg(depth_dir=depth_dir, target_width=target_width, target_height=target_height,
                                                output_path=str(output_path), fps=fps, video_4k_path=video_4k_path,
                                                guide_start_frame=guide_start_frame)
        print(f"✓ Depth upscaling complete!")
        print(f"  Input: {depth_dir}")
        print(f"  Output: {result}")
        print(f"  Resolution: {target_width}x{target_height}")
        return result


def main(argv=None, backend=None):
    """ Command line interface for depth upscaling (backend: a stand-in for host tests) """
    parser = argparse.ArgumentParser(description='Depth upscaling to the 4K frame (guided filter)')
    parser.add_argument('depth_dir', help='Directory containing depth maps')
    parser.add_argument('video_4k', help='Path to 4K 2D video (dimensions and guide frames)')
    parser.add_argument('--output', help='Output path for 4K depth video')
    parser.add_argument('--no-nvenc', action='store_true', help='Disable NVENC, use CPU encoding')
    parser.add_argument('--force', action='store_true', help='Force reprocessing even if output exists')
    from .align import add_guide_arguments, resolve_guide_start
    add_guide_arguments(parser, 'depth_000000')
    from .png_gpu import add_png_arguments, png_options
    add_png_arguments(parser)
    from .register import add_apply_arguments, resolve
    add_apply_arguments(parser)
    args = parser.parse_args(argv)
    if not resolve_guide_start(args):
        return 1
    try:
        spatial = None
        if not args.no_spatial and (args.alignment_file is not None or args.spatial_map is not None):
            def guide_size():
                info = get_video_info(args.video_4k)
                return None if not info else [info["width"], info["height"]]
            spatial = resolve(args.alignment_file, False, args.spatial_map, None, guide_size)
            if spatial is not None:
                print(f"Spatial map {spatial['map']} from {spatial['source']}: depth maps are warped before the guided filter")
        from . import sharding
        sharding.init_process_group()            # no-op for one process; under torchrun: one rank per GPU (sets the device)
        upscaler = SimpleDepthUpscaler(use_nvenc=not args.no_nvenc, backend=backend, spatial=spatial, **png_options(args))
        output_path = upscaler.process_depth_upscaling(depth_dir=args.depth_dir, video_4k_path=args.video_4k,
                                                       output_path=args.output, force_reprocess=args.force,
                                                       guide_start_frame=args.guide_start_frame)
        print(f"\n✓ Success! 4K depth video: {output_path}")
        print(f"Ready for VisionDepth3D processing!")
    except Exception as e:
        print(f"Error: {e}")
        return 1
    return 0


if __name__ == "__main__":
    exit(main())
