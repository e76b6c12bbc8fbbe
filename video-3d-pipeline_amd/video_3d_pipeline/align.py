"""Audio-only temporal alignment (mirror of the reference's align.py and of utils.py:137-165 find_audio_offset).

The two audio tracks are decoded on the host (utils.load_audio) and checked there; the normalisation, the FFT
cross-correlation and the peak search run in libv3d_hip (v3d_align_audio).  Everything that can make the alignment
impossible -- a missing file, no audio track, no decoder, a silent track, differing sample rates -- is detected before
the first GPU call and raised as a RuntimeError that names --skip-alignment.  No correlation plot is drawn (the
reference's plot_audio_correlation needs matplotlib, which this package does not require).

Optional second step, not in the reference: --refine-video matches frames of the two clips on the device around the rounded audio
offset and --video-only does so without an audio step (framematch.py); alignment_data.json then also carries guide_start_frame,
which guide_start_frame_from prefers.  --register-spatial (register.py) then fits the left eye to the 4K frame's framing on the
device and adds a "spatial" block, which the upscale and pipeline CLIs apply to the low-res depth.
"""
import argparse
import json
from pathlib import Path
from typing import Dict, Optional

import numpy as np

from .utils import create_work_directory, get_video_info, load_audio

_SKIP = "run the pipeline with --skip-alignment, or align the clips by hand and pass --guide-start-frame"


def _fail(msg: str):
    raise RuntimeError(f"audio alignment impossible: {msg}; {_SKIP}")


class VideoAligner:
    """Audio-only temporal alignment - no video re-encoding.  The constructor touches neither the disk nor the GPU."""

    def __init__(self, video1_path: str, video2_path: str, work_dir: str = "temp_alignment"):
        self.video1_path = video1_path
        self.video2_path = video2_path
        self.work_dir = Path(work_dir)          # created by find_alignment when it writes alignment_data.json
        self.video1_info = None
        self.video2_info = None

    def _load(self, path: str, max_audio_length: float):
        try:
            audio, rate = load_audio(path, max_seconds=max_audio_length)
        except FileNotFoundError:
            _fail(f"{path} does not exist")
        except LookupError as e:
            _fail(f"no audio track: {e}")
        except (RuntimeError, ValueError, OSError) as e:
            _fail(f"cannot decode the audio of {path}: {e}")
        if audio.size == 0:
            _fail(f"{path} has an empty audio track")
        if audio.max() == audio.min():                 # population std 0: find_audio_offset would divide by 1e-10
            _fail(f"the audio track of {path} is silent (constant)")
        if not np.isfinite(audio).all():
            _fail(f"the audio track of {path} holds non-finite samples")
        return audio, rate

    def _info(self, path: str):
        info = get_video_info(path)
        if not info or not info.get("fps"):
            _fail(f"could not read the video information of {path}")
        return info

    def find_alignment(self, max_audio_length: float = 300) -> Dict:
        """Find temporal alignment and return offset data (the reference's ten keys); also written to
        work_dir/alignment_data.json."""
        audio1, sr1 = self._load(self.video1_path, max_audio_length)
        audio2, sr2 = self._load(self.video2_path, max_audio_length)
        if sr1 != sr2:
            _fail(f"sample rate mismatch: {sr1} Hz vs {sr2} Hz")
        if audio1.size + audio2.size - 1 > 2 ** 26:
            _fail(f"{audio1.size} + {audio2.size} samples exceed the largest correlation (2^26 lags); lower max_audio_length")
        self.video1_info = self._info(self.video1_path)
        self.video2_info = self._info(self.video2_path)
        print(f"Video 1: {self.video1_info['width']}x{self.video1_info['height']} "
              f"@ {self.video1_info['fps']:.2f} fps, {self.video1_info['duration']:.1f}s")
        print(f"Video 2: {self.video2_info['width']}x{self.video2_info['height']} "
              f"@ {self.video2_info['fps']:.2f} fps, {self.video2_info['duration']:.1f}s")

        import torch
        from . import _native
        print("Computing audio cross-correlation (GPU FFT)...")
        dev = _native.resolve_device(None)
        with torch.cuda.device(dev):
            res = _native.align_audio(_native.to_device(audio1, dev), _native.to_device(audio2, dev)).cpu().numpy()
        lag, correlation_strength = int(res[0]), float(res[2])
        time_offset = lag / sr1
        print(f"Audio offset: {time_offset:.3f}s, correlation strength: {correlation_strength:.4f}")
        print("Correlation plot: not drawn (matplotlib is not a dependency of this build)")

        frame_duration = 1.0 / self.video1_info['fps']
        offset_frames = time_offset / frame_duration
        print(f"Audio alignment: {time_offset:.3f}s offset ({offset_frames:.1f} frames)")
        print(f"Correlation strength: {correlation_strength:.4f}")
        alignment_data = {
            'video1_path': str(self.video1_path),
            'video2_path': str(self.video2_path),
            'time_offset_seconds': float(time_offset),
            'offset_frames': float(offset_frames),
            'correlation_strength': float(correlation_strength),
            'frame_duration': float(frame_duration),
            'video1_fps': self.video1_info['fps'],
            'video2_fps': self.video2_info['fps'],
            'sample_rate': int(sr1),
            'audio_length_analyzed': float(max_audio_length)
        }
        self.work_dir = create_work_directory(str(self.work_dir))
        alignment_file = self.work_dir / 'alignment_data.json'
        with open(alignment_file, 'w') as f:
            json.dump(alignment_data, f, indent=2)
        print(f"Alignment data saved to: {alignment_file}")
        return alignment_data

    def video_only_data(self) -> Dict:
        """--video-only: the reference's ten keys without an audio step; what only the audio gives is null"""
        self.video1_info = self._info(self.video1_path)
        self.video2_info = self._info(self.video2_path)
        return {
            'video1_path': str(self.video1_path),
            'video2_path': str(self.video2_path),
            'time_offset_seconds': None,
            'offset_frames': None,
            'correlation_strength': None,
            'frame_duration': 1.0 / self.video1_info['fps'],
            'video1_fps': self.video1_info['fps'],
            'video2_fps': self.video2_info['fps'],
            'sample_rate': None,
            'audio_length_analyzed': None
        }

    def refine_video(self, alignment_data: Dict, seed: int, seed_audio: Optional[int], backend=None, **options) -> Dict:
        """Match frames around the seed (framematch.refine: signatures and their correlation on the GPU), add the visual keys
        to alignment_data and write alignment_data.json again.  The ten keys of the audio step stay as they are."""
        from .framematch import alignment_keys, refine
        print(f"Refining the guide start frame around {seed} by frame matching (GPU signatures)...")
        res = refine(self.video1_path, self.video2_path, seed, backend=backend, **options)
        alignment_data.update(alignment_keys(res, seed_audio))
        score = "n/a" if res["score"] is None else f"{res['score']:.4f}"
        margin = "n/a" if res["margin"] is None else f"{res['margin']:.4f}"
        print(f"Video refinement: {res['status']}, shift {res['shift']:+d} frames (best {res['best_shift']:+d}, score {score}, "
              f"margin {margin}, probe shifts {res['probe_shifts']}); guide start frame {alignment_data['guide_start_frame']}")
        if res["status"] == "inconsistent":
            print("Warning: the probes disagree (differing cuts or drift between the clips); the seed is kept")
        elif res["status"] == "undetermined":
            print("Warning: the frames do not decide the shift (static or flat scene, too few informative frames); the seed is kept")
        self.work_dir = create_work_directory(str(self.work_dir))
        alignment_file = self.work_dir / 'alignment_data.json'
        with open(alignment_file, 'w') as f:
            json.dump(alignment_data, f, indent=2)
        print(f"Alignment data saved to: {alignment_file}")
        return alignment_data

    def register_spatial(self, alignment_data: Dict, guide_start_frame: int, backend=None, **options) -> Dict:
        """Fit the left eye of video1 to the frames of video2 (register.estimate: profiles and their match on the GPU), add the
        "spatial" block to alignment_data and write alignment_data.json again.  Every other key stays as it is."""
        from .register import estimate, spatial_block
        print(f"Registering the left eye to the 4K frame from guide start frame {guide_start_frame} (GPU profiles)...")
        res = estimate(self.video1_path, self.video2_path, guide_start_frame, backend=backend, **options)
        alignment_data["spatial"] = spatial_block(res)
        score = "n/a" if res["score"] is None else ", ".join(f"{v:.4f}" for v in res["score"])
        print(f"Spatial registration: {res['status']}, map (Ax, Bx, Ay, By) = {tuple(res['map'])}, scores {score}")
        if res["status"] == "inconsistent":
            print("Warning: the probe frames disagree (a film that switches aspect ratio?); the identity is kept")
        elif res["status"] == "undetermined":
            print("Warning: the frames do not decide the map (flat or dark probes, weak texture); the identity is kept")
        self.work_dir = create_work_directory(str(self.work_dir))
        alignment_file = self.work_dir / 'alignment_data.json'
        with open(alignment_file, 'w') as f:
            json.dump(alignment_data, f, indent=2)
        print(f"Alignment data saved to: {alignment_file}")
        return alignment_data

    def assess_alignment_quality(self, alignment_data: Dict, tolerance_frames: float = 2.0) -> str:
        """Assess alignment quality and provide recommendations."""
        return assess_alignment_quality(alignment_data, tolerance_frames)


def assess_alignment_quality(alignment_data: Dict, tolerance_frames: float = 2.0) -> str:
    """The reference's grades: EXCELLENT (|offset| < tolerance_frames frames), else GOOD (strength > 0.8), MODERATE
    (> 0.6) or POOR."""
    offset = alignment_data['time_offset_seconds']
    correlation = alignment_data['correlation_strength']
    frame_duration = alignment_data['frame_duration']
    precision_limit = frame_duration * tolerance_frames

    print("\nAlignment Assessment:")
    print(f"Frame precision limit: ±{precision_limit:.3f}s ({tolerance_frames} frames)")
    if abs(offset) < precision_limit:
        quality = "EXCELLENT"
        print(f"✓ {quality}: Offset {offset:.3f}s is within frame precision")
        print("Videos are already well-aligned - no adjustment needed")
    elif correlation > 0.8:
        quality = "GOOD"
        print(f"✓ {quality}: Strong correlation ({correlation:.3f})")
        print(f"Apply {offset:.3f}s offset in processing pipeline")
    elif correlation > 0.6:
        quality = "MODERATE"
        print(f"⚠ {quality}: Acceptable correlation ({correlation:.3f})")
        print(f"Apply {offset:.3f}s offset - verify results")
    else:
        quality = "POOR"
        print(f"✗ {quality}: Low correlation ({correlation:.3f})")
        print("Videos may not be from same source or need manual sync")
    return quality


def apply_offset_to_pipeline(alignment_file: str, target_video: str, output_path: str, start_time: float = 0,
                             duration: Optional[float] = None) -> float:
    """Start time (seconds) in target_video that matches start_time of the reference (video1); clamped at 0 as in the
    reference.  output_path and duration are accepted for the reference's signature and unused there too."""
    alignment_data = load_alignment_data(alignment_file)
    offset = alignment_data['time_offset_seconds']
    if target_video == alignment_data['video1_path']:
        adjusted_start = start_time
        print(f"Video1 (reference): start at {adjusted_start:.3f}s")
    elif target_video == alignment_data['video2_path']:
        adjusted_start = start_time + offset
        print(f"Video2 (offset): start at {adjusted_start:.3f}s (original: {start_time:.3f}s + {offset:.3f}s offset)")
    else:
        raise ValueError(f"Target video {target_video} not found in alignment data")
    if adjusted_start < 0:
        print(f"Warning: Adjusted start time {adjusted_start:.3f}s < 0, using 0")
        adjusted_start = 0
    print(f"Use start_time={adjusted_start:.3f}s for {target_video}")
    return adjusted_start


def load_alignment_data(alignment_file: str) -> Dict:
    """Load previously computed alignment data."""
    alignment_path = Path(alignment_file)
    if not alignment_path.exists():
        raise FileNotFoundError(f"Alignment file not found: {alignment_file}")
    with open(alignment_path, 'r') as f:
        return json.load(f)


def guide_start_frame_from(alignment_file: str, video_4k: str) -> int:
    """--alignment-file of the upscale / pipeline CLIs: the 4K frame that matches the first SBS frame: the file's
    guide_start_frame when it has one (--refine-video / --video-only wrote it), else
    round(time_offset_seconds * fps of the 4K clip).  A negative offset (the 4K clip starts later) is not clamped:
    ValueError naming the SBS --start-frame that compensates, round(-offset * video1_fps)."""
    data = load_alignment_data(alignment_file)
    if data.get('guide_start_frame') is not None:
        g = int(data['guide_start_frame'])
        if g < 0:
            raise ValueError(_negative_start_advice(alignment_file, f"{-g} frames", -g))
        return g
    offset = float(data['time_offset_seconds'])
    info = get_video_info(video_4k)
    if not info or not info.get("fps"):
        raise ValueError(f"could not read the frame rate of {video_4k}")
    if offset < 0:
        sbs_fps = float(data.get('video1_fps') or info['fps'])
        raise ValueError(_negative_start_advice(alignment_file, f"{-offset:.3f}s", int(round(-offset * sbs_fps))))
    return int(round(offset * float(info['fps'])))


def _negative_start_advice(alignment_file, by: str, start_frame: int) -> str:
    return (f"{alignment_file}: the 4K clip starts {by} after the SBS clip (negative offset); "
            f"start the SBS side at --start-frame {start_frame} and pass "
            f"--guide-start-frame 0 instead of --alignment-file")


def add_guide_arguments(parser, frame0_help: str, offset_help: str = 'alignment offset in frames'):
    """--guide-start-frame | --alignment-file of the upscale, pipeline and convert CLIs; frame0_help: what 4K frame N is paired with"""
    guide = parser.add_mutually_exclusive_group()
    guide.add_argument('--guide-start-frame', type=int, default=0,
                       help=f'4K frame that matches {frame0_help} ({offset_help}; default 0)')
    guide.add_argument('--alignment-file', default=None,
                       help='alignment_data.json of the audio aligner: --guide-start-frame = '
                            'round(time_offset_seconds * fps of the 4K clip)')


def resolve_guide_start(args) -> bool:
    """--alignment-file -> args.guide_start_frame, announced; False, the error printed, when the file gives none (the CLI returns 1)"""
    if args.alignment_file is None:
        return True
    try:
        args.guide_start_frame = guide_start_frame_from(args.alignment_file, args.video_4k)
    except (OSError, ValueError, KeyError) as e:
        print(f"Error: {e}")
        return False
    print(f"Alignment file {args.alignment_file}: --guide-start-frame {args.guide_start_frame}")
    return True


def main(argv=None, backend=None):
    """Command line interface for fast audio-only alignment (+ optional frame matching on the GPU).  backend: a stand-in for
    the refinement's HipPipelineBackend (host-logic tests)."""
    parser = argparse.ArgumentParser(description='Fast audio-only video alignment (GPU FFT cross-correlation)')
    parser.add_argument('video1', help='Path to first video (reference)')
    parser.add_argument('video2', help='Path to second video (to be aligned)')
    parser.add_argument('--work-dir', default='temp_alignment', help='Working directory for temporary files')
    parser.add_argument('--max-audio', type=float, default=300.0, help='Maximum audio length for analysis (seconds)')
    parser.add_argument('--tolerance', type=float, default=2.0, help='Alignment tolerance in frame intervals')
    parser.add_argument('--min-correlation', type=float, default=0.6, help='Minimum correlation to proceed')
    from .framematch import add_refine_arguments, refine_options
    add_refine_arguments(parser)
    from .register import add_register_arguments
    add_register_arguments(parser)
    args = parser.parse_args(argv)
    from .depth import input_layout_options
    spatial = dict(start_frame=args.start_frame, probes=args.register_probes, unsqueeze=not args.no_unsqueeze,
                   max_frames=args.max_frames, min_score=args.register_min_score, bins=args.register_bins, **input_layout_options(args))
    try:
        aligner = VideoAligner(args.video1, args.video2, args.work_dir)
        if args.video_only:
            data = aligner.refine_video(aligner.video_only_data(), args.guide_start_frame, None, backend, **refine_options(args))
            if args.register_spatial:
                aligner.register_spatial(data, data['guide_start_frame'], backend, **spatial)
            print(f"\n✓ Video-only alignment: {data['visual_status']}, guide start frame {data['guide_start_frame']}")
            return 0
        alignment_data = aligner.find_alignment(args.max_audio)
        if args.refine_video:
            offset = alignment_data['time_offset_seconds']
            if offset < 0:
                raise ValueError(_negative_start_advice("--refine-video", f"{-offset:.3f}s",
                                                        int(round(-offset * float(alignment_data['video1_fps'])))))
            seed = int(round(offset * float(alignment_data['video2_fps'])))
            aligner.refine_video(alignment_data, seed, seed, backend, **refine_options(args))
        if args.register_spatial:
            g0 = alignment_data.get('guide_start_frame')
            if g0 is None:
                offset = alignment_data['time_offset_seconds']
                if offset < 0:
                    raise ValueError(_negative_start_advice("--register-spatial", f"{-offset:.3f}s",
                                                            int(round(-offset * float(alignment_data['video1_fps'])))))
                g0 = int(round(offset * float(alignment_data['video2_fps'])))
            aligner.register_spatial(alignment_data, int(g0), backend, **spatial)
        quality = aligner.assess_alignment_quality(alignment_data, args.tolerance)
        if alignment_data['correlation_strength'] < args.min_correlation:
            print(f"\nWarning: Correlation {alignment_data['correlation_strength']:.3f} below threshold {args.min_correlation}")
            try:
                response = input("Continue anyway? (y/n): ")
            except EOFError:                     # no terminal: "no"
                response = "n"
            if response.strip().lower() != 'y':
                return 1
        print("\n✓ Alignment complete! Use alignment_data.json in pipeline steps.")
        print(f"Quality: {quality}")
        print(f"Offset: {alignment_data['time_offset_seconds']:.3f}s")
        return 0
    except Exception as e:
        print(f"Error: {e}")
        return 1


if __name__ == "__main__":
    exit(main())
