"""Temporal stabilisation stage on one GPU, 1080p, a 34-frame pass in steady state (2R carried frames + 34 new ones, 34 targets):
time per frame of the filter kernel alone and of the whole stage (concat of the carry, cuts, min/max, range, filter,
normalisation) from HIP events (warm-up, 20 timed launches), the filter's share of 8 TB/s on its algorithmic 9 B/px, and the
device step of the one-pass pipeline (sbs_to_disparity + u16 samples) with the stage on and off, alternating in this one
process.  Prints one JSON line.

--range-percentile P adds the robust range (v3d_depth_robust_minmax_batch) against v3d_depth_minmax_batch on the same 34-frame
buffers (the synthetic clip, the matcher's output on the synthetic SBS frames, a constant frame: the worst case for same-address
LDS atomics), alternating, and the stage at R = 2 and the radius-0 u16 step with and without the option.

--motion S [S ...] adds the motion-compensated window (--temporal-motion): the stage at R = 2 on one panning 34-frame pass with
the option off (v3d_temporal_cuts + v3d_temporal_filter_batch: what the stage always was) and on at each S, alternating, and
v3d_temporal_motion and v3d_temporal_filter_mc_batch alone, the filter with the clip's own cuts and with an all-zero cut array (full
windows: on a pan the search may leave cuts that shorten them).

    python tools/temporal_rate.py [--kernel-only] [--radius 2 4] [--range-percentile 98] [--motion 8 16 32 [--motion-only]]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]
from video_3d_pipeline import _native as N  # noqa: E402
import envopts  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

W, H, NF, REPS, HBM = 1920, 1080, 34, 20, 8.0e12


def clip(T, seed=0):
    """static scene + per-frame noise: disparity with sub-pixel jitter and 5 % invalid pixels, luma with sigma-3 noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.linspace(4, 60, W, device="cuda")[None, None, :].expand(T, H, W)
    d16 = torch.round((x + 0.1 * torch.randn((T, H, W), generator=g, device="cuda")) * 16)
    d16[torch.rand((T, H, W), generator=g, device="cuda") < 0.05] = 0
    base = torch.randint(0, 256, (1, H, W), generator=g, device="cuda").float()
    gray = (base + 3 * torch.randn((T, H, W), generator=g, device="cuda")).clamp(0, 255).round().to(torch.uint8)
    return (d16 / 16).float().contiguous(), gray.contiguous()


def timed(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps            # us per call


def stage_rates(radii):
    from video_3d_pipeline.depth import HipStereoBackend
    be = HipStereoBackend()
    res = {}
    for R in radii:
        T = NF + 2 * R
        depth, gray = clip(T, R)
        cut = N.temporal_cuts(gray, 20)
        out = torch.empty((NF, H, W), dtype=torch.float32, device="cuda")
        us_f = timed(lambda: N.temporal_filter_batch(depth, gray, R, 12, cut, True, R, NF, out)) / NF
        carry_d, carry_g, new_d, new_g = depth[:2 * R], gray[:2 * R], depth[2 * R:], gray[2 * R:]

        def stage():
            d, g = be.temporal_concat(carry_d, new_d), be.temporal_concat(carry_g, new_g)
            return be.temporal_stabilize(d, g, R, NF, R, 12, 20, True)

        us_s = timed(stage) / NF
        nbytes = W * H * 9
        res[f"R{R}"] = {"filter_us_per_frame": round(us_f, 2), "stage_us_per_frame": round(us_s, 2),
                        "filter_algorithmic_bytes_per_frame": nbytes,
                        "filter_fraction_of_8TBps": round(nbytes / (us_f * 1e-6) / HBM, 3),
                        "filter_bytes_read_per_frame_walking_the_window": W * H * (5 * (2 * R + 1) + 4)}
    return res


def pipeline_step(R=2, rounds=5):
    """sbs_to_disparity + the u16 samples of a 34-frame pass, stage off / on alternating; us per frame"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend
    be = HipPipelineBackend()
    frames = [syn.sbs_frame(W, H, i % 4) for i in range(NF)]
    state = {}

    def off():
        return be.depth_to_u16_batch(be.sbs_to_disparity(frames, True))

    def on():
        depth = be.sbs_to_disparity(frames, True)
        gray = be.left_gray(NF)
        if "d" in state:
            depth, gray = be.temporal_concat(state["d"], depth), be.temporal_concat(state["g"], gray)
        else:
            depth, gray = depth.clone(), gray.clone()
        t0 = len(depth) - NF - R if len(depth) > NF else 0
        out = be.temporal_stabilize(depth, gray, max(t0, 0), NF if len(depth) > NF else NF - R, R, 12, 20, True)
        state["d"], state["g"] = depth[-2 * R:], gray[-2 * R:]
        return out

    off(), on(), on()
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(timed(off, reps=2, warm=0) / NF)
        t_on.append(timed(on, reps=2, warm=0) / NF)
    return {"radius": R, "off_us_per_frame": [round(t, 1) for t in t_off], "on_us_per_frame": [round(t, 1) for t in t_on],
            "off_median": round(float(np.median(t_off)), 1), "on_median": round(float(np.median(t_on)), 1)}


def range_rates(percentile, R=2, rounds=3, entry_only=False):
    """us per 34-frame call, max entry / robust entry alternating; floor: one 4 B/px read of the buffer at 8 TB/s"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend
    from video_3d_pipeline.temporal import check_range_percentile
    q = check_range_percentile(percentile)
    be = HipPipelineBackend()
    depth, gray = clip(NF + 2 * R, 1)
    matched = be.sbs_to_disparity([syn.sbs_frame(W, H, i % 4) for i in range(NF)], True).clone()
    bufs = {"synthetic_clip": depth[:NF], "matcher_output": matched, "constant_frame": torch.full_like(matched, 7.25)}
    floor_us = NF * W * H * 4 / HBM * 1e6
    res = {"q": q, "floor_us_one_read_at_8TBps": round(floor_us, 1), "entry_us_per_call": {}}
    for name, buf in bufs.items():
        mx, rb = [], []
        for _ in range(rounds):
            mx.append(timed(lambda: N.depth_minmax_batch(buf)))
            rb.append(timed(lambda: N.depth_robust_minmax_batch(buf, q)))
        res["entry_us_per_call"][name] = {"minmax": [round(t, 1) for t in mx], "robust": [round(t, 1) for t in rb],
                                          "minmax_median": round(float(np.median(mx)), 1), "robust_median": round(float(np.median(rb)), 1),
                                          "robust_times_floor": round(float(np.median(rb)) / floor_us, 2),
                                          "minmax_times_floor": round(float(np.median(mx)) / floor_us, 2)}
    if entry_only:
        return res
    off, on, off0, on0 = [], [], [], []
    for _ in range(rounds):
        off.append(timed(lambda: be.temporal_stabilize(depth, gray, R, NF, R, 12, 20, True)) / NF)
        on.append(timed(lambda: be.temporal_stabilize(depth, gray, R, NF, R, 12, 20, True, q)) / NF)
        off0.append(timed(lambda: be.depth_to_u16_batch(matched)) / NF)
        on0.append(timed(lambda: be.depth_to_u16_robust(matched, q)) / NF)
    res["stage_R2_us_per_frame"] = {"max": round(float(np.median(off)), 2), "robust": round(float(np.median(on)), 2)}
    res["u16_step_R0_us_per_frame"] = {"max": round(float(np.median(off0)), 2), "robust": round(float(np.median(on0)), 2)}
    return res


def pan_clip(T, pan=5, seed=0):
    """clip()'s disparity over a texture that pans by `pan` pixels per frame, sigma-3 noise"""
    depth, _ = clip(T, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 100)
    base = torch.randint(0, 256, (H, W + pan * T), generator=g, device="cuda").float()
    base = (base + base.roll(1, 0) + base.roll(1, 1) + base.roll((1, 1), (0, 1))) / 4
    gray = torch.stack([base[:, pan * t:pan * t + W] for t in range(T)])
    gray = (gray + 3 * torch.randn((T, H, W), generator=g, device="cuda")).clamp(0, 255).round().to(torch.uint8)
    return depth, gray.contiguous()


def motion_rates(searches, R=2, rounds=3):
    """us per frame of a 34-frame pass (34 targets, 2R carried frames): stage off / on alternating, then the two new entries alone"""
    from video_3d_pipeline.depth import HipStereoBackend
    be = HipStereoBackend()
    T = NF + 2 * R
    depth, gray = pan_clip(T)
    out = torch.empty((NF, H, W), dtype=torch.float32, device="cuda")
    res = {"radius": R, "pan_px_per_frame": 5, "uncompensated_cuts": int(N.temporal_cuts(gray, 20).sum())}
    for S in searches:
        off, on, search, filt, full = [], [], [], [], []
        fwd, bwd, resid, cut = N.temporal_motion(gray, S, 20)
        nocut = torch.zeros_like(cut)
        for _ in range(rounds):
            off.append(timed(lambda: be.temporal_stabilize(depth, gray, R, NF, R, 12, 20, True)) / NF)
            on.append(timed(lambda: be.temporal_stabilize(depth, gray, R, NF, R, 12, 20, True, motion_search=S)) / NF)
            search.append(timed(lambda: N.temporal_motion(gray, S, 20)) / NF)
            filt.append(timed(lambda: N.temporal_filter_mc_batch(depth, gray, R, 12, cut, fwd, bwd, True, R, NF, out)) / NF)
            full.append(timed(lambda: N.temporal_filter_mc_batch(depth, gray, R, 12, nocut, fwd, bwd, True, R, NF, out)) / NF)
        res[f"S{S}"] = {"stage_off_us_per_frame": [round(t, 2) for t in off], "stage_on_us_per_frame": [round(t, 2) for t in on],
                        "stage_off_median": round(float(np.median(off)), 2), "stage_on_median": round(float(np.median(on)), 2),
                        "motion_entry_us_per_frame": round(float(np.median(search)), 2),
                        "filter_mc_us_per_frame": round(float(np.median(filt)), 2), "compensated_cuts": int(cut.sum()),
                        "filter_mc_full_windows_us_per_frame": round(float(np.median(full)), 2),
                        "sad_lane_ops_per_frame": 2 * (2 * S + 1) ** 2 * W * H // 4}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--kernel-only", action="store_true", help="skip the pipeline step (profiler runs)")
    ap.add_argument("--range-percentile", type=float, default=None, help="also time the robust range at this percentile")
    ap.add_argument("--range-only", action="store_true", help="with --range-percentile: only the two min/max entries (profiler, A/B runs)")
    ap.add_argument("--motion", type=int, nargs="+", default=None, help="also time the motion-compensated window at these search radii")
    ap.add_argument("--motion-only", action="store_true", help="with --motion: only that leg")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "frames_per_pass": NF}
    if a.motion is not None:
        res["motion"] = motion_rates(a.motion)
        if a.motion_only:
            print(json.dumps(res))
            return
    if a.range_percentile is not None:
        res["robust_range"] = range_rates(a.range_percentile, entry_only=a.range_only)
    if not a.range_only:
        res["stage"] = stage_rates(a.radius)
    if not a.kernel_only and not a.range_only:
        res["pipeline_step"] = pipeline_step()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
