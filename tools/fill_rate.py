"""Hole filling (--fill-holes) on one GPU, 1080p, a 34-frame pass: time per frame of v3d_fill_holes_disp16_batch (both launches)
from HIP events (3 warm-up, 20 timed launches), in place and out of place, on the matcher's own output and on a random 20 %
hole pattern; the share of 8 TB/s on its algorithmic 4 B/px (2 W H read + 2 W H written); and the device step of the one-pass
pipeline (sbs_to_disparity + u16 samples) with the flag off and on, alternating in this one process.  Prints one JSON line.

    python tools/fill_rate.py [--kernel-only]

Kernel times: rocprofv3 --kernel-trace --stats -- python tools/fill_rate.py --kernel-only, in a run of its own.
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


def matcher_output():
    from video_3d_pipeline import synthetic as syn
    m = N.StereoSGBM(W, H, NF)
    sbs = torch.stack([N.to_device(syn.sbs_frame(W, H, i % 4)) for i in range(NF)])
    lg, rg = N.sbs_to_gray_batch(sbs, True)
    disp = m.compute(lg, rg).clone()
    assert m.sync_errors() == 0
    m.close()
    return disp


def entry_rates(rounds=3):
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = torch.randint(0, 1024, (NF, H, W), generator=g, device="cuda", dtype=torch.int16)
    rnd[torch.rand((NF, H, W), generator=g, device="cuda") < 0.2] = -16
    rnd[:, :, :64] = -16
    bufs = {"matcher_output": matcher_output(), "random_20pct_holes": rnd}
    nbytes = 4 * W * H
    res = {"algorithmic_bytes_per_frame": nbytes, "floor_us_per_frame_at_8TBps": round(nbytes / HBM * 1e6, 3)}
    for name, src in bufs.items():
        ws = torch.empty(N.lib().v3d_fill_holes_ws_bytes(NF, H), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(src)
        work = src.clone()                                 # in place: idempotent, so every launch after the first sees a filled input
        oop, inp = [], []
        for _ in range(rounds):
            oop.append(timed(lambda: N.fill_holes_disp16_batch(src, out=out, ws=ws)) / NF)
            inp.append(timed(lambda: N.fill_holes_disp16_batch(work, out=work, ws=ws)) / NF)
        res[name] = {"holes_fraction": round(float((src < 0).float().mean()), 4),
                     "out_of_place_us_per_frame": [round(t, 3) for t in oop], "in_place_us_per_frame": [round(t, 3) for t in inp],
                     "out_of_place_median": round(float(np.median(oop)), 3), "in_place_median": round(float(np.median(inp)), 3),
                     "out_of_place_fraction_of_8TBps": round(nbytes / (float(np.median(oop)) * 1e-6) / HBM, 3)}
    return res


def pipeline_step(rounds=5):
    """sbs_to_disparity + the u16 samples of a 34-frame pass, flag off / on alternating; us per frame"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend
    be = HipPipelineBackend()
    frames = [syn.sbs_frame(W, H, i % 4) for i in range(NF)]
    off = lambda: be.depth_to_u16_batch(be.sbs_to_disparity(frames, True))
    on = lambda: be.depth_to_u16_batch(be.sbs_to_disparity(frames, True, fill_holes=True))
    off(), on()
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(timed(off, reps=2, warm=0) / NF)
        t_on.append(timed(on, reps=2, warm=0) / NF)
    return {"off_us_per_frame": [round(t, 1) for t in t_off], "on_us_per_frame": [round(t, 1) for t in t_on],
            "off_median": round(float(np.median(t_off)), 1), "on_median": round(float(np.median(t_on)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true", help="skip the pipeline step (profiler runs)")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "frames_per_pass": NF, "entry": entry_rates(1 if a.kernel_only else 3)}
    if not a.kernel_only:
        res["pipeline_step"] = pipeline_step()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
