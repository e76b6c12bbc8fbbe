"""The matcher at two search windows on one GPU: v3d_sgbm_compute_batch on 34 resident 1920x1080 pairs with minDisparity 0 and
-32, one handle each, alternating in this one process; time per call from HIP events (3 warm-up, 10 timed calls, 5 rounds).  The
kernels are the same at every window -- k_cost reads its left records 32 columns further left, the L-R check + median places its
columns 32 further left -- so the expectation is equal time.  Prints one JSON line; --save writes profiles/mind_rate.json.

    python tools/mind_rate.py [--save]
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

W, H, NF, REPS, ROUNDS = 1920, 1080, 34, 10, 5
WINDOWS = (0, -32)


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
    return e0.elapsed_time(e1) / reps                  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", action="store_true", help="write profiles/mind_rate.json")
    a = ap.parse_args()
    from video_3d_pipeline import synthetic as syn
    sbs = torch.stack([N.to_device(syn.sbs_frame(W, H, i % 4)) for i in range(NF)])
    lg, rg = N.sbs_to_gray_batch(sbs, True)
    del sbs
    out = torch.empty((NF, H, W), dtype=torch.int16, device="cuda")
    handles = {m: N.StereoSGBM(W, H, NF, minDisparity=m) for m in WINDOWS}
    ms = {m: [] for m in WINDOWS}
    valid = {}
    for _ in range(ROUNDS):
        for m, h in handles.items():
            ms[m].append(timed(lambda: h.compute(lg, rg, out)))
            valid[m] = round(float((out != 16 * (m - 1)).float().mean()), 4)
    for m, h in handles.items():
        assert h.sync_errors() == 0, f"m={m}: lock-step time-outs"
        h.close()
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "frames_per_call": NF, "timed_calls_per_round": REPS}
    for m in WINDOWS:
        med = float(np.median(ms[m]))
        res[f"m={m}"] = {"ms_per_call": [round(t, 3) for t in ms[m]], "median_ms_per_call": round(med, 3),
                         "frames_per_s": round(NF / med * 1e3, 1), "valid_share": valid[m]}
    res["ratio_m-32_over_m0"] = round(res["m=-32"]["median_ms_per_call"] / res["m=0"]["median_ms_per_call"], 4)
    line = json.dumps(res)
    print(line)
    if a.save:
        with open(os.path.join(ROOT, "profiles", "mind_rate.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
