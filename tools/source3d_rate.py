"""Source fill (v3d_render_stereo_source_batch) on one GPU: kernel time per 4K frame from HIP events (8 distinct frames per
launch, 3 warm-up and 20 timed launches), full SBS at the gains of --parallax source (the left eye untouched, the right eye moved
by the film's parallax at 2 4K pixels per matcher pixel).  The yardstick is v3d_render_stereo_packed_batch in the same run: it is
timed first, then the new entry at fill_eyes 0 and 2, and the three alternate for ROUNDS rounds so that a drift of the clock
shows as a spread and not as a difference.  The eye source is a 1920 x 1080 SBS frame per 4K frame (960 x 1080 stored eyes).
Prints one JSON line and writes it to profiles/source3d_rate.json.

    python tools/source3d_rate.py [--subpixel]
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
from video_3d_pipeline import convert  # noqa: E402
import envopts  # noqa: E402
from convert_rate import H, NF, REPS, W, inputs  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

WS, HS, ROUNDS = 1920, 1080, 3


def rates(subpixel):
    frames, depth = inputs(NF)
    f = torch.from_numpy(frames).cuda()
    d = torch.from_numpy(depth.view(np.int16)).cuda()
    sbs = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (NF, HS, WS, 3), dtype=np.uint8)).cuda()
    p = convert.source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": WS}, W)
    gains = N.stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    q = convert.fill_map_q16(None, (WS // 2, HS), (W, H))
    out = torch.empty((NF, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    calls = {
        "packed": lambda: N.render_stereo_packed_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, out, subpixel=subpixel),
        "source_fill0": lambda: N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 0, *q, out=out, subpixel=subpixel),
        "source_fill2": lambda: N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 2, *q, out=out, subpixel=subpixel),
    }
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, render in calls.items():
            for _ in range(3):
                render()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                render()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(round(e0.elapsed_time(e1) * 1e3 / (REPS * NF), 2))
    # the share of the right eye's targets that are holes, from the entry itself: a black source against a white frame
    white, black = torch.full_like(f[:1], 255), torch.zeros_like(sbs[:1])
    eye = N.render_stereo_source_batch(white, d[:1].contiguous(), *gains, N.STEREO_PACK_FULL_SBS, black, 2, *q, subpixel=subpixel)[0, :, W:]
    res = {name: {"us_per_frame": sorted(v)[len(v) // 2], "rounds": v} for name, v in us.items()}
    res["gains"] = list(gains)
    res["hole_share_frame0"] = round(float((eye == 0).all(dim=2).float().mean()), 4)
    res["fill0_over_packed"] = round(res["source_fill0"]["us_per_frame"] / res["packed"]["us_per_frame"], 3)
    res["fill2_over_packed"] = round(res["source_fill2"]["us_per_frame"] / res["packed"]["us_per_frame"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subpixel", action="store_true", help="also measure the sub-pixel renderer, after the integer one")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "source": f"{WS}x{HS}", "frames_per_launch": NF,
           "timed_launches": REPS, "integer": rates(False)}
    if a.subpixel:
        res["subpixel"] = rates(True)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "source3d_rate.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
