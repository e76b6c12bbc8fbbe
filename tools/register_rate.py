"""Spatial registration: kernel time of v3d_plane_profiles_batch on 34 planes of 3840x2160 and of v3d_warp_u16_batch on 34 planes
of 1920x1080, each against its algorithmic bytes at the 8 TB/s HBM roofline, and the time of one search level's match call.
Prints one JSON line and, with --save, writes it to profiles/register_rate.json (--out: another path).

    python tools/register_rate.py [--save] [--out PATH]

Times: HIP events around `reps` back-to-back calls of the binding, inputs resident, warmed, best of 5 such groups, divided by
reps.  The binding allocates the outputs and the workspace per call from torch's caching allocator (no device allocation in the
steady state).  Algorithmic bytes: the profiles read 1 byte per pixel and write 4 (W + H) bytes per plane (the band partials in
the workspace are not counted); the warp reads the source once and writes 2 bytes per output pixel.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]

HBM = 8.0e12
Q = 65536


def _best_ms(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return min(ms), [round(m, 4) for m in ms]


def _entry(ms, groups, nbytes):
    return {"ms": round(ms, 4), "ms_groups": groups, "algorithmic_bytes": int(nbytes), "TBps": round(nbytes / (ms * 1e-3) / 1e12, 3),
            "fraction_of_hbm_roofline_8TBps": round(nbytes / (ms * 1e-3) / HBM, 4), "roofline_ms": round(nbytes / HBM * 1e3, 4)}


def kernel_times():
    import numpy as np
    import torch
    from video_3d_pipeline import _native as N, register as R
    out = {}
    gen = torch.Generator("cuda").manual_seed(1)
    n, H, W = 34, 2160, 3840
    gray = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    ms, groups = _best_ms(lambda: N.plane_profiles_batch(gray), 8)
    out["profiles_34x3840x2160"] = _entry(ms, groups, n * (H * W + 4 * (W + H)))
    one = gray[:1]
    ms, groups = _best_ms(lambda: N.plane_profiles_batch(one), 20)
    out["profiles_1x3840x2160"] = _entry(ms, groups, H * W + 4 * (W + H))
    col, row = N.plane_profiles_batch(gray[:3])
    del gray
    n, Hs, Ws = 34, 1080, 1920
    src = torch.randint(-32768, 32768, (n, Hs, Ws), dtype=torch.int16, device="cuda", generator=gen)
    dst = torch.empty((n, Hs, Ws), dtype=torch.int16, device="cuda")
    for name, amap in (("letterbox", (1.0, 0.0, 0.875, 0.0625)), ("identity", R.IDENTITY)):
        q = R.warp_q16(amap, (Ws, Hs), (2 * Ws, 2 * Hs))["q"]
        ms, groups = _best_ms(lambda: N.warp_u16_batch(src, *q, Ws, Hs, 0, dst), 8)
        out[f"warp_34x1920x1080_{name}"] = _entry(ms, groups, n * 2 * (round(amap[0] * amap[2] * Hs * Ws) + Hs * Ws))
    # one call of the match: the first search level of a 1920 -> 3840 axis (64 bins) and a refinement at 512 bins, three probes
    eye = col[:, ::2].contiguous()
    levels = R.search_levels(Ws, 2 * Ws, 512)
    _, cand0 = R.to_candidates(R.first_grid(Ws, 2 * Ws, levels[0][1]), 2 * Ws)
    _, cand2 = R.to_candidates(R.refine_grid((0, Ws * Q), levels[2][1], levels[2][2]), 2 * Ws)
    for name, cand, bins in (("match_first_level", cand0, levels[0][0]), ("match_last_level", cand2, levels[2][0])):
        c = torch.from_numpy(np.ascontiguousarray(cand)).cuda()
        ms, groups = _best_ms(lambda: N.profile_match_scores(eye, col, c, bins), 8)
        out[name] = {"frames": 3, "candidates": int(len(cand)), "bins": int(bins), "ms": round(ms, 4), "ms_groups": groups}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", action="store_true", help="also write profiles/register_rate.json")
    ap.add_argument("--out", default=None, help="write the line to this path")
    a = ap.parse_args()
    import torch
    line = json.dumps({"device": torch.cuda.get_device_name(0), "kernel": kernel_times()})
    print(line)
    for path in ([os.path.join(ROOT, "profiles", "register_rate.json")] if a.save else []) + ([a.out] if a.out else []):
        with open(path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
