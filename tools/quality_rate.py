"""Quality report (--quality-report): time per call of v3d_quality_reproj_batch and v3d_quality_flicker_batch next to
v3d_bgr_to_gray on the same resident frames, and the file-to-file rate of the one-pass pipeline with and without the flag.  Prints
one JSON line and, with --save, writes it to profiles/quality_rate.json.

    python tools/quality_rate.py [--save] [--no-pipeline]

Kernel times: 8 and 34 resident 1920x1080 frames, HIP events around each of 20 calls after 3 warm-up calls; median, min and max in
microseconds.  Reprojection reads 4 bytes per pixel (two grays, the int16 disparity) plus a row-local gather, flicker 10 (two
float depths and two grays per pair); v3d_bgr_to_gray moves 4.  Bytes over the median time are given against the 8 TB/s HBM
roofline.  The disparity is the matcher's own on synthetic frames (repeated to fill the batch), so the gather sees real offsets.
Pipeline: a 1920x1080 synthetic SBS clip and its 3840x2160 guide clip as .npy stacks through `python -m
video_3d_pipeline.pipeline` in-process, stereo-only, alternating without / with the flag: frames per second of the whole run
(decode, kernels, zlib), so the spread between equal runs is visible next to the difference.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]

HBM = 8.0e12
W, H = 1920, 1080


def _times_us(fn, warm=3, timed=20):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(timed):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    us.sort()
    return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def kernel_times():
    import torch
    from video_3d_pipeline import _native as N, synthetic as syn
    base = N.to_device(np.stack([syn.sbs_frame(W, H, i) for i in range(4)]))
    lg4, rg4 = N.sbs_to_gray_batch(base, True)
    m = N.StereoSGBM(W, H, 4)
    disp4 = m.compute(lg4, rg4)
    assert m.sync_errors() == 0
    m.close()
    out = {}
    for n in (8, 34):
        idx = torch.arange(n, device="cuda") % 4
        lg, rg, disp = lg4[idx].contiguous(), rg4[idx].contiguous(), disp4[idx].contiguous()
        depth = N.disp_to_depth(disp)
        bgr = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        gray = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        ro = torch.empty((n, N.QUALITY_REPROJ_FIELDS), dtype=torch.int64, device="cuda")
        fo = torch.empty((n - 1, N.QUALITY_FLICKER_FIELDS), dtype=torch.int64, device="cuda")
        rws = torch.empty(N.lib().v3d_quality_reproj_ws_bytes(n, W, H), dtype=torch.uint8, device="cuda")
        fws = torch.empty(N.lib().v3d_quality_flicker_ws_bytes(n, W, H), dtype=torch.uint8, device="cuda")
        px = n * H * W
        r = _times_us(lambda: N.quality_reproj_batch(lg, rg, disp, 16, ro, rws))
        f = _times_us(lambda: N.quality_flicker_batch(depth, lg, 4, 16, fo, fws))
        g = _times_us(lambda: N.bgr_to_gray(bgr, gray))
        r["bytes"], f["bytes"], g["bytes"] = 4 * px, 10 * (n - 1) * H * W, 4 * px
        for t in (r, f, g):
            t["TBps"] = round(t["bytes"] / (t["median_us"] * 1e-6) / 1e12, 3)
            t["fraction_of_hbm_roofline_8TBps"] = round(t["bytes"] / (t["median_us"] * 1e-6) / HBM, 4)
        rec = ro[0].cpu().numpy().tolist()
        out[f"{n}x{W}x{H}"] = {"reproj": r, "flicker": f, "bgr_to_gray": g, "reproj_record_frame0": rec}
        del bgr, gray, lg, rg, disp, depth
    return out


def pipeline_rate(n_frames=24):
    """file-to-file frames per second of the one-pass pipeline without and with --quality-report, alternating (zlib-bound)"""
    from video_3d_pipeline import pipeline, synthetic as syn
    out = {}
    with tempfile.TemporaryDirectory() as d:
        base = [syn.sbs_frame(W, H, i) for i in range(4)]
        np.save(os.path.join(d, "sbs.npy"), np.stack([base[i % 4] for i in range(n_frames)]))
        g = [np.repeat(syn.guide_frame(W, H, i)[..., None], 3, axis=2) for i in range(4)]
        np.save(os.path.join(d, "g4k.npy"), np.stack([g[i % 4] for i in range(n_frames)]))
        del base, g
        for tag, extra in (("warm", []), ("plain", []), ("quality", ["--quality-report"]), ("plain_again", []), ("quality_again", ["--quality-report"])):
            t0 = time.perf_counter()
            rc = pipeline.main([os.path.join(d, "sbs.npy"), os.path.join(d, "g4k.npy"), "--output", os.path.join(d, f"{tag}.json"),
                                "--work-dir", os.path.join(d, f"w_{tag}"), "--stereo-only", *extra])
            dt = time.perf_counter() - t0
            assert rc == 0
            if tag != "warm":
                out[tag] = {"seconds": round(dt, 3), "frames_per_second": round(n_frames / dt, 2)}
            if extra:
                q = json.load(open(os.path.join(d, f"{tag}.json")))["quality"]
                out[tag]["reproj"] = {k: q["reproj"][k] for k in ("valid_share", "mean_abs_error", "mean_abs_error_d0", "bad_share")}
    out["frames"] = n_frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", action="store_true", help="also write profiles/quality_rate.json")
    ap.add_argument("--no-pipeline", action="store_true", help="kernel times only")
    a = ap.parse_args()
    import torch
    import envopts
    from video_3d_pipeline import _native as N
    envopts.select_variant_lib(N)           # V3D_HIP_LIB=path: an experiment build of the library (development only)
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_times()}
    if not a.no_pipeline:
        res["pipeline_1080p_to_4k"] = pipeline_rate()
    line = json.dumps(res)
    print(line)
    if a.save:
        with open(os.path.join(ROOT, "profiles", "quality_rate.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
