"""Frame matching (--check-guide, --refine-video): kernel time of v3d_frame_signature_batch against v3d_bgr_to_gray on the same
frames, v3d_signature_scores, and the file-to-file pipeline rate with and without --check-guide.  Prints one JSON line and, with
--save, writes it to profiles/framematch_rate.json.

    python tools/framematch_rate.py [--save] [--no-pipeline]

Kernel times: HIP events around `reps` back-to-back launches, warmed, best of 5 such groups, divided by reps: 8 and 34 resident
3840x2160 luma planes and 34 planes of 1920x1080.  The signature reads 1 byte per pixel and writes 4.6 KB per frame;
v3d_bgr_to_gray reads 3 bytes and writes 1 per pixel, so the signature must not take longer.  Bytes over time are given against
the 8 TB/s HBM roofline.  Pipeline: a 1920x1080 synthetic SBS clip and its 3840x2160 guide clip as .npy stacks through
`python -m video_3d_pipeline.pipeline` in-process, stereo-only, frames per second of the whole run (decode, kernels, zlib).
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


def kernel_times():
    import torch
    from video_3d_pipeline import _native as N
    out = {}
    gen = torch.Generator("cuda").manual_seed(1)
    for name, n, H, W in (("8x3840x2160", 8, 2160, 3840), ("34x3840x2160", 34, 2160, 3840), ("34x1920x1080", 34, 1080, 1920)):
        bgr = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=gen)
        gray = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        sig = torch.empty((n, N.SIG_CELLS), dtype=torch.int16, device="cuda")
        reps = 20 if n == 8 else 8
        g_ms, g_all = _best_ms(lambda: N.bgr_to_gray(bgr, gray), reps)
        s_ms, s_all = _best_ms(lambda: N.frame_signature_batch(gray, sig), reps)
        px = n * H * W
        out[name] = {
            "signature_us_per_frame": round(s_ms * 1e3 / n, 3), "bgr_to_gray_us_per_frame": round(g_ms * 1e3 / n, 3),
            "signature_ms": round(s_ms, 4), "bgr_to_gray_ms": round(g_ms, 4), "signature_ms_groups": s_all, "bgr_to_gray_ms_groups": g_all,
            "signature_TBps": round((px + n * N.SIG_CELLS * 2) / (s_ms * 1e-3) / 1e12, 3), "bgr_to_gray_TBps": round(4 * px / (g_ms * 1e-3) / 1e12, 3),
            "signature_fraction_of_hbm_roofline_8TBps": round((px + n * N.SIG_CELLS * 2) / (s_ms * 1e-3) / HBM, 4),
            "signature_not_slower_than_bgr_to_gray": bool(s_ms <= g_ms)}
        del bgr, gray
    a = torch.randint(0, 32768, (24, N.SIG_CELLS), dtype=torch.int16, device="cuda", generator=gen)
    b = torch.randint(0, 32768, (32, N.SIG_CELLS), dtype=torch.int16, device="cuda", generator=gen)
    ms, _ = _best_ms(lambda: N.signature_scores(a, b), 20)
    out["scores_24x32_us"] = round(ms * 1e3, 2)
    a8 = a[:8].contiguous()
    ms, _ = _best_ms(lambda: N.signature_scores(a8, a8), 20)
    out["scores_8x8_us"] = round(ms * 1e3, 2)
    return out


def pipeline_rate(n_frames=24):
    """file-to-file frames per second of the one-pass pipeline with and without --check-guide (zlib-bound: no threshold)"""
    from video_3d_pipeline import pipeline, synthetic as syn
    W, H = 1920, 1080
    out = {}
    with tempfile.TemporaryDirectory() as d:
        base = [syn.sbs_frame(W, H, i) for i in range(4)]
        np.save(os.path.join(d, "sbs.npy"), np.stack([base[i % 4] for i in range(n_frames)]))
        g = [np.repeat(syn.guide_frame(W, H, i)[..., None], 3, axis=2) for i in range(4)]
        np.save(os.path.join(d, "g4k.npy"), np.stack([g[i % 4] for i in range(n_frames)]))
        del base, g
        for tag, extra in (("warm", []), ("plain", []), ("check_guide", ["--check-guide"]), ("plain_again", []), ("check_guide_again", ["--check-guide"])):
            t0 = time.perf_counter()
            rc = pipeline.main([os.path.join(d, "sbs.npy"), os.path.join(d, "g4k.npy"), "--output", os.path.join(d, f"{tag}.json"),
                                "--work-dir", os.path.join(d, f"w_{tag}"), "--stereo-only", *extra])
            dt = time.perf_counter() - t0
            assert rc == 0
            if tag != "warm":
                out[tag] = {"seconds": round(dt, 3), "frames_per_second": round(n_frames / dt, 2)}
            if extra:
                out[tag]["guide_match"] = json.load(open(os.path.join(d, f"{tag}.json")))["guide_match"]
    out["frames"] = n_frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", action="store_true", help="also write profiles/framematch_rate.json")
    ap.add_argument("--no-pipeline", action="store_true", help="kernel times only")
    a = ap.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "kernel": kernel_times()}
    if not a.no_pipeline:
        res["pipeline_1080p_to_4k"] = pipeline_rate()
    line = json.dumps(res)
    print(line)
    if a.save:
        with open(os.path.join(ROOT, "profiles", "framematch_rate.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
