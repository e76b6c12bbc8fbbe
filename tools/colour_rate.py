"""Colour matching (v3d_bgr_hist_batch, v3d_colour_lut_batch, v3d_bgr_lut_batch) on one GPU: kernel time per frame from HIP events
(resident buffers, 8 distinct frames per launch, 3 warm-up and 20 timed launches), the calls of a group alternating for ROUNDS
rounds so that a drift of the clock shows as a spread and not as a difference; the median round is reported.

  histogram   a 3840 x 2160 frame and the 960 x 1080 stored left eye of a 1920 x 1080 SBS frame, on a noisy, a real-looking
              (synthetic.stereo_pair, enlarged) and a constant frame: microseconds per frame and the share of the 8 TB/s roofline on
              the algorithmic bytes 3 W H; beside it k_rr_hist (v3d_depth_robust_minmax_batch on 8 float frames of 3840 x 2160) per
              input byte in the same run, the project's existing histogram as the yardstick.  --ab-lib PATH times the same entry
              of a second build of the library in the same rounds (an experiment build: the A/B of DESIGN.md, "Colour matching")
  frame mode  its whole addition per frame (the eye's and the frame's histogram, the tables, the apply on the right eye) beside
              v3d_render_stereo_source_batch with fill_eyes = 2
  clip mode   its addition per batch: the apply alone
Prints one JSON line and writes it to profiles/colour_match_rate.json.

    python tools/colour_rate.py [--ab-lib build/libv3d_variant.so]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]
from video_3d_pipeline import _native as N  # noqa: E402
from video_3d_pipeline import convert  # noqa: E402
from video_3d_pipeline import synthetic  # noqa: E402
import envopts  # noqa: E402
from convert_rate import H, HBM, NF, REPS, W, inputs  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

WS, HS, ROUNDS = 1920, 1080, 3


def timed(calls, per):
    """{name: call} -> {name: {us: the median round's microseconds per `per` units, rounds}}"""
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                call()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(round(e0.elapsed_time(e1) * 1e3 / (REPS * per), 2))
    return {name: {"us": sorted(v)[len(v) // 2], "rounds": v} for name, v in us.items()}


def contents(w, h):
    """8 distinct frames of each kind, u8 [8,h,w,3] on the device"""
    rng = np.random.default_rng(3)
    small = synthetic.stereo_pair(480, 270, 0)[0]
    real = np.repeat(np.repeat(small, -(-h // 270), axis=0), -(-w // 480), axis=1)[:h, :w]
    kinds = {"noise": rng.integers(0, 256, (NF, h, w, 3), dtype=np.uint8),
             "synthetic": np.stack([np.roll(real, 17 * i, axis=1) for i in range(NF)]),
             "constant": np.stack([np.full((h, w, 3), 40 + 20 * i, np.uint8) for i in range(NF)])}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in kinds.items()}


def raw_hist(lib, t, rect, out):
    """v3d_bgr_hist_batch of another build of the library, on the same tensors"""
    n, h, w, _ = t.shape
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.v3d_bgr_hist_batch(C.c_void_p(t.data_ptr()), C.c_size_t(t.stride(0)), n, w, h, t.stride(1), *rect, C.c_void_p(out.data_ptr()), st)
    assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab-lib", default=None, help="a second build of libv3d_hip.so whose histogram entry is timed beside the in-tree one")
    a = ap.parse_args()
    other = C.CDLL(os.path.abspath(a.ab_lib)) if a.ab_lib else None
    res = {"device": torch.cuda.get_device_name(0), "frames_per_launch": NF, "timed_launches": REPS, "rounds": ROUNDS}

    # 1. the histogram, beside k_rr_hist
    depth = torch.from_numpy(inputs(NF)[1].astype(np.float32) / 1024).cuda()            # [8,2160,3840]: 0 .. 64, smooth
    hist = {}
    for label, (w, h, rect) in {"3840x2160": (W, H, (0, 0, W, H)), "eye960x1080": (WS, HS, (0, 0, WS // 2, HS))}.items():
        out = torch.empty((NF, 3, 256), dtype=torch.int32, device="cuda")
        calls = {"k_rr_hist": lambda: N.depth_robust_minmax_batch(depth, 9900)}
        frames = contents(w, h)
        for kind, t in frames.items():
            calls[kind] = lambda t=t: N.bgr_hist_batch(t, rect, out=out)
            if other is not None:
                calls[kind + "_ab"] = lambda t=t: raw_hist(other, t, rect, out)
                raw_hist(other, t, rect, out)
                assert torch.equal(out, N.bgr_hist_batch(t, rect)), "the two builds disagree"
        r = timed(calls, NF)
        nbytes = 3 * (rect[2] - rect[0]) * (rect[3] - rect[1])
        for k, v in r.items():
            b = H * W * 4 if k == "k_rr_hist" else nbytes
            v["ns_per_kilobyte"] = round(v["us"] * 1e3 / (b / 1024), 3)
            v["roofline_share"] = round(b / HBM / (v["us"] * 1e-6), 4)
        hist[label] = r
    res["histogram"] = hist

    # 2. and 3. what the two modes add to a batch, beside the render they precede
    frames, d16 = inputs(NF)
    f = torch.from_numpy(frames).cuda()
    d = torch.from_numpy(d16.view(np.int16)).cuda()
    sbs = contents(WS, HS)["noise"]
    p = convert.source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": WS}, W)
    gains = N.stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    q = convert.fill_map_q16(None, (WS // 2, HS), (W, H))
    out = torch.empty((NF, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    eye, right = (0, 0, WS // 2, HS), (WS // 2, 0, WS, HS)
    hs, hd = torch.empty((NF, 3, 256), dtype=torch.int32, device="cuda"), torch.empty((NF, 3, 256), dtype=torch.int32, device="cuda")
    tables = torch.empty((NF, 3, 256), dtype=torch.uint8, device="cuda")
    one = N.colour_lut_batch(N.bgr_hist_batch(sbs, eye), N.bgr_hist_batch(f), NF)

    def frame_mode():
        N.colour_lut_batch(N.bgr_hist_batch(sbs, eye, out=hs), N.bgr_hist_batch(f, out=hd), 1, out=tables)
        N.bgr_lut_batch(sbs, tables, right, out=sbs)

    r = timed({"render_source_fill2": lambda: N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 2, *q, out=out),
               "frame_mode_addition": frame_mode,
               "clip_mode_addition": lambda: N.bgr_lut_batch(sbs, one, right, out=sbs),
               "table_alone": lambda: N.colour_lut_batch(hs, hd, 1, out=tables)}, NF)
    r["frame_over_render"] = round(r["frame_mode_addition"]["us"] / r["render_source_fill2"]["us"], 3)
    r["clip_over_render"] = round(r["clip_mode_addition"]["us"] / r["render_source_fill2"]["us"], 3)
    res["per_frame"] = r
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "colour_match_rate.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
