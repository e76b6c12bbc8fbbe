"""DIBR step (v3d_render_stereo_batch) on one GPU: kernel time per 4K frame from HIP events (8 distinct frames per launch,
warm-up, 20 timed launches, both layouts), the algorithmic bytes and their share of 8 TB/s, and the convert CLI's end-to-end
frames/s on a synthetic .npy 4K clip.  Prints one JSON line.  --subpixel measures v3d_render_stereo_subpixel_batch the same way
after the integer entry (the yardstick, same process and inputs) and adds "kernel_subpixel" and the ratio of the two.  --packings
adds the packings of v3d_render_stereo_packed_batch (top-bottom, row-interleaved, anaglyph) to each of those tables.

    python tools/convert_rate.py [--frames 24] [--kernel-only] [--subpixel] [--packings]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]
from video_3d_pipeline import _native as N  # noqa: E402
import envopts  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

W, H, NF, REPS, HBM = 3840, 2160, 8, 20, 8.0e12


def inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    x = np.arange(W)[None, :]
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.empty((n, H, W), np.uint16)
    for i in range(n):
        d = rng.integers(0, 65536) + x * int(rng.integers(-12, 12)) + (np.arange(H)[:, None] * int(rng.integers(-20, 20)))
        d[H // 4:H // 2, W // 3:W // 2] = rng.integers(0, 65536)
        depth[i] = np.clip(d, 0, 65535)
    return frames, depth


# name, packing code, output bytes per source pixel; codes >= 2 are v3d_render_stereo_packed_batch (--packings)
SBS = (("full_sbs", N.STEREO_FULL_SBS, 6), ("half_sbs", N.STEREO_HALF_SBS, 3))
PACKED = (("full_tb", N.STEREO_PACK_FULL_TB, 6), ("half_tb", N.STEREO_PACK_HALF_TB, 3), ("interlaced", N.STEREO_PACK_ROWS, 3),
          ("anaglyph_colour", N.STEREO_PACK_ANAGLYPH_COLOUR, 3), ("anaglyph_dubois", N.STEREO_PACK_ANAGLYPH_DUBOIS, 3))


def kernel_rates(subpixel=False, layouts=SBS):
    frames, depth = inputs(NF)
    f = torch.from_numpy(frames).cuda()
    d = torch.from_numpy(depth.view(np.int16)).cuda()
    gl, gr, conv = N.stereo_gains()
    res = {}
    for name, layout, out_px in layouts:
        oW, oH = N.stereo_output_size(layout, W, H)
        out = torch.empty((NF, oH, oW, 3), dtype=torch.uint8, device="cuda")
        if layout >= 2:
            render = lambda: N.render_stereo_packed_batch(f, d, gl, gr, conv, layout, out, subpixel=subpixel)
        else:
            render = lambda: N.render_stereo_batch(f, d, gl, gr, conv, layout, out, subpixel=subpixel)
        for _ in range(3):
            render()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            render()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / (REPS * NF)
        nbytes = W * H * (2 + 3 + out_px)
        res[name] = {"us_per_frame": round(us, 2), "algorithmic_bytes_per_frame": nbytes,
                     "fraction_of_8TBps": round(nbytes / (us * 1e-6) / HBM, 3)}
    return res


def cli_rate(n, encoders=("zlib",), subpixel=False):
    from video_3d_pipeline import convert, utils
    frames, depth = inputs(n, seed=1)
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "v4k.npy"), frames)
        ddir = os.path.join(tmp, "d_frames")
        os.makedirs(ddir)
        for i in range(n):
            utils.write_png16(os.path.join(ddir, f"depth4k_{i:06d}.png"), depth[i])
        del frames, depth
        res = {}
        for enc in encoders:                                   # alternating in this one process
            conv = convert.DepthTo3DConverter(png_encoder=enc, subpixel=subpixel)
            conv.process_conversion(os.path.join(tmp, "v4k.npy"), ddir, os.path.join(tmp, f"warm_{enc}.json"), max_frames=2)
            t0 = time.perf_counter()
            conv.process_conversion(os.path.join(tmp, "v4k.npy"), ddir, os.path.join(tmp, f"out_{enc}.json"))
            dt = time.perf_counter() - t0
            res.setdefault(enc, []).append({"frames": n, "seconds": round(dt, 2), "frames_per_s": round(n / dt, 2)})
    return res["zlib"][0] if list(encoders) == ["zlib"] else res       # an encoder listed twice is run twice: the spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24, help="frames of the synthetic clip the CLI converts")
    ap.add_argument("--kernel-only", action="store_true", help="skip the end-to-end CLI run (profiler runs)")
    ap.add_argument("--png-encoder", nargs="+", choices=["zlib", "gpu"], default=["zlib"],
                    help="the CLI run once per listed encoder, alternating in this one process")
    ap.add_argument("--subpixel", action="store_true", help="also measure the sub-pixel entry, after the integer one; the CLI run uses it")
    ap.add_argument("--packings", action="store_true",
                    help="also measure the top-bottom, row-interleaved and anaglyph packings, after the two side-by-side layouts")
    a = ap.parse_args()
    layouts = SBS + PACKED if a.packings else SBS
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "kernel": kernel_rates(layouts=layouts)}
    if a.subpixel:
        res["kernel_subpixel"] = kernel_rates(subpixel=True, layouts=layouts)
        res["subpixel_over_integer"] = {k: round(res["kernel_subpixel"][k]["us_per_frame"] / res["kernel"][k]["us_per_frame"], 3)
                                        for k in res["kernel"]}
    if not a.kernel_only:
        res["convert_cli_full_sbs"] = cli_rate(a.frames, a.png_encoder, a.subpixel)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
