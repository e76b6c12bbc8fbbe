"""The two gray splits on one GPU, and the depth CLI on a clip of either layout.

    python tools/split_tb_rate.py kernels        v3d_tb_to_gray_batch and v3d_sbs_to_gray_batch, unsqueeze = 1, on 34 resident
                                                 1920x1080 frames (random bytes: both read and write the same number of bytes),
                                                 alternating, 3 warm-up and 40 timed calls each.  Meant to run under
                                                 `rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python ...`
    python tools/split_tb_rate.py stats TRACE    the kernel trace CSV of that run -> per-kernel median, quartiles, min and max of
                                                 the timed dispatches, the ratio of the medians, algorithmic bytes and HBM share
    python tools/split_tb_rate.py cli            the depth CLI's frames/s on a synthetic top-bottom clip and on the side-by-side
                                                 clip of the same size, raw sink (no zlib), batch 34, alternating, 3 rounds
Each mode prints one JSON line; --save FILE merges it into that JSON file under the mode's name."""
import argparse
import contextlib
import csv
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]

W, H, NF, WARM, CALLS = 1920, 1080, 34, 3, 40
HBM_PEAK_TBS = 8.0
KERNELS = {"tb": "k_split_tb<true>", "sbs": "k_split_sbs<true>"}


def kernels():
    import torch
    from video_3d_pipeline import _native as N
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (NF, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    out = (torch.empty((NF, H, W), dtype=torch.uint8, device="cuda"), torch.empty((NF, H, W), dtype=torch.uint8, device="cuda"))
    for _ in range(WARM + CALLS):
        N.tb_to_gray_batch(frames, True, out)
        N.sbs_to_gray_batch(frames, True, out)
    torch.cuda.synchronize()
    return {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "frames_per_call": NF, "calls": WARM + CALLS}


def stats(trace):
    us = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(trace)):
        for k, name in KERNELS.items():
            if name in row["Kernel_Name"]:
                us[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    read, written = NF * H * W * 3, 2 * NF * H * W                  # one read of every frame byte, one write of every gray byte
    res = {"size": f"{W}x{H}", "frames_per_call": NF, "algorithmic_bytes": read + written, "hbm_peak_TB_per_s": HBM_PEAK_TBS}
    for k, v in us.items():
        assert len(v) == WARM + CALLS, f"{KERNELS[k]}: {len(v)} dispatches in the trace"
        t = np.array(v[WARM:])
        med = float(np.median(t))
        res[k] = {"kernel": KERNELS[k], "timed_dispatches": len(t), "median_us": round(med, 2), "q1_us": round(float(np.percentile(t, 25)), 2),
                  "q3_us": round(float(np.percentile(t, 75)), 2), "min_us": round(float(t.min()), 2), "max_us": round(float(t.max()), 2),
                  "TB_per_s": round((read + written) / med / 1e6, 3), "hbm_share": round((read + written) / med / 1e6 / HBM_PEAK_TBS, 4)}
    res["ratio_tb_over_sbs"] = round(res["tb"]["median_us"] / res["sbs"]["median_us"], 4)
    return res


class RawSink:
    """stands where utils.PngWriterPool stands: raw little-endian samples, written synchronously"""

    def submit(self, path, img_u16):
        np.ascontiguousarray(img_u16).tofile(str(path) + ".raw")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def cli(frames=102, rounds=3):
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = tempfile.mkdtemp(prefix="split_tb_rate_")
    try:
        clips = {}
        for layout, make in (("sbs", syn.sbs_frame), ("tb", syn.tb_frame)):
            base = [make(W, H, i) for i in range(4)]
            clips[layout] = os.path.join(work, f"{layout}.npy")
            np.save(clips[layout], np.stack([base[i % 4] for i in range(frames)]))
        fps = {k: [] for k in clips}
        with contextlib.redirect_stdout(io.StringIO()):
            ex = {k: HybridStereoDepthExtractor(work_dir=work, cache_dir=work, stereo_only=True, batch_size=NF,
                                                **({"input_layout": k} if k != "sbs" else {})) for k in clips}
            for e in ex.values():
                e.writer_pool_factory = RawSink
            for r in range(rounds + 1):                              # round 0 warms up (library load, workspace, pinned blocks)
                for k, e in ex.items():
                    t0 = time.perf_counter()
                    e.process_video_sbs(clips[k], force_reprocess=True)
                    if r:
                        fps[k].append(frames / (time.perf_counter() - t0))
        res = {"size": f"{W}x{H}", "frames": frames, "batch": NF, "sink": "raw"}
        for k, v in fps.items():
            res[k] = {"frames_per_s": [round(x, 1) for x in v], "median_frames_per_s": round(float(np.median(v)), 1)}
        return res
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "stats", "cli"])
    ap.add_argument("trace", nargs="?", help="stats: the kernel trace CSV")
    ap.add_argument("--save", default=None, metavar="FILE")
    a = ap.parse_args()
    res = kernels() if a.mode == "kernels" else stats(a.trace) if a.mode == "stats" else cli()
    print(json.dumps(res))
    if a.save:
        whole = json.load(open(a.save)) if os.path.exists(a.save) else {}
        whole[a.mode] = res
        with open(a.save, "w") as f:
            f.write(json.dumps(whole, indent=1) + "\n")


if __name__ == "__main__":
    main()
