"""Source-fused right eye (v3d_fuse_eye_source_batch) on one GPU: kernel time per 4K frame from HIP events (8 distinct frames per
launch, 3 warm-up and 20 timed launches), on the right eye of a full-SBS output at the gains of --parallax source.  The frames,
shapes and timing scheme are those of tools/verify_rate.py; the yardsticks are v3d_render_stereo_source_batch (fill_eyes 2) and
v3d_verify_eye_source_batch in the same run.  Timed, alternating for ROUNDS rounds so that a drift of the clock shows as a spread and
not as a difference:

    render               the source render alone
    render_verify        the render, then the verification of its right eye at tau 48 (a stored eye that disagrees with the render
                         in about a tenth of the cells)
    render_verify_fuse   the convert step's sequence with --verify-source --fuse-source: the same, then the fusion
    fuse                 the fusion alone, over and over on the same eye (it works in place: the eye drifts towards the stored
                         eye's low band, which changes no address and no amount of work)

The fusion's algorithmic bytes per frame are the eye read twice and written once and the stored eye and the means plane read and
written once each (the taps of both come from cache); the share of the 8 TB/s roofline is those bytes over the time of `fuse`.
The entry's two kernels cannot be launched apart: their split comes from a `rocprofv3 --kernel-trace --stats` run of this tool
(k_fuse_means and k_fuse_apply in its kernel statistics).  Prints one JSON line and writes it to profiles/fuse_rate.json.

    python tools/fuse_rate.py
"""
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
from verify_rate import HS, ROUNDS, TAU, WS, smooth_frames  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

SHARE = 0.1
ROOFLINE = 8e12                             # bytes per second


def rates():
    _, depth = inputs(NF)
    f = torch.from_numpy(smooth_frames(NF)).cuda()
    d = torch.from_numpy(depth.view(np.int16)).cuda()
    p = convert.source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": WS}, W)
    gains = N.stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    q = convert.fill_map_q16(None, (WS // 2, HS), (W, H))
    out = torch.empty((NF, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    counts = torch.empty((NF,), dtype=torch.int32, device="cuda")
    ws = torch.empty((N.fuse_eye_source_ws_bytes(NF, WS, HS),), dtype=torch.uint8, device="cuda")
    right = out[:, :, W:]
    # the stored eyes: the render's own right eye (holes from the background), box-reduced, then changed in a share of its pixels
    N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, None, 0, *q, out=out)
    eye = right.cpu().numpy().reshape(NF, HS, 2, WS // 2, 4, 3).astype(np.uint16).sum(axis=(2, 4))
    eye = ((eye + 4) // 8).astype(np.uint8)
    e = eye.copy()
    e[np.random.default_rng(5).random(e.shape[:3]) < SHARE] += 128
    sbs = torch.from_numpy(np.concatenate([eye, e], axis=2)).cuda()

    def render():
        N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 2, *q, out=out)

    def render_verify():
        render()
        N.verify_eye_source_batch(right, sbs, 1, *q, TAU, out=counts)

    def render_verify_fuse():
        render_verify()
        N.fuse_eye_source_batch(right, sbs, 1, *q, ws=ws)

    calls = {"render": render, "render_verify": render_verify, "render_verify_fuse": render_verify_fuse,
             "fuse": lambda: N.fuse_eye_source_batch(right, sbs, 1, *q, ws=ws)}
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
            us[name].append(round(e0.elapsed_time(e1) * 1e3 / (REPS * NF), 2))
    res = {name: {"us_per_frame": sorted(v)[len(v) // 2], "rounds": v} for name, v in us.items()}
    t = {k: r["us_per_frame"] for k, r in res.items()}
    eye_bytes, low_bytes = 3 * W * H, 3 * (WS // 2) * HS
    alg = 3 * eye_bytes + 3 * low_bytes                        # E read twice and written once; the stored eye read, M written and read
    res.update(gains=list(gains), tau=TAU, map=list(q), algorithmic_bytes_per_frame=alg,
               verify_us=round(t["render_verify"] - t["render"], 2), fuse_after_verify_us=round(t["render_verify_fuse"] - t["render_verify"], 2),
               fuse_roofline_share=round(alg / (t["fuse"] * 1e-6) / ROOFLINE, 4), fuse_over_render=round(t["fuse"] / t["render"], 3),
               fuse_over_verify=round(t["fuse"] / max(t["render_verify"] - t["render"], 1e-9), 3))
    return res


def main():
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "source": f"{WS}x{HS}", "frames_per_launch": NF,
           "timed_launches": REPS, "rounds": ROUNDS, **rates()}
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "fuse_rate.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
