"""Rendered-eye fidelity (v3d_eye_fidelity_batch, --fidelity-report) on one GPU: kernel time per 4K frame from HIP events (8
distinct frames per launch, 3 warm-up and 20 timed launches), on the eyes of a full-SBS output at the gains of --parallax source.
The yardsticks are v3d_render_stereo_source_batch (fill_eyes 2) and v3d_verify_eye_source_batch at tau 765 (every cell read and
summed, none replaced: what the entry's first stage reads) in the same run.  Timed per geometry, alternating for ROUNDS rounds so
that a drift of the clock shows as a spread and not as a difference:

    render          the source render alone (fill_eyes 2)
    render_warp     the report's extra render (fill_eyes 0) into a scratch output
    verify_keep     the verification alone at tau 765
    fidelity        the entry on the right eye
    fidelity_left   the entry on the left eye against the stored left eye (the ceiling series)
    report          what the flag adds to a batch: the extra render and the three metric calls

Two geometries: `2x2`, a 1920 x 1080 stored eye (a 3840 x 1080 SBS frame) under the 3840 x 2160 frame, and `4x2`, the 960 x 1080
eye of tools/verify_rate.py.  The 4K frames are that tool's (smooth, +-4 of noise), the stored right eye is the rendered right eye
itself, box-reduced to the eye's size, with a tenth of its pixels moved by half the range; the stored left eye is the 4K frame
box-reduced.  Prints one JSON line and writes it to profiles/fidelity_rate.json.

    python tools/fidelity_rate.py
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
from verify_rate import smooth_frames  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

HS, ROUNDS, BAD, SHARE = 1080, 3, 48, 0.1
GEOMETRIES = {"2x2": 3840, "4x2": 1920}     # name -> width of the SBS frame


def _box(img, We):
    """u8 [n,H,W,3] -> the box-reduced eye u8 [n,HS,We,3]"""
    n = len(img)
    fy, fx = H // HS, W // We
    s = img.reshape(n, HS, fy, We, fx, 3).astype(np.uint32).sum(axis=(2, 4))
    return ((2 * s + fx * fy) // (2 * fx * fy)).astype(np.uint8)


def rates(f, d, name, Ws):
    p = convert.source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": Ws}, W)
    gains = N.stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    q = convert.fill_map_q16(None, (Ws // 2, HS), (W, H))
    cx, cy = N.verify_cell(q[0], q[2])
    out = torch.empty((NF, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    scratch = torch.empty_like(out)
    counts = torch.empty((NF,), dtype=torch.int32, device="cuda")
    rec = torch.empty((3, NF, N.FIDELITY_FIELDS), dtype=torch.int64, device="cuda")
    ws = torch.empty((N.lib().v3d_eye_fidelity_ws_bytes(NF, W, H, q[0], q[2]),), dtype=torch.uint8, device="cuda")
    left, right, wright = out[:, :, :W], out[:, :, W:], scratch[:, :, W:]
    N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, None, 0, *q, out=out)
    eye_r, eye_l = _box(right.cpu().numpy(), Ws // 2), _box(left.cpu().numpy(), Ws // 2)
    rng = np.random.default_rng(5)
    eye_r[rng.random(eye_r.shape[:3]) < SHARE] += 128
    sbs = torch.from_numpy(np.concatenate([eye_l, eye_r], axis=2)).cuda()

    def render():
        N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 2, *q, out=out)

    def render_warp():
        N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs, 0, *q, out=scratch)

    def fidelity(view=right, eye=1, k=1):
        N.eye_fidelity_batch(view, sbs, eye, *q, BAD, out=rec[k], ws=ws)

    def report():
        render_warp()
        fidelity(wright, 1, 0)
        fidelity(right, 1, 1)
        fidelity(left, 0, 2)

    render()
    calls = {"render": render, "render_warp": render_warp, "verify_keep": lambda: N.verify_eye_source_batch(right, sbs, 1, *q, 765, out=counts),
             "fidelity": fidelity, "fidelity_left": lambda: fidelity(left, 0, 2), "report": report}
    us = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for key, call in calls.items():
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                call()
            e1.record()
            torch.cuda.synchronize()
            us[key].append(round(e0.elapsed_time(e1) * 1e3 / (REPS * NF), 2))
    res = {key: {"us_per_frame": sorted(v)[len(v) // 2], "rounds": v} for key, v in us.items()}
    report()
    torch.cuda.synchronize()
    r = rec.cpu().numpy()
    for k, series in enumerate(("warp", "final", "ceiling")):
        t = r[k].sum(axis=0)
        res[series] = {"ssim": round(float(t[5]) / (1 << 20) / float(t[4]), 4), "mean_abs": round(float(t[1]) / (3 * float(t[0])), 3),
                       "bad_share": round(float(t[3]) / float(t[0]), 4)}
    res.update(source=f"{Ws}x{HS}", cell=[cx, cy], gains=list(gains), cells_windows=list(N.fidelity_grid(W, H, q[0], q[2])),
               ws_bytes_per_frame=ws.numel() // NF)
    res["fidelity_over_verify_keep"] = round(res["fidelity"]["us_per_frame"] / res["verify_keep"]["us_per_frame"], 3)
    res["report_over_render"] = round(res["report"]["us_per_frame"] / res["render"]["us_per_frame"], 3)
    return res


def main():
    _, depth = inputs(NF)
    f = torch.from_numpy(smooth_frames(NF)).cuda()
    d = torch.from_numpy(depth.view(np.int16)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "frames_per_launch": NF, "timed_launches": REPS, "rounds": ROUNDS,
           "bad_threshold": BAD, **{name: rates(f, d, name, Ws) for name, Ws in GEOMETRIES.items()}}
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "fidelity_rate.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
