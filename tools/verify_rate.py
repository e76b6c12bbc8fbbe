"""Source-verified right eye (v3d_verify_eye_source_batch) on one GPU: kernel time per 4K frame from HIP events (8 distinct
frames per launch, 3 warm-up and 20 timed launches), on the right eye of a full-SBS output at the gains of --parallax source.  The
yardstick is v3d_render_stereo_source_batch (fill_eyes 2) in the same run.  Timed, alternating for ROUNDS rounds so that a drift of
the clock shows as a spread and not as a difference:

    render              the source render alone
    render_verify_S     the convert step's sequence: the render, then the verification of its right eye at tau 48, against a
                        stored eye that disagrees with the render in about the share S of the cells (0, 0.1 and 1)
    verify_keep         the verification alone at tau 765: every cell read and summed, none replaced (the entry works in place, so
                        a second call at any other tau would find the cells of the first already replaced)

The 4K frames are smooth (two sinusoids and +-4 of noise), the eye source is a 1920 x 1080 SBS frame per 4K frame whose stored
right eye is the rendered right eye itself, box-reduced 4 x 2, with the share S of its pixels moved by half the range: a cell then
disagrees where a changed pixel is among its taps.  The replaced share is the entry's own count.  Prints one JSON line and writes
it to profiles/verify_rate.json.

    python tools/verify_rate.py
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

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)

WS, HS, ROUNDS, TAU, SHARES = 1920, 1080, 3, 48, (0.0, 0.1, 1.0)


def smooth_frames(n):
    rng = np.random.default_rng(3)
    y, x = np.arange(H, dtype=np.float32)[:, None], np.arange(W, dtype=np.float32)[None, :]
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            plane = 128 + 60 * np.sin(x / (90 + 20 * c) + i) + 50 * np.sin(y / (70 + 10 * c) - i) + rng.integers(-4, 5, (H, W))
            out[i, :, :, c] = np.clip(plane, 0, 255)
    return out


def rates():
    _, depth = inputs(NF)
    f = torch.from_numpy(smooth_frames(NF)).cuda()
    d = torch.from_numpy(depth.view(np.int16)).cuda()
    p = convert.source_parallax({"mode": "metric", "lo": 0, "hi": 64, "min_disparity": 0, "eye_width": WS}, W)
    gains = N.stereo_gains(p["max_shift"], p["convergence"], p["eye_split"])
    q = convert.fill_map_q16(None, (WS // 2, HS), (W, H))
    cx, cy = N.verify_cell(q[0], q[2])
    cells = -(-W // cx) * -(-H // cy)
    out = torch.empty((NF, H, 2 * W, 3), dtype=torch.uint8, device="cuda")
    counts = torch.empty((NF,), dtype=torch.int32, device="cuda")
    right = out[:, :, W:]
    # the stored eyes: the render's own right eye (holes from the background), box-reduced, then changed in a share of its pixels
    N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, None, 0, *q, out=out)
    eye = right.cpu().numpy().reshape(NF, HS, 2, WS // 2, 4, 3).astype(np.uint16).sum(axis=(2, 4))
    eye = ((eye + 4) // 8).astype(np.uint8)
    rng = np.random.default_rng(5)
    sbs = {}
    for s in SHARES:
        e = eye.copy()
        e[rng.random(e.shape[:3]) < s] += 128
        sbs[s] = torch.from_numpy(np.concatenate([eye, e], axis=2)).cuda()

    def render(s=SHARES[0]):
        N.render_stereo_source_batch(f, d, *gains, N.STEREO_PACK_FULL_SBS, sbs[s], 2, *q, out=out)

    def render_verify(s):
        render(s)
        N.verify_eye_source_batch(right, sbs[s], 1, *q, TAU, out=counts)

    calls = {"render": render, "verify_keep": lambda: N.verify_eye_source_batch(right, sbs[SHARES[0]], 1, *q, 765, out=counts)}
    calls.update({f"render_verify_{s:g}": (lambda s=s: render_verify(s)) for s in SHARES})
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
    for s in SHARES:
        render_verify(s)
        torch.cuda.synchronize()
        r = res[f"render_verify_{s:g}"]
        r["replaced_share"] = round(float(counts.cpu().numpy().view(np.uint32).mean()) / cells, 4)
        r["verify_us"] = round(r["us_per_frame"] - res["render"]["us_per_frame"], 2)
    res.update(gains=list(gains), tau=TAU, cell=[cx, cy])
    res["verify_keep_over_render"] = round(res["verify_keep"]["us_per_frame"] / res["render"]["us_per_frame"], 3)
    return res


def main():
    res = {"device": torch.cuda.get_device_name(0), "size": f"{W}x{H}", "source": f"{WS}x{HS}", "frames_per_launch": NF,
           "timed_launches": REPS, "rounds": ROUNDS, **rates()}
    line = json.dumps(res)
    print(line)
    with open(os.path.join(ROOT, "profiles", "verify_rate.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
