"""Correlation lookup at 270x480x256, G = 4 (BASELINE configs[3]), both patterns, default route: us per call from HIP events, the
median of 5 samples of 50 calls after 10 warm-up calls.  Prints one JSON line.  V3D_HIP_LIB=path times another build of the library
(an A/B against the parent's: alternate fresh processes).

    python tools/corr_rate.py
"""
import json
import os
import sys

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]
from video_3d_pipeline import _native as N  # noqa: E402
import envopts  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)
h, w, G = 270, 480, 4
g = torch.Generator(device="cuda").manual_seed(0)
fl = torch.randn((h, w, 64 * G), generator=g, device="cuda").bfloat16()
fr = torch.randn((h, w, 64 * G), generator=g, device="cuda").bfloat16()
flow = (torch.rand((2, h, w), generator=g, device="cuda") * 8 - 4).float()
res = {}
for pattern in (0, 1):
    for _ in range(10):
        N.corr_lookup(fl, fr, flow, G, pattern)
    torch.cuda.synchronize()
    ts = []
    for rep in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            N.corr_lookup(fl, fr, flow, G, pattern)
        e1.record()
        torch.cuda.synchronize()
        ts.append(round(e0.elapsed_time(e1) * 1e3 / 50, 2))
    res[f"pattern{pattern}_us"] = sorted(ts)[2]
print(json.dumps(res))
