"""sha256 of the guided filter's outputs on clean inputs, per input type (int16 disparity, u16 samples, float32), radius (1, 8, 16),
route (fused, sweeps, tiled) and geometry (two exact 2x, one 3x): one line per case and one digest over all int16 and u16 lines.
V3D_HIP_LIB=path hashes another build of the library: equal lines mean equal output bits (a change of the float route's loads
must leave the int16 and u16 routes alone).

    python tools/gf_route_hash.py
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd")]
from video_3d_pipeline import _native as N  # noqa: E402
import envopts  # noqa: E402

envopts.select_variant_lib(N)               # V3D_HIP_LIB=path: an experiment build of the library (development only)
ROUTES = {"fused": {"gf_fused": 1, "gf_tiled": 0}, "sweeps": {"gf_fused": 0, "gf_tiled": 0}, "tiled": {"gf_fused": 1, "gf_tiled": 1}}
rng = np.random.default_rng(7)
both = hashlib.sha256()
for (Wlo, Hlo, s) in ((48, 27, 2), (96, 54, 2), (50, 30, 3)):
    disp = rng.integers(-16, 1000, (3, Hlo, Wlo)).astype(np.int16)
    u16 = (np.maximum(disp, 0).astype(np.uint16) * 60).view(np.int16)
    guide = rng.integers(0, 256, (3, Hlo * s, Wlo * s), dtype=np.uint8)
    f32 = np.where(disp > 0, disp / 16.0, 0).astype(np.float32)
    for r in (1, 8, 16):
        for route, opts in ROUTES.items():
            for k, v in opts.items():
                N.set_option(k, v)
            a = N.guided_upscale_batch(torch.from_numpy(disp).cuda(), torch.from_numpy(guide).cuda(), r, 1e-3).cpu().numpy()
            b = N.guided_upscale_u16_batch(torch.from_numpy(u16).cuda(), torch.from_numpy(guide).cuda(), r, 1e-3).cpu().numpy()
            c = N.guided_upscale_batch(torch.from_numpy(f32).cuda(), torch.from_numpy(guide).cuda(), r, 1e-3).cpu().numpy()
            both.update(a.tobytes() + b.tobytes())
            print(f"{Wlo}x{Hlo}x{s} r={r} {route}: int16 {hashlib.sha256(a.tobytes()).hexdigest()[:16]} u16 {hashlib.sha256(b.tobytes()).hexdigest()[:16]} f32 {hashlib.sha256(c.tobytes()).hexdigest()[:16]}")
print(f"all int16 and u16 outputs: {both.hexdigest()}")
