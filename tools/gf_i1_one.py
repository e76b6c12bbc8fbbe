"""The fused guided filter alone on one 34-frame batch of random int16 disparity and guide (1080p -> 4K, r = 8: the integer
route the headline runs), timed with HIP events: target of rocprofv3 passes and source of profiles/gff_valu_kernel_alone.txt.
V3D_HIP_LIB=path times another build of the library, GF_COLS=512 the wide strips, GF_REPS the launches (default 5)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "video-3d-pipeline_amd"))
import numpy as np, torch
from video_3d_pipeline import _native as N
import envopts; envopts.select_variant_lib(N)
if os.environ.get("GF_COLS"): N.set_option("gf_cols", int(os.environ["GF_COLS"]))
W, H, B = 1920, 1080, 34
g = torch.Generator(device="cuda").manual_seed(1)
disp = torch.randint(-16, 1024, (B, H, W), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
guide = torch.randint(0, 256, (B, 2 * H, 2 * W), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)
out = torch.empty((B, 2 * H, 2 * W), dtype=torch.float32, device="cuda")
for _ in range(2): N.guided_upscale_batch(disp, guide, 8, 1e-3, out)
torch.cuda.synchronize(); e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True); e0.record()
R = int(os.environ.get("GF_REPS", "5"))
for _ in range(R): N.guided_upscale_batch(disp, guide, 8, 1e-3, out)
e1.record(); torch.cuda.synchronize()
import hashlib
print("guided i1 batch", B, "lib", os.environ.get("V3D_HIP_LIB", "tree"), "cols", os.environ.get("GF_COLS", "256"), ":", e0.elapsed_time(e1) / R, "ms",
      "sha", hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16], flush=True)
