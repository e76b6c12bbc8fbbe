"""Time v3d_align_audio (HIP events) on two 300 s tracks at 22,050 Hz, and scipy.signal.correlate(..., method='fft') on
the CPU for comparison.  Prints one JSON line.

    python tools/align_rate.py [--seconds 300] [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-3d-pipeline_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=2)
    args = ap.parse_args()
    import torch
    from video_3d_pipeline import _native as N
    if not torch.cuda.is_available():
        raise SystemExit("align_rate.py needs a GPU")
    n = int(args.seconds * args.rate)
    rng = np.random.default_rng(0)
    s = rng.standard_normal(n + 50000).astype(np.float32)
    a1 = s[:n] + 0.3 * rng.standard_normal(n).astype(np.float32)
    a2 = s[12345:12345 + n] + 0.3 * rng.standard_normal(n).astype(np.float32)
    d1, d2 = N.to_device(a1), N.to_device(a2)
    ws_bytes = int(N.lib().v3d_xcorr_ws_bytes(n, n))
    for _ in range(3):
        res = N.align_audio(d1, d2)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(args.reps):
        ev[0].record()
        res = N.align_audio(d1, d2)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    r = res.cpu().numpy()
    cpu_ms = None
    try:
        from scipy import signal
        a1n = (a1 - a1.mean()) / (a1.std() + 1e-10)
        a2n = (a2 - a2.mean()) / (a2.std() + 1e-10)
        ct = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            c = signal.correlate(a2n, a1n, mode="full", method="fft")
            int(np.argmax(np.abs(c)))
            ct.append((time.perf_counter() - t0) * 1e3)
        cpu_ms = min(ct)
    except ImportError:
        pass
    print(json.dumps({"samples_per_track": n, "fft_points": 1 << int(np.ceil(np.log2(2 * n - 1))), "ws_bytes": ws_bytes,
                      "gpu_ms_median": float(np.median(times)), "gpu_ms_min": float(np.min(times)),
                      "gpu_ms_max": float(np.max(times)), "lag": int(r[0]), "expected_lag": -12345,
                      "strength": float(r[2]), "cpu_scipy_fft_ms": cpu_ms,
                      "cpu_threads": os.environ.get("OMP_NUM_THREADS")}))


if __name__ == "__main__":
    main()
