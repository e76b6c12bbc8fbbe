"""v3d_xcorr's error per spectrum bin against the float64 correlation at every FFT size 2^10 .. 2^24: zero-mean white float32
tracks, n1 odd and unequal to n2, n1 + n2 - 1 in (N/2, N] and == N, both orders; tests/align_ref.py's spectral_error, in units
of eps32 log2 N (eps32 = 2^-24).  The bound K of tests/test_align_edges_gpu.py is four times the largest value.  Prints one JSON
line; --save writes profiles/align_accuracy.json.

    python tools/align_accuracy.py [--min 10] [--max 24] [--save]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-3d-pipeline_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min", type=int, default=10)
    ap.add_argument("--max", type=int, default=24)
    ap.add_argument("--save", action="store_true", help="write profiles/align_accuracy.json")
    args = ap.parse_args()
    import torch
    import align_ref as AR
    import envopts
    from video_3d_pipeline import _native as N
    envopts.select_variant_lib(N)
    if not torch.cuda.is_available():
        raise SystemExit("align_accuracy.py needs a GPU")
    per_m = {}
    for m in range(args.min, args.max + 1):
        rng = np.random.default_rng(7000 + m)
        vals = []
        for exact in (False, True):
            n1, n2 = AR.xcorr_sizes(m, exact)
            for a, b in ((n1, n2), (n2, n1)):
                a1, a2 = AR.white(a, rng), AR.white(b, rng)
                got = N.xcorr(N.to_device(a1), N.to_device(a2)).cpu().numpy().astype(np.float64)
                vals.append(round(AR.spectral_error(got, a1, a2), 3))
        per_m[str(m)] = {"plan": AR.plan_digits(m), "units": vals, "max": max(vals)}
        print(f"2^{m} {per_m[str(m)]}", file=sys.stderr, flush=True)
    worst = max(v["max"] for v in per_m.values())
    line = json.dumps({"metric": "max_k |rfft(got - want)_k| / rms_k |P_k| / (2^-24 log2 N)",
                       "cases": "(n1, n2), (n2, n1) with n1 + n2 - 1 = N - 37 (N - 5 at 2^10); the same with n1 + n2 - 1 = N",
                       "device": torch.cuda.get_device_name(0), "per_m": per_m, "max": worst, "K": round(4 * worst, 3)})
    print(line)
    if args.save:
        with open(os.path.join(ROOT, "profiles", "align_accuracy.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
