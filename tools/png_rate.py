"""GPU PNG encoding (--png-encoder gpu): size and kernel time of v3d_png_deflate_batch.  Prints one JSON line and, with
--save, writes it to profiles/png_rate.json.

    python tools/png_rate.py --cpu          # size only, on the CPU: tests/png_ref.py is bit-exact, no GPU needed
    python tools/png_rate.py [--save]       # + the device's streams on product frames and the launch set's time

Size: bytes of the stream over zlib.compress(payload, 1) on the same payload, for the two seeded inputs of
tests/test_png_ref.py (CPU reference) and, on the GPU, for the frames the product makes: the depth path's 1080p u16 maps of
the synthetic clip, their 4K guided upscale, and the 7680x2160 side-by-side frames DIBR renders from them.
Time: the four launches from HIP events, warmed, best of 5, for 34 x 1080p gray16, 8 x 4K gray16 and 4 x (7680x2160) BGR8;
input + output bytes over that time against the 8 TB/s HBM roofline (the slots in `ws` are written and read once more on top).
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-pipeline_amd"), os.path.join(ROOT, "tests")]
import png_ref as P  # noqa: E402

HBM = 8.0e12


def seeded_sizes():
    out = {}
    for name, img, fmt in (("depth_1920x96_u16", P.seeded_depth(), P.GRAY16), ("rgb_1920x48_noise1.5", P.seeded_rgb(), P.BGR8)):
        raw = P.raw_rows(img, fmt).tobytes()
        s, used = P.stream(img, fmt, want_books=True)
        z1 = len(zlib.compress(raw, 1))
        out[name] = {"payload_bytes": len(raw), "stream_bytes": len(s), "zlib1_bytes": z1, "ratio_to_zlib1": round(len(s) / z1, 4),
                     "book0_only_ratio_to_zlib1": round(len(P.stream(img, fmt, 0)) / z1, 4),
                     "books_used": {P.BOOKS[k]["name"]: int(c) for k, c in enumerate(np.bincount(used, minlength=P.K)) if c}}
    return out


def product_frames():
    """device tensors of the frames the sinks see: 1080p u16 depth, its 4K upscale, the 7680x2160 stereo frames"""
    import torch
    from video_3d_pipeline import _native as N, synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend
    W, H, n = 1920, 1080, 4
    be = HipPipelineBackend()
    frames = [syn.sbs_frame(W, H, i) for i in range(n)]
    u16 = be.depth_to_u16_batch(be.sbs_to_disparity(frames, True)).clone()
    guides = [np.repeat(syn.guide_frame(W, H, i)[..., None], 3, axis=2) for i in range(n)]
    q = be.guided_upscale_u16(u16, be.guide_luma(guides, 2 * H, 2 * W, n), 8, 1e-3).clone()
    gl, gr, conv = N.stereo_gains()
    sbs3d = N.render_stereo_batch(be._bufs["guide_dev"][:n], q, gl, gr, conv, N.STEREO_FULL_SBS).clone()
    torch.cuda.synchronize()
    return {"depth_1080p": u16, "depth_4k": q, "stereo_7680x2160": sbs3d}


def device_sizes(frames):
    import torch
    from video_3d_pipeline import _native as N, utils
    out = {}
    for name, t in frames.items():
        fmt = P.GRAY16 if t.dim() == 3 else P.BGR8
        o, off = N.png_deflate_batch(t)
        torch.cuda.synchronize()
        o, off = o.cpu().numpy(), off.cpu().tolist()
        host = t.cpu().numpy()
        ratios = []
        for f in range(t.shape[0]):
            img = host[f].view(np.uint16) if fmt == P.GRAY16 else host[f]
            raw = P.raw_rows(img, fmt).tobytes()
            s = bytes(o[off[f]:utils.png_stream_end(o, off[f], off[f + 1])])
            assert zlib.decompress(s) == raw
            ratios.append(len(s) / len(zlib.compress(raw, 1)))
        out[name] = {"frames": t.shape[0], "ratio_to_zlib1": [round(r, 4) for r in ratios], "stream_over_payload": round(len(s) / len(raw), 4)}
    return out


def kernel_times(frames):
    import torch
    from video_3d_pipeline import _native as N
    out = {}
    for name, src, n in (("34x1080p_gray16", frames["depth_1080p"], 34), ("8x4K_gray16", frames["depth_4k"], 8),
                         ("4x7680x2160_bgr8", frames["stereo_7680x2160"], 4)):
        t = src[torch.arange(n, device=src.device) % src.shape[0]].contiguous()
        fmt = P.GRAY16 if t.dim() == 3 else P.BGR8
        H, W = t.shape[1:3]
        L = N.lib()
        o = torch.empty(L.v3d_png_out_bytes(fmt, n, W, H), dtype=torch.uint8, device="cuda")
        ws = torch.empty(L.v3d_png_ws_bytes(fmt, n, W, H), dtype=torch.uint8, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        for _ in range(2):
            N.png_deflate_batch(t, out=o, offsets=off, ws=ws)
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            N.png_deflate_batch(t, out=o, offsets=off, ws=ws)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        used, nbytes = int(off[n]), t.numel() * t.element_size()
        best = min(ms)
        out[name] = {"ms": [round(m, 3) for m in ms], "best_ms": round(best, 3), "ms_per_frame": round(best / n, 4),
                     "input_bytes": nbytes, "output_bytes": used, "capacity_bytes": o.numel(),
                     "in_plus_out_TBps": round((nbytes + used) / (best * 1e-3) / 1e12, 3),
                     "fraction_of_hbm_roofline_8TBps": round((nbytes + used) / (best * 1e-3) / HBM, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="size of the two seeded inputs only (no GPU)")
    ap.add_argument("--save", action="store_true", help="also write profiles/png_rate.json")
    a = ap.parse_args()
    res = {"books": P.K, "seeded": seeded_sizes()}
    if not a.cpu:
        import torch
        import envopts
        from video_3d_pipeline import _native as N
        envopts.select_variant_lib(N)       # V3D_HIP_LIB=path: an experiment build of the library (development only)
        frames = product_frames()
        res.update(device=torch.cuda.get_device_name(0), product=device_sizes(frames), kernel=kernel_times(frames))
    line = json.dumps(res)
    print(line)
    if a.save:
        with open(os.path.join(ROOT, "profiles", "png_rate.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
