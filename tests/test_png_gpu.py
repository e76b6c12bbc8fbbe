"""v3d_png_deflate_batch against tests/png_ref.py, byte for byte: streams, offsets, zero gaps and tail.

Shapes: widths of 1 .. 97 positions per thread, around a multiple of the 16-byte load (127 / 128 / 129, 85 / 86), one row and
several; every call is a batch of 3 frames that start at odd element offsets with a padded stride, and every frame is encoded
once more alone (n = 1), which must give the same bytes.  Row content (png_ref.content_rows): noise, a constant row (at
W = 8192 one run of 63 maximal matches and a remainder), runs of exactly 2 .. 518 matching bytes, runs that end on, before and
after every thread's border, and rows drawn from the model of every code book."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import png_ref as P

SHAPES = [(P.GRAY16, W, H) for W in (1, 2, 127, 128, 129, 1001, 8192) for H in (1, 5)] + \
         [(P.BGR8, W, H) for W in (1, 85, 86, 2731, 8192) for H in (1, 4)]
N = 3


@functools.lru_cache(maxsize=None)
def _case(fmt, W, H):
    frames = [P.content_image(fmt, W, H, 5 * W + H + 2 * f) for f in range(N)]
    return frames, P.batch(frames, fmt)


def _on_device(frames, fmt, pad, skew):
    """the frames in one device buffer, `skew` elements in, `pad` elements between them -> a strided [n,H,W(,3)] view"""
    import torch
    a = np.stack(frames)
    n, per = a.shape[0], a[0].size
    host = np.full(skew + n * (per + pad), 0xA5A5 if fmt == P.GRAY16 else 0xA5, a.dtype)
    for f in range(n):
        host[skew + f * (per + pad):skew + f * (per + pad) + per] = a[f].reshape(-1)
    t = torch.from_numpy(host.view(np.int16) if fmt == P.GRAY16 else host).cuda()
    return torch.as_strided(t, a.shape, (per + pad,) + tuple(s // a.itemsize for s in a[0].strides), skew)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,W,H", SHAPES, ids=[f"{'g16' if f == 0 else 'bgr'}-{w}x{h}" for f, w, h in SHAPES])
def test_streams_and_offsets_equal_the_reference(native, fmt, W, H):
    import torch
    frames, (want, want_off, streams) = _case(fmt, W, H)
    out, off = native.png_deflate_batch(_on_device(frames, fmt, 7, 1))
    torch.cuda.synchronize()
    got, got_off = out.cpu().numpy(), off.cpu().numpy().astype(np.uint64)
    assert got.size == P.out_bytes(fmt, N, W, H) == native.lib().v3d_png_out_bytes(fmt, N, W, H)
    assert np.array_equal(got_off, want_off), (got_off, want_off)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0])} (frame starts {want_off.tolist()})"
    from video_3d_pipeline import utils
    for f in range(N):
        lo, hi = int(want_off[f]), int(want_off[f + 1])
        assert utils.png_stream_end(got, lo, hi) == lo + len(streams[f])
        alone, aoff = native.png_deflate_batch(_on_device(frames[f:f + 1], fmt, 0, 0))
        torch.cuda.synchronize()
        assert int(aoff[1]) == hi - lo and bytes(alone.cpu().numpy()[:len(streams[f])]) == streams[f], f"frame {f} alone differs"
        assert not alone.cpu().numpy()[len(streams[f]):].any()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,n", [(3, 2, 300), (64, 300, 2)], ids=["3x2x300", "64x300x2"])
def test_many_frames_and_many_rows_byte_for_byte(native, W, H, n):
    """more than 256 frames: the second round of k_png_offsets and its carry; more than 256 rows: the second round of k_png_frame"""
    import torch
    frames = [P.content_image(P.GRAY16, W, H, 3 * W + f) for f in range(n)]
    want, want_off, _ = P.batch(frames, P.GRAY16)
    out, off = native.png_deflate_batch(_on_device(frames, P.GRAY16, 3, 1))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.size == want.size and np.array_equal(off.cpu().numpy().astype(np.uint64), want_off)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0])}"


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [P.GRAY16, P.BGR8], ids=["g16", "bgr"])
def test_product_size_frame_inflates_to_the_payload(native, fmt):
    """3840 x 2160, one frame: zlib.decompress == the host encoder's payload (no Python reference at this size)"""
    import torch
    from video_3d_pipeline import utils
    W, H = 3840, 2160
    img = np.tile(P.seeded_depth(W, 135, 5), (16, 1)) if fmt == P.GRAY16 else np.tile(P.seeded_rgb(W, 135, 6), (16, 1, 1))
    img[7] = img[7, 0]                                                # one constant row
    t = torch.from_numpy(img.view(np.int16) if fmt == P.GRAY16 else img).cuda()[None]
    out, off = native.png_deflate_batch(t)
    torch.cuda.synchronize()
    got, end = out.cpu().numpy(), int(off[1])
    assert int(off[0]) == 0 and end % 16 == 0 and end <= P.out_bytes(fmt, 1, W, H) and not got[end:].any()
    e = utils.png_stream_end(got, 0, end)
    raw = P.raw_rows(img, fmt).tobytes()
    d = zlib.decompressobj()
    assert d.decompress(bytes(got[:e])) == raw and d.eof and not d.unused_data
    print(f"fmt {fmt}: {e} bytes, {e / len(zlib.compress(raw, 1)):.3f} of zlib level 1")


@pytest.mark.gpu
def test_refusals_match_the_header(native):
    import torch
    L = native.lib()
    W, H, n = 64, 4, 2
    img = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
    out = torch.full((L.v3d_png_out_bytes(0, n, W, H),), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.v3d_png_ws_bytes(0, n, W, H) + 16, dtype=torch.uint8, device="cuda")
    P_, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i, o, f, w = img.data_ptr(), out.data_ptr(), off.data_ptr(), ws.data_ptr()
    call = lambda i=i, fs=2 * W * H, fmt=0, n=n, W=W, H=H, o=o, f=f, w=w: L.v3d_png_deflate_batch(P_(i), fs, fmt, n, W, H, P_(o), P_(f), P_(w), st)
    ARG, UNSUP = -1, -3
    for what, rc, kw in (("null img", ARG, dict(i=None)), ("null out", ARG, dict(o=None)), ("null offsets", ARG, dict(f=None)),
                         ("null ws", ARG, dict(w=None)), ("n = 0", ARG, dict(n=0)), ("n = 65536", ARG, dict(n=65536)),
                         ("W = 0", ARG, dict(W=0)), ("H = 0", ARG, dict(H=0)), ("fmt = 2", ARG, dict(fmt=2)), ("fmt = -1", ARG, dict(fmt=-1)),
                         ("stride below a frame", ARG, dict(fs=2 * W * H - 2)), ("misaligned ws", ARG, dict(w=w + 8)),
                         ("misaligned offsets", ARG, dict(f=f + 4)), ("odd gray16 pointer", ARG, dict(i=i + 1)),
                         ("W = 8193", UNSUP, dict(W=8193, n=1)), ("H = 65536", UNSUP, dict(H=65536, n=1))):
        assert call(**kw) == rc, what
        assert L.v3d_last_error(), what
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (off == -1).all(), "a refused call wrote"
    assert call(fs=0, n=1) == 0                                       # n == 1 ignores the stride
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    for fmt in (0, 1):
        assert L.v3d_png_stream_bound(fmt, W, H) == P.stream_bound(fmt, W, H) and L.v3d_png_out_bytes(fmt, 5, 8192, 7) == P.out_bytes(fmt, 5, 8192, 7)
        for bad in ((fmt, 0, W, H), (fmt, 65536, W, H), (fmt, 1, 0, H), (fmt, 1, W, 0), (fmt, 1, 8193, H), (fmt, 1, W, 65536), (2, 1, W, H)):
            assert L.v3d_png_out_bytes(*bad) == 0 and L.v3d_png_ws_bytes(*bad) == 0 and P.out_bytes(*bad) == 0, bad
        for bad in ((fmt, 0, H), (fmt, W, 0), (fmt, 8193, H), (fmt, W, 65536), (2, W, H)):
            assert L.v3d_png_stream_bound(*bad) == 0 and P.stream_bound(*bad) == 0, bad
