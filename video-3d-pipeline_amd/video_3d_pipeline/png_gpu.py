"""--png-encoder {zlib,gpu}: where the PNG sinks of the depth, upscale, one-pass pipeline and convert paths compress.

zlib (the default): the writer threads run utils.encode_png16 / encode_png8 on pixels that crossed PCIe -- 20 ms of deflate per
1080p map, 80 ms per 4K map on one core.  gpu: the final u16 / BGR frames are deflated on the device while they are still
there (v3d_png_deflate_batch; contract in include/v3d_hip.h and tests/png_ref.py), only the compressed streams cross, and the
writer threads add the PNG chunks and the CRC-32 (utils.png_from_stream) and write the file.  Same file names, same decoded
pixels; the bytes of the IDAT chunk differ (another deflate of the same payload).
"""
from functools import partial

import numpy as np

from .utils import png_from_stream, png_stream_end

PNG_ENCODERS = ("zlib", "gpu")


def check_png_encoder(value) -> str:
    if value not in PNG_ENCODERS:
        raise ValueError(f"png_encoder must be one of {PNG_ENCODERS}, got {value!r}")
    return value


def add_png_arguments(parser):
    """--png-encoder, shared by the depth, upscale, pipeline and convert CLIs"""
    parser.add_argument('--png-encoder', choices=list(PNG_ENCODERS), default='zlib',
                        help='Where the PNG frames are compressed: zlib on the writer threads (default), or gpu: deflate on the '
                             'device before the frames cross PCIe (same pixels, the host only adds the PNG chunks)')


def png_options(args) -> dict:
    return dict(png_encoder=args.png_encoder)


def gray16_file(w: int, h: int):
    """encode= of PngWriterPool.submit for a ready 16-bit gray stream"""
    return partial(png_from_stream, w=w, h=h, bit_depth=16, colour_type=0)


def rgb8_file(w: int, h: int):
    return partial(png_from_stream, w=w, h=h, bit_depth=8, colour_type=2)


class DevicePngEncoder:
    """Final frames on the device -> one zlib stream per frame on the host.  Owns the encoder's workspace, its output buffer and
    the pinned word the offsets land in; per batch one launch set, a D2H of the offsets, ONE D2H of the used bytes and a
    synchronise.  The streams are views of a pinned block from torch's caching host allocator, which takes it back once the
    writers have dropped the last of them."""

    def __init__(self, torch, native, device):
        self.torch, self.native, self.device = torch, native, device
        self._key = self._out = self._ws = self._off = self._off_host = None

    def _buffers(self, fmt, n, W, H):
        torch, L = self.torch, self.native.lib()
        if self._key != (fmt, n, W, H):
            need_out, need_ws = L.v3d_png_out_bytes(fmt, n, W, H), L.v3d_png_ws_bytes(fmt, n, W, H)
            if not need_out:
                raise ValueError(f"--png-encoder gpu: {n} frames of {W}x{H} are outside the encoder's range "
                                 f"(W <= {self.native.PNG_MAX_WIDTH}, H <= {self.native.PNG_MAX_HEIGHT})")
            if self._out is None or self._out.numel() < need_out:
                self._out = torch.empty(need_out, dtype=torch.uint8, device=self.device)
            if self._ws is None or self._ws.numel() < need_ws:
                self._ws = torch.empty(need_ws, dtype=torch.uint8, device=self.device)
            if self._off is None or self._off.numel() < n + 1:
                self._off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
                self._off_host = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
            self._key = (fmt, n, W, H)
        return self._out, self._ws, self._off, self._off_host

    def encode(self, frames):
        """int16 [n,H,W] (u16 bit patterns) or uint8 [n,H,W,3] (BGR) device tensor -> list of n uint8 NumPy views, the streams"""
        torch, nat = self.torch, self.native
        fmt = nat.PNG_GRAY16 if frames.dim() == 3 else nat.PNG_BGR8
        n, H, W = frames.shape[:3]
        out, ws, off, off_host = self._buffers(fmt, n, W, H)
        with torch.cuda.device(self.device):
            nat.png_deflate_batch(frames, out=out, offsets=off, ws=ws)
            off_host[:n + 1].copy_(off[:n + 1], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            starts = off_host[:n + 1].tolist()
            host = torch.empty(starts[n], dtype=torch.uint8, pin_memory=True)
            host.copy_(out[:starts[n]], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        buf = host.numpy()
        return [buf[starts[f]:png_stream_end(buf, starts[f], starts[f + 1])] for f in range(n)]
