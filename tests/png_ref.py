"""CPU reference of the GPU PNG encoder's stream contract (include/v3d_hip.h, v3d_png_deflate_batch; DESIGN.md section 4,
"GPU PNG encoding").  csrc/v3d_png.hip must produce these bytes, bit for bit.  NumPy for everything per byte, Python loops
only per row.

The stream of one frame (a complete zlib stream, RFC 1950 / 1951):
    78 01
    per scanline: one deflate block (BFINAL = 0) coded with ONE code book, then an empty stored block that realigns to a byte:
        header of the book (3 bits for book 0, the fixed code; the constant dynamic header otherwise)
        tokens, end-of-block code
        000, zero bits up to the next byte boundary, 00 00 FF FF
    01 00 00 FF FF                      the final, empty stored block
    Adler-32 of the payload, big-endian

The payload of a scanline is the byte 1 (filter "sub") and the filtered samples: RL = 1 + bpp * W bytes, byte for byte what
utils.encode_png16 / encode_png8(bgr=True) hand to zlib.  Tokens of a scanline, i counting from its filter byte:
    m[i] = i >= bpp and raw[i] == raw[i - bpp]
    a maximal run of L true positions starting at s: matches of length 258 (distance bpp) at s, s + 258, ... while 258 fit,
    then the remainder r = L % 258: one match of length r if r >= 3, else r literals; every other position is a literal.
The book of a scanline is the one with the fewest bits, header + codes (the extra bits are the same for all), ties to the
lowest index.  Frames of a batch start at multiples of 16 in `out`; what lies between and behind them is zero."""
import os
import struct
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_png_books  # noqa: E402

GRAY16, BGR8 = 0, 1
BPP = {GRAY16: 2, BGR8: 3}
MAX_W, MAX_H, MAX_N = 8192, 65535, 65535
BOOKS = make_png_books.books()
K = len(BOOKS)
_LL_LEN = np.array([b["ll_len"] for b in BOOKS], np.int64)              # [K][286]
_LL_CODE = np.array([b["ll_code"] for b in BOOKS], np.uint64)
_HDR_BITS = np.array([b["hdr_bits"] for b in BOOKS], np.int64)

# length 3 .. 258 -> symbol, extra bits, extra value (RFC 1951 3.2.5)
_LEN_SYM = np.zeros(259, np.int64)
_LEN_EB = np.zeros(259, np.int64)
_LEN_EV = np.zeros(259, np.uint64)
_base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_ebits = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
for _s, (_b, _e) in enumerate(zip(_base, _ebits)):
    for _l in range(_b, min(_b + (1 << _e), 259)):
        if _l == 258 and _s != 28:
            continue
        _LEN_SYM[_l], _LEN_EB[_l], _LEN_EV[_l] = 257 + _s, _e, _l - _b


def row_bytes(fmt, W):
    return 1 + BPP[fmt] * W


def row_bound(fmt, W):
    """most bytes one scanline's two blocks take: book 0 is always a candidate, 9 bits per byte at the most"""
    return (9 * row_bytes(fmt, W) + 7) // 8 + 8


def _ok(fmt, n, W, H):
    return fmt in BPP and 1 <= n <= MAX_N and 1 <= W <= MAX_W and 1 <= H <= MAX_H


def stream_bound(fmt, W, H):
    return 2 + H * row_bound(fmt, W) + 9 if _ok(fmt, 1, W, H) else 0


def out_bytes(fmt, n, W, H):
    return n * ((stream_bound(fmt, W, H) + 15) & ~15) if _ok(fmt, n, W, H) else 0


def raw_rows(img, fmt):
    """[H][RL] uint8: filter byte 1, then the sub-filtered samples (gray16 big-endian, BGR8 as RGB)"""
    a = np.asarray(img)
    if fmt == GRAY16:
        h, w = a.shape
        rows = a.astype(np.uint16).astype(">u2").view(np.uint8).reshape(h, 2 * w)
    else:
        h, w, _ = a.shape
        rows = np.ascontiguousarray(a[..., ::-1]).reshape(h, 3 * w)
    bpp = BPP[fmt]
    raw = np.empty((h, 1 + bpp * w), np.uint8)
    raw[:, 0] = 1
    raw[:, 1:1 + bpp] = rows[:, :bpp]
    if w > 1:
        np.subtract(rows[:, bpp:], rows[:, :-bpp], out=raw[:, 1 + bpp:])
    return raw


def tokens(row, bpp):
    """-> (symbol [T], match length [T] (0 for a literal)) in stream order, without the end-of-block symbol"""
    RL = row.size
    idx = np.arange(RL)
    m = np.zeros(RL, bool)
    m[bpp:] = row[bpp:] == row[:-bpp]
    s = np.maximum.accumulate(np.where(~m, idx, -1)) + 1                 # run start: one past the nearest non-match at or before i
    e = np.minimum.accumulate(np.where(~m, idx, RL)[::-1])[::-1]         # run end: the nearest non-match at or after i
    L, k = e - s, idx - s
    full = (L // 258) * 258
    r = L - full
    m258 = m & (k < full) & (k % 258 == 0)
    mrem = m & (k == full) & (r >= 3)
    lit = ~m | (m & (k >= full) & (r < 3))
    start = lit | m258 | mrem
    length = np.where(m258, 258, np.where(mrem, r, 0))[start]
    sym = np.where(length > 0, _LEN_SYM[length], row[start].astype(np.int64))
    return sym, length


def _pack(values, nbits):
    """values[i] (uint64, below 2^nbits[i]) concatenated least significant bit first -> (uint8 bytes, bit count)"""
    nbits = np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    off = np.cumsum(nbits) - nbits
    j = np.arange(total) - np.repeat(off, nbits)
    bits = ((np.repeat(np.asarray(values, np.uint64), nbits) >> j.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little"), total


def book_costs(sym, length, bpp):
    """bits of the row's block under every book, extra bits left out (the same for all)"""
    hist = np.bincount(sym, minlength=286).astype(np.int64)
    hist[256] += 1
    nm = int((length > 0).sum())
    dlen = np.array([b["d_len"][bpp - 1] for b in BOOKS], np.int64)
    return _HDR_BITS + _LL_LEN @ hist + nm * dlen


def deflate_row(row, bpp, force_book=None):
    """one scanline -> (bytes of its two blocks, book index)"""
    sym, length = tokens(row, bpp)
    k = int(np.argmin(book_costs(sym, length, bpp))) if force_book is None else int(force_book)     # argmin: the first minimum
    b = BOOKS[k]
    code, clen = _LL_CODE[k][sym], _LL_LEN[k][sym]
    eb, ev = _LEN_EB[length], _LEN_EV[length]
    isn = length > 0
    dl = np.where(isn, b["d_len"][bpp - 1], 0)
    dc = np.where(isn, b["d_code"][bpp - 1], 0).astype(np.uint64)
    val = code | (ev << clen.astype(np.uint64)) | (dc << (clen + eb).astype(np.uint64))
    nb = clen + eb + dl
    hdr = [(b["hdr"] >> (32 * i)) & 0xFFFFFFFF for i in range((b["hdr_bits"] + 31) // 32)]
    hb = [32] * (b["hdr_bits"] // 32) + ([b["hdr_bits"] % 32] if b["hdr_bits"] % 32 else [])
    values = np.concatenate([np.array(hdr, np.uint64), val, np.array([b["ll_code"][256], 0], np.uint64)])
    nbits = np.concatenate([np.array(hb, np.int64), nb, np.array([b["ll_len"][256], 3], np.int64)])
    body, _ = _pack(values, nbits)
    return body.tobytes() + b"\x00\x00\xff\xff", k


def adler32(raw):
    return zlib.adler32(np.ascontiguousarray(raw).tobytes()) & 0xFFFFFFFF


def stream(img, fmt, force_book=None, want_books=False):
    """the zlib stream of one frame"""
    raw = raw_rows(img, fmt)
    parts, used = [b"\x78\x01"], []
    for row in raw:
        data, k = deflate_row(row, BPP[fmt], force_book)
        parts.append(data)
        used.append(k)
    parts.append(b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler32(raw)))
    s = b"".join(parts)
    return (s, used) if want_books else s


def batch(frames, fmt):
    """what v3d_png_deflate_batch leaves: (out uint8 [out_bytes], offsets uint64 [n + 1], [stream of frame f])"""
    n = len(frames)
    H, W = frames[0].shape[:2]
    streams = [stream(f, fmt) for f in frames]
    out = np.zeros(out_bytes(fmt, n, W, H), np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    pos = 0
    for f, s in enumerate(streams):
        out[pos:pos + len(s)] = np.frombuffer(s, np.uint8)
        pos += (len(s) + 15) & ~15
        offsets[f + 1] = pos
    return out, offsets, streams


def stream_end(out, lo, hi):
    """where the stream inside out[lo:hi] (hi a multiple of 16 past lo, zero-padded) ends.  The stream closes with
    01 00 00 FF FF and four Adler bytes and the padding is zero, so among the 16 candidate ends only the true one has the
    marker 9 bytes before it: a shifted marker would need its 01 on a 00 or FF of the true one, or an FF in the padding."""
    mark = bytes([1, 0, 0, 0xFF, 0xFF])
    for e in range(hi, max(hi - 16, lo + 10), -1):
        if bytes(out[e - 9:e - 4]) == mark:
            return e
    raise ValueError("no stream trailer in the last 16 bytes")


def png(stream_bytes, w, h, bit_depth, colour_type):
    """the file around a stream (the reference restatement of utils.png_from_stream)"""
    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, bit_depth, colour_type, 0, 0, 0))
            + chunk(b"IDAT", bytes(stream_bytes)) + chunk(b"IEND", b""))


# ------------------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and the GPU tests
# ------------------------------------------------------------------------------------------------------------------------
def image_from_residuals(res, fmt):
    """filtered bytes [H][bpp * W] (PNG order, without the filter byte) -> the image whose "sub" filter gives them"""
    bpp = BPP[fmt]
    h, w = res.shape[0], res.shape[1] // bpp
    px = np.cumsum(res.reshape(h, w, bpp), axis=1, dtype=np.uint8)
    if fmt == GRAY16:
        return (px[..., 0].astype(np.uint16) << 8) | px[..., 1]
    return np.ascontiguousarray(px[..., ::-1])


def book_residuals(k, fmt, W, rng):
    """one row of filtered bytes drawn from the model book k (>= 1) was built for: literals from its law (a mixture book
    peaked on the first byte of every sample and wide on the others), runs of equal samples for its share of matches"""
    _, b_peak, b_wide, pm = make_png_books.MODELS[k - 1]
    bpp = BPP[fmt]
    law = lambda b: np.array(make_png_books._law(b))
    res = rng.choice(256, size=(W, bpp), p=law(b_wide)).astype(np.uint8)
    if b_peak is not None:
        lanes = (0,) if fmt == GRAY16 else (0, 2)
        for c in lanes:
            res[:, c] = rng.choice(256, size=W, p=law(b_peak))
        if fmt == BGR8:
            res[:, 1] = np.where(rng.random(W) < 0.5, rng.choice(256, size=W, p=law(b_peak)), res[:, 1])
    if pm >= 0.1:                                                        # about pm of the tokens are matches: short gaps of
        x, gap = 0, max(1, int(round(1 / pm)) - 1)                       # literals between runs of equal samples
        while x < W:
            x += int(rng.integers(1, 2 * gap + 1))
            n = int(rng.integers(2, 6)) if rng.random() < 0.5 else -(-258 * int(rng.integers(1, 3)) // bpp)
            res[x:x + n] = 0
            x += n
    return res.reshape(-1)


def run_row(fmt, W, lengths, rng):
    """a noise row with runs of exactly the given numbers of matching bytes (a run of L matching bytes needs L + bpp equal-lane
    bytes: the residuals of L consecutive positions repeat the ones bpp before them), separated by noise"""
    bpp = BPP[fmt]
    res = rng.integers(0, 256, bpp * W).astype(np.uint8)
    pos = 1 + int(rng.integers(0, 5))
    for L in lengths:
        if pos + bpp + L + 1 >= res.size:
            break
        res[pos + bpp - 1] = res[pos - 1] ^ 0xAA                         # the run starts exactly behind this byte
        for i in range(pos + bpp, pos + bpp + L):
            res[i] = res[i - bpp]
        res[pos + bpp + L] = res[pos + L] ^ 0x55                         # and ends exactly here
        pos += bpp + L + 2 + int(rng.integers(0, 7))
    return res


RUN_LENGTHS = (2, 3, 257, 258, 259, 260, 261, 516, 517, 518)


def content_rows(fmt, W, H, seed):
    """H rows of filtered bytes cycling through the kinds the kernel can go wrong on"""
    rng = np.random.default_rng(seed)
    bpp = BPP[fmt]
    rows = []
    for y in range(H):
        kind = (y + seed) % 5
        if kind == 0:
            r = rng.integers(0, 256, bpp * W).astype(np.uint8)           # noise
        elif kind == 1:
            r = np.zeros(bpp * W, np.uint8)                              # a constant row: one run over the whole row
            r[:bpp] = rng.integers(0, 256, bpp)
        elif kind == 2:
            r = run_row(fmt, W, RUN_LENGTHS, rng)
        elif kind == 3:                                                  # runs whose ends fall on every thread border
            r = rng.integers(0, 256, bpp * W).astype(np.uint8)
            ppt = -(-(1 + bpp * W) // 256)
            for t in range(1, 256):
                e = t * ppt - 1 + (t % 3) - 1                            # payload index of a border, -1 / 0 / +1
                lo = max(e - 2 - (t % 7), bpp)
                if e < r.size and lo < e:
                    r[lo:e] = 0
        else:
            r = book_residuals(1 + (seed * 7 + y) % (K - 1), fmt, W, rng)
        rows.append(r)
    return np.stack(rows)


def content_image(fmt, W, H, seed):
    return image_from_residuals(content_rows(fmt, W, H, seed), fmt)


def seeded_depth(W=1920, H=96, seed=1):
    """a smoothed u16 depth map, min-max normalised like the depth CLI's output (the size measurement's first input)"""
    from scipy.ndimage import gaussian_filter
    d = gaussian_filter(np.random.default_rng(seed).random((H, W)), 25.0)
    return np.rint((d - d.min()) / (d.max() - d.min()) * 65535).astype(np.uint16)


def seeded_rgb(W=1920, H=48, seed=2):
    """a smooth colour image with sensor noise of sigma 1.5 grey levels, BGR u8 (the size measurement's second input)"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    a = gaussian_filter(rng.random((H, W, 3)), (8.0, 8.0, 0.0))
    a = (a - a.min()) / (a.max() - a.min()) * 255 + rng.normal(0.0, 1.5, a.shape)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def size_ratio(img, fmt):
    """bytes of the reference stream over zlib level 1 on the same payload"""
    return len(stream(img, fmt)) / len(zlib.compress(raw_rows(img, fmt).tobytes(), 1))
