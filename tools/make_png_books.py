#!/usr/bin/env python3
"""The constant Huffman code books of the GPU PNG encoder (include/v3d_hip.h, v3d_png_deflate_batch).

    python tools/make_png_books.py            # rewrites video-3d-pipeline_amd/csrc/v3d_png_books.h
    python tools/make_png_books.py --check    # exit status 1 if the committed file differs

Book 0 is deflate's fixed code (BTYPE 01).  Books 1 .. K-1 are dynamic codes (BTYPE 10) built here, once, from model
distributions of "sub"-filtered PNG bytes; the device never builds a code, it only picks the cheapest book per scanline.
Every book gives all 286 literal/length symbols a length in 1 .. 15 and codes the distances 2 and 3 (distance codes 1 and 2).

The models (frequencies in parts of 2^20, every symbol at least 1):
  literals   residual v (a byte, signed r = v or v - 256) from a two-sided geometric law exp(-|r| / b); a mixture book draws
             half its bytes from a law peaked at 0 (the high bytes of 16-bit samples) and half from a wide one (the low bytes);
  lengths    a share `pm` of all tokens, half of it on 258 (symbol 285: long constant runs), the rest falling off with the symbol;
  end of block / filter byte: one per scanline of about 4096 tokens.
Everything here is integer or correctly rounded float arithmetic on fixed inputs, then sorted with explicit tie-breaks: the
output does not depend on the platform.  tests/png_ref.py imports books() -- the C header is the same data, printed.
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "video-3d-pipeline_amd", "csrc", "v3d_png_books.h")

NSYM = 286                      # literal/length symbols 0 .. 285
NDIST = 3                       # distance codes 0 .. 2 (distances 1, 2, 3); code 0 is never used
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
INF = 1e30

# (name, b of the peaked half or None, b of the wide half, pm)
MODELS = (
    ("lap0.7", None, 0.7, 0.02), ("lap1.5", None, 1.5, 0.02), ("lap3", None, 3.0, 0.02), ("lap6", None, 6.0, 0.02),
    ("lap12", None, 12.0, 0.02), ("lap24", None, 24.0, 0.02), ("lap48", None, 48.0, 0.01), ("flat", None, INF, 0.002),
    ("mix0.3+2", 0.3, 2.0, 0.02), ("mix0.3+4", 0.3, 4.0, 0.02), ("mix0.3+8", 0.3, 8.0, 0.02), ("mix0.3+16", 0.3, 16.0, 0.02),
    ("mix0.3+32", 0.3, 32.0, 0.02), ("mix0.3+flat", 0.3, INF, 0.01),
    ("mix1+6", 1.0, 6.0, 0.02), ("mix1+12", 1.0, 12.0, 0.02), ("mix1+24", 1.0, 24.0, 0.02), ("mix1+flat", 1.0, INF, 0.01),
    ("runs+lap1", None, 1.0, 0.5), ("runs+mix0.3+8", 0.3, 8.0, 0.3),
)


def _law(b):
    w = [1.0 if b >= INF else math.exp(-min(v, 256 - v) / b) for v in range(256)]
    s = sum(w)
    return [x / s for x in w]


def model_freq(b_peak, b_wide, pm):
    """integer frequencies of the 286 symbols, parts of 2^20, each at least 1"""
    wide = _law(b_wide)
    lit = wide if b_peak is None else [0.5 * p + 0.5 * q for p, q in zip(_law(b_peak), wide)]
    ln = [0.5 ** (1 + (s - 257) / 4.0) for s in range(257, 285)] + [0.0]
    t = sum(ln)
    ln = [0.5 * x / t for x in ln[:-1]] + [0.5]
    f = [(1.0 - pm) * p for p in lit] + [1.0 / 4096] + [pm * x for x in ln]
    f[1] += 1.0 / 4096                                            # the filter-type byte
    return [max(1, int(round(x * (1 << 20)))) for x in f]


def huffman_lengths(freq, limit):
    """code lengths of a Huffman code for the symbols with freq > 0, no length above `limit`: the plain two-smallest merge
    (ties: the smaller frequency, then the subtree holding the smaller symbol), and while the deepest leaf is too deep the
    frequencies are flattened (f -> (f + 1) // 2) and the code rebuilt"""
    import heapq
    f = list(freq)
    while True:
        heap = [(w, s, (s,)) for s, w in enumerate(f) if w > 0]
        lens = [0] * len(f)
        if len(heap) == 1:
            lens[heap[0][1]] = 1
            return lens
        heapq.heapify(heap)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= limit:
            return lens
        f = [(w + 1) // 2 if w > 0 else 0 for w in f]


def canonical_codes(lens):
    """RFC 1951 3.2.2: code of every symbol (0 where the length is 0), most significant bit first"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lens:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def bit_reverse(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


class _Bits:
    """deflate's bit order: values least significant bit first, Huffman codes most significant bit first"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def huff(self, code, nbits):
        self.put(bit_reverse(code, nbits), nbits)


def _rle(lens):
    """the code-length sequence in the alphabet 0 .. 18 as (symbol, extra value, extra bits), greedy like zlib's scan_tree"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11, 7))
                run -= k
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3, 2))
                run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


def dynamic_header(ll_len, d_len):
    """BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code and both length sequences -> (bits as an int, bit count)"""
    seq = _rle(list(ll_len) + list(d_len))
    cl_freq = [0] * 19
    for s, _, _ in seq:
        cl_freq[s] += 1
    cl_len = huffman_lengths(cl_freq, 7)
    cl_code = canonical_codes(cl_len)
    hclen = 19
    while hclen > 4 and cl_len[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    b = _Bits()
    b.put(0, 1)
    b.put(2, 2)
    b.put(len(ll_len) - 257, 5)
    b.put(len(d_len) - 1, 5)
    b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cl_len[CL_ORDER[k]], 3)
    for s, ev, eb in seq:
        b.huff(cl_code[s], cl_len[s])
        b.put(ev, eb)
    return b.acc, b.n


def books():
    """[{name, ll_len[286], ll_code[286] (bit-reversed: emit least significant bit first), d_len[3], d_code[3], hdr (int), hdr_bits}]"""
    out = []
    fixed = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    out.append(_book("fixed", fixed, [5, 5, 5], 2, 3, fixed_dist=True))
    for name, bp, bw, pm in MODELS:
        ll = huffman_lengths(model_freq(bp, bw, pm), 15)
        d = [0, 1, 1]
        hdr, n = dynamic_header(ll, d)
        out.append(_book(name, ll, d, hdr, n))
    assert len(out) <= 32
    return out


def _book(name, ll_len, d_len, hdr, hdr_bits, fixed_dist=False):
    assert len(ll_len) == NSYM and all(1 <= n <= 15 for n in ll_len)
    if fixed_dist:
        ll_code = canonical_codes(ll_len + [8, 8])[:NSYM]         # the fixed code numbers 288 symbols
        d_code = [0, 1, 2]                                        # 5-bit codes, the value is the distance code
    else:
        ll_code = canonical_codes(ll_len)
        d_code = canonical_codes(d_len)
    return {"name": name, "ll_len": list(ll_len), "ll_code": [bit_reverse(c, n) for c, n in zip(ll_code, ll_len)],
            "d_len": list(d_len), "d_code": [bit_reverse(c, n) for c, n in zip(d_code, d_len)], "hdr": hdr, "hdr_bits": hdr_bits}


def render():
    bk = books()
    K = len(bk)
    words = max((b["hdr_bits"] + 31) // 32 for b in bk)
    L = ["// v3d_png_books.h -- GENERATED by tools/make_png_books.py: do not edit, regenerate.",
         "// The constant code books of v3d_png_deflate_batch (csrc/v3d_png.hip); tests/png_ref.py reads the same data from the tool.",
         "// ll[k][s]: (code length << 16) | code, the code bit-reversed so that it leaves least significant bit first;",
         "// dist[k][c]: the same for distance code c (distance c + 1); hdr[k]: the block header, hdr_bits[k] bits, as dwords.",
         "#pragma once",
         "#include <stdint.h>",
         f"#define V3D_PNG_BOOKS {K}",
         f"#define V3D_PNG_HDR_WORDS {words}",
         "static const char* const v3d_png_book_name[V3D_PNG_BOOKS] = {" + ", ".join('"%s"' % b["name"] for b in bk) + "};",
         "__device__ const uint32_t v3d_png_ll[V3D_PNG_BOOKS][286] = {"]
    for b in bk:
        v = [(n << 16) | c for c, n in zip(b["ll_code"], b["ll_len"])]
        L.append("  { // " + b["name"])
        for i in range(0, NSYM, 13):
            L.append("    " + ", ".join("0x%05x" % x for x in v[i:i + 13]) + ",")
        L.append("  },")
    L.append("};")
    L.append("__device__ const uint32_t v3d_png_dist[V3D_PNG_BOOKS][3] = {")
    for b in bk:
        L.append("  {" + ", ".join("0x%05x" % ((n << 16) | c) for c, n in zip(b["d_code"], b["d_len"])) + "},")
    L.append("};")
    L.append("__device__ const uint32_t v3d_png_hdr_bits[V3D_PNG_BOOKS] = {" + ", ".join(str(b["hdr_bits"]) for b in bk) + "};")
    L.append("__device__ const uint32_t v3d_png_hdr[V3D_PNG_BOOKS][V3D_PNG_HDR_WORDS] = {")
    for b in bk:
        w = [(b["hdr"] >> (32 * i)) & 0xFFFFFFFF for i in range(words)]
        L.append("  {" + ", ".join("0x%08x" % x for x in w) + "},")
    L.append("};")
    return "\n".join(L) + "\n"


def main(argv):
    text = render()
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("v3d_png_books.h is up to date" if same else "v3d_png_books.h differs from the generator's output")
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    bk = books()
    print(f"{HEADER}: {len(bk)} books, headers {min(b['hdr_bits'] for b in bk[1:])} .. {max(b['hdr_bits'] for b in bk)} bits")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
