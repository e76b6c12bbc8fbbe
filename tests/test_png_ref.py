"""The stream contract of the GPU PNG encoder, held on the CPU: tests/png_ref.py produces zlib streams that inflate to exactly
the payload utils.encode_png16 / encode_png8(bgr=True) hand to zlib, stay under the bound include/v3d_hip.h states, and wrap
into files Pillow and utils.read_png16 open to the original pixels.  Every code book is validated by forcing it on every
input (its header and every code it emits must inflate), and the seeded inputs make the free choice take every book.

The bound holds for the free choice only: it rests on book 0 being a candidate, and a forced dynamic book pays its header
(up to 66 bytes) even on a 3-byte row."""
import io
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import png_ref as P
from conftest import ROOT

FMTS = (P.GRAY16, P.BGR8)


def _host_raw(img, fmt):
    """the `raw` array of utils.encode_png16 / encode_png8(bgr=True), recovered from the file they write"""
    from video_3d_pipeline import utils
    data = utils.encode_png16(img) if fmt == P.GRAY16 else utils.encode_png8(img, bgr=True)
    pos, idat = 8, b""
    while pos < len(data):
        n, tag = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8]
        if tag == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return zlib.decompress(idat)


def _random(fmt, W, H, rng):
    return rng.integers(0, 65536, (H, W)).astype(np.uint16) if fmt == P.GRAY16 else rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _inputs():
    """name -> (fmt, image): the issue's list for both formats, plus one row pair per model book"""
    out = {}
    for fmt in FMTS:
        rng = np.random.default_rng(40 + fmt)
        t = "g16" if fmt == P.GRAY16 else "bgr"
        out[f"{t}-1x1"] = (fmt, _random(fmt, 1, 1, rng))
        out[f"{t}-zeros"] = (fmt, np.zeros_like(_random(fmt, 300, 3, rng)))
        out[f"{t}-noise"] = (fmt, _random(fmt, 333, 3, rng))
        every = np.tile(np.arange(256, dtype=np.uint8), 3 * P.BPP[fmt])[None, :].repeat(2, 0)
        every[1] = every[1, ::-1]
        out[f"{t}-every-byte"] = (fmt, P.image_from_residuals(every, fmt))
        runs = np.stack([P.run_row(fmt, 2000, P.RUN_LENGTHS[s:] + P.RUN_LENGTHS[:s], rng) for s in range(3)])
        out[f"{t}-runs"] = (fmt, P.image_from_residuals(runs, fmt))
        out[f"{t}-content"] = (fmt, P.content_image(fmt, 1001, 5, 3))
        for k in range(1, P.K):
            res = np.stack([P.book_residuals(k, fmt, 1500, np.random.default_rng(100 * fmt + k)) for _ in range(2)])
            out[f"{t}-book{k}"] = (fmt, P.image_from_residuals(res, fmt))
    return out


INPUTS = _inputs()


def test_run_rows_hold_the_runs_they_claim():
    """the run inputs contain maximal runs of exactly 2, 3, 257, 258, 259, 260, 261, 516, 517 and 518 matching bytes"""
    for fmt in FMTS:
        bpp = P.BPP[fmt]
        raw = P.raw_rows(INPUTS[("g16" if fmt == P.GRAY16 else "bgr") + "-runs"][1], fmt)
        found = set()
        for row in raw:
            m = np.zeros(row.size + 1, bool)
            m[bpp:-1] = row[bpp:] == row[:-bpp]
            edges = np.flatnonzero(m[1:] != m[:-1]) + 1
            if m[0]:
                edges = np.concatenate([[0], edges])
            found |= set((edges[1::2] - edges[0::2]).tolist())
        assert set(P.RUN_LENGTHS) <= found, sorted(set(P.RUN_LENGTHS) - found)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_stream_inflates_to_the_host_encoders_payload(name):
    fmt, img = INPUTS[name]
    H, W = img.shape[:2]
    want = _host_raw(img, fmt)
    assert want == P.raw_rows(img, fmt).tobytes()
    s = P.stream(img, fmt)
    assert s[:2] == b"\x78\x01" and zlib.decompress(s) == want
    assert len(s) <= P.stream_bound(fmt, W, H) == 2 + H * ((9 * (1 + P.BPP[fmt] * W) + 7) // 8 + 8) + 9
    assert len(s) <= len(P.stream(img, fmt, force_book=0)), "the free choice is never worse than book 0"
    for k in range(P.K):
        assert zlib.decompress(P.stream(img, fmt, force_book=k)) == want, f"book {k} ({P.BOOKS[k]['name']})"


def test_every_book_is_complete_and_the_free_choice_takes_each():
    assert 2 <= P.K <= 32
    for b in P.BOOKS:
        assert len(b["ll_len"]) == 286 and all(1 <= n <= 15 for n in b["ll_len"]) and b["d_len"][1] >= 1 and b["d_len"][2] >= 1
    assert P.BOOKS[0]["hdr_bits"] == 3
    picked = set()
    for fmt, img in INPUTS.values():
        picked |= set(P.stream(img, fmt, want_books=True)[1])
    assert picked == set(range(P.K)), f"never chosen: {sorted(set(range(P.K)) - picked)}"


def test_ties_go_to_the_lowest_index_and_rows_are_independent():
    fmt, img = INPUTS["g16-content"]
    whole = P.stream(img, fmt)
    rows = [P.deflate_row(r, 2)[0] for r in P.raw_rows(img, fmt)]
    assert whole[2:-9] == b"".join(rows)                            # a row's bytes do not depend on its neighbours
    sym, length = P.tokens(P.raw_rows(img, fmt)[0], 2)
    costs = P.book_costs(sym, length, 2)
    assert P.deflate_row(P.raw_rows(img, fmt)[0], 2)[1] == int(np.flatnonzero(costs == costs.min())[0])


def test_batch_layout_and_stream_end():
    frames = [P.content_image(P.BGR8, 85, 4, s) for s in range(3)]
    out, offsets, streams = P.batch(frames, P.BGR8)
    assert out.size == P.out_bytes(P.BGR8, 3, 85, 4) and offsets[0] == 0 and not (offsets % 16).any()
    for f, s in enumerate(streams):
        lo, hi = int(offsets[f]), int(offsets[f + 1])
        assert P.stream_end(out, lo, hi) == lo + len(s) and bytes(out[lo:lo + len(s)]) == s and not out[lo + len(s):hi].any()
    assert not out[int(offsets[3]):].any()
    assert P.out_bytes(7, 1, 4, 4) == 0 and P.out_bytes(0, 0, 4, 4) == 0 and P.stream_bound(0, 8193, 4) == 0 and P.stream_bound(1, 4, 65536) == 0


def test_stream_end_finds_every_padding():
    """utils.png_stream_end and png_ref.stream_end over all 16 paddings 0 .. 15 (stream sizes 16 k + 1 .. 16 k + 16), with Adler
    bytes that end in zeros or repeat the marker's own bytes, at a slot start and behind another stream"""
    from video_3d_pipeline import utils
    rng = np.random.default_rng(7)
    seen = set()
    for adler in (b"\x12\x34\x56\x78", b"\x00\x00\x00\x00", b"\x01\x00\x00\x00", b"\xff\xff\x01\x00", b"\x00\x01\x00\x00", b"\x00\xff\xff\x00"):
        for size in range(16, 49):
            body = rng.integers(0, 256, size - 11).astype(np.uint8).tobytes()
            s = b"\x78\x01" + body + b"\x01\x00\x00\xff\xff" + adler
            for lo in (0, 32):
                hi = lo + ((len(s) + 15) & ~15)
                buf = np.zeros(hi + 16, np.uint8)
                buf[:lo] = 0xFF
                buf[lo:lo + len(s)] = np.frombuffer(s, np.uint8)
                assert utils.png_stream_end(buf, lo, hi) == lo + len(s) == P.stream_end(buf, lo, hi), (adler, size, lo)
                seen.add(hi - lo - len(s))
    assert seen == set(range(16))


@pytest.mark.parametrize("name", ["g16-content", "g16-1x1", "bgr-content", "bgr-1x1"])
def test_wrapped_png_opens_to_the_original_pixels(name, tmp_path):
    from PIL import Image
    from video_3d_pipeline import utils
    fmt, img = INPUTS[name]
    H, W = img.shape[:2]
    data = utils.png_from_stream(P.stream(img, fmt), W, H, 16 if fmt == P.GRAY16 else 8, 0 if fmt == P.GRAY16 else 2)
    assert data == P.png(P.stream(img, fmt), W, H, 16 if fmt == P.GRAY16 else 8, 0 if fmt == P.GRAY16 else 2)
    with Image.open(io.BytesIO(data)) as im:
        got = np.asarray(im)
    if fmt == P.GRAY16:
        assert np.array_equal(got.astype(np.uint16), img)
        path = tmp_path / "a.png"
        path.write_bytes(data)
        assert np.array_equal(utils.read_png16(path), img)
        assert utils._decode_png16_fast(data) is not None            # filter "sub" on every row: the one-call path
    else:
        assert np.array_equal(got[..., ::-1], img)


def test_regenerating_the_books_reproduces_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_png_books.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    import make_png_books
    assert open(make_png_books.HEADER).read() == make_png_books.render()


# size of the reference stream over zlib level 1 on the same payload, as recorded in DESIGN.md section 4 ("GPU PNG encoding");
# 5 % for another zlib build's level-1 output
RECORDED = {"depth": 1.0892, "rgb": 0.8923}


def test_seeded_size_ratios_stay_at_the_recorded_ones():
    got = {"depth": P.size_ratio(P.seeded_depth(), P.GRAY16), "rgb": P.size_ratio(P.seeded_rgb(), P.BGR8)}
    print(got)
    for name, want in RECORDED.items():
        assert got[name] <= 1.05 * want, f"{name}: {got[name]:.4f} against the recorded {want:.4f}"
        assert got[name] >= want / 1.05, f"{name}: {got[name]:.4f} against the recorded {want:.4f}"
