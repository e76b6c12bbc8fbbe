"""csrc/v3d_depth_math.h on the host: the header is plain C11, so it is compiled here with the oracle Makefile's compiler and flags
into a small shared library and held, bit for bit, to the NumPy contracts the GPU entries are held to (tests/temporal_ref.py,
numpy.rint) and to the oracle's own save_depth_map.  No GPU, no native library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-3d-pipeline_amd", "csrc")

SHIM = r"""
#include <stddef.h>
#include "v3d_depth_math.h"
void shim_norm_u16(const float* d, size_t n, float lo, float hi, uint16_t* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_norm_u16(d[i], lo, hi); }
void shim_d16(const float* d, size_t n, float* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_d16(d[i]); }
void shim_d16_tap(const float* d, size_t n, int32_t* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_d16_tap(d[i]); }
void shim_rint_u16(const float* d, size_t n, uint16_t* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_rint_u16(d[i]); }
void shim_f2ord(const float* d, size_t n, uint32_t* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_f2ord(d[i]); }
void shim_ord2f(const uint32_t* o, size_t n, float* out) { for (size_t i = 0; i < n; i++) out[i] = v3d_ord2f(o[i]); }
"""


def _make_var(text, name):
    m = re.search(rf"^{name}\s*\??=\s*(.+)$", text, re.M)
    assert m, f"oracle/Makefile sets no {name}"
    return m.group(1).split()


@pytest.fixture(scope="module")
def dm(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("depth_math")
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    src, so = tmp_path / "shim.c", tmp_path / "libdepthmath.so"
    src.write_text(SHIM)
    subprocess.check_call(_make_var(mk, "CC") + _make_var(mk, "CFLAGS") + ["-Werror", "-I", CSRC, "-shared", "-o", str(so), str(src), "-lm"])
    lib = C.CDLL(str(so))

    def run(fn, a, in_t, out_t, *scalars):
        a = np.ascontiguousarray(a, in_t).ravel()
        out = np.empty(a.shape, out_t)
        getattr(lib, fn)(C.c_void_p(a.ctypes.data), C.c_size_t(a.size), *[C.c_float(float(s)) for s in scalars], C.c_void_p(out.ctypes.data))
        return out

    class M:
        norm_u16 = staticmethod(lambda d, lo, hi: run("shim_norm_u16", d, np.float32, np.uint16, lo, hi))
        d16 = staticmethod(lambda d: run("shim_d16", d, np.float32, np.float32))
        d16_tap = staticmethod(lambda d: run("shim_d16_tap", d, np.float32, np.int32))
        rint_u16 = staticmethod(lambda d: run("shim_rint_u16", d, np.float32, np.uint16))
        f2ord = staticmethod(lambda d: run("shim_f2ord", d, np.float32, np.uint32))
        ord2f = staticmethod(lambda o: run("shim_ord2f", o, np.uint32, np.float32))
    return M


def test_header_stands_alone_in_plain_c(tmp_path):
    """the header by itself, with nothing included before it, is a C11 translation unit"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    (tmp_path / "alone.c").write_text('#include "v3d_depth_math.h"\n')
    subprocess.check_call(_make_var(mk, "CC") + _make_var(mk, "CFLAGS") + ["-Werror", "-I", CSRC, "-c", str(tmp_path / "alone.c"),
                          "-o", str(tmp_path / "alone.o")])
    text = open(os.path.join(CSRC, "v3d_depth_math.h")).read()
    assert sorted(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == ["math.h", "stdint.h", "string.h"]


def _want_norm(d, lo, hi):
    with np.errstate(over="ignore"):                      # a one-ulp range at zero: the quotient is inf, the clamp takes it
        return TR.to_u16_range(np.asarray(d, np.float32)[None], np.float32([[lo, hi]]))[0]


def test_norm_u16_equals_the_numpy_contract(dm, oracle):
    rng = np.random.default_rng(1)
    d = rng.uniform(-10.0, 80.0, 200000).astype(np.float32)
    d16 = (rng.integers(-64, 1200, 50000) / 16.0).astype(np.float32)
    up = np.nextafter(np.float32(7.25), np.float32(np.inf))
    for what, x, lo, hi in (
            ("below, inside and above", d, 2.5, 61.75),
            ("below, inside and above, fixed point", d16, 1.0625, 40.5),
            ("negative lo", d, -3.7, 55.3),
            ("flat", d, 7.25, 7.25),
            ("flat at zero", d16, 0.0, 0.0),
            ("unordered", d, 9.0, 3.0),
            ("one ulp wide", np.float32([7.0, 7.25, up, 7.5, -1.0, 100.0]), 7.25, up),
            ("one ulp wide at zero", np.float32([-1.0, -0.0, 0.0, 1e-45, 2e-45, 1.0]), 0.0, 1e-45),
            ("near flat", d, 20.0, np.nextafter(np.float32(20.0), np.float32(np.inf)))):
        got, want = dm.norm_u16(x, lo, hi), _want_norm(x, lo, hi)
        assert np.array_equal(got, want), f"{what}: {np.flatnonzero(got != want)[:4]}"
    # the frame's own range: the contract and the oracle's save_depth_map (which has no clamp: none is needed there)
    for x in (d, d16, np.abs(d), np.float32([3.0, 3.0, 3.0]), np.float32([5.5])):
        lo, hi = x.min(), x.max()
        got = dm.norm_u16(x, lo, hi)
        assert np.array_equal(got, _want_norm(x, lo, hi))
        assert np.array_equal(got, oracle.depth_to_u16(x))
        if hi > lo:
            assert got.min() == 0 and got.max() == 65535
    # NaN -> 0, in the sample and in the range
    assert not dm.norm_u16(np.float32([np.nan]), 0.0, 1.0).any()
    assert not dm.norm_u16(d[:64], np.nan, 1.0).any() and not dm.norm_u16(d[:64], 0.0, np.nan).any()


def test_d16_equals_the_numpy_contract(dm):
    rng = np.random.default_rng(2)
    for x in ((np.arange(-64, 40000) / 16.0).astype(np.float32),                 # multiples of 1/16: exact
              rng.uniform(-5.0, 2100.0, 500000).astype(np.float32),
              (np.arange(-200, 70001) / 32.0).astype(np.float32)):              # every half-way case k/32: ties go to even
        got = dm.d16(x)
        assert np.array_equal(got, np.rint(got))
        assert np.array_equal(got.view(np.uint32), np.rint(x * np.float32(16)).view(np.uint32))   # the float itself, negatives included
        assert np.array_equal(np.clip(got, 0, TR.D16_MAX).astype(np.int64), TR.d16_of(x))         # finite values only: the cast is defined
        assert np.array_equal(dm.d16_tap(x), TR.d16_of(x))
    assert np.isnan(dm.d16(np.float32([np.nan]))[0])


def _ladder():
    """every class of float32: NaNs of both signs and several payloads, infinities, the largest and smallest normals, denormals,
    both zeros, and rint(16 D) exactly at 0.5, 1, 1.5, 2.5, 2046, 2047, 32766.5, 32767, 32767.5, 32768, 2^31, 2^63 and FLT_MAX"""
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    sub_lo, sub_hi = np.float32(1e-45), np.nextafter(fmin, np.float32(0))
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float32)
    pos = np.float32([0.0, sub_lo, sub_hi, fmin, 1 / 64, 1 / 32, np.nextafter(np.float32(1 / 32), np.float32(1)), 1 / 16, 3 / 32, 5 / 32,
                      1.0, 2046 / 16, 2047 / 16, 2048 / 16, 32766.5 / 16, 2047.9375, 32767.5 / 16, 2048.0, 4096.0, 1e9, 2.0 ** 27,
                      np.nextafter(np.float32(2.0 ** 27), np.float32(0)), 2.0 ** 28, 2.0 ** 59, 2.0 ** 60, 1e30, fmax / 16, fmax, np.inf])
    return np.concatenate([nans, pos, -pos])


def test_d16_tap_decides_in_float_and_saturates(dm):
    """v3d_d16_tap against its NumPy statement (tests/temporal_ref.py d16_of and its one-sample twin) on every class of float"""
    x = _ladder()
    got = dm.d16_tap(x)
    assert np.array_equal(got, TR.d16_of(x)), (x[got != TR.d16_of(x)], got[got != TR.d16_of(x)])
    assert got.tolist() == [TR.d16_loop(v) for v in x]
    at = lambda v: int(dm.d16_tap(np.float32([v]))[0])                      # noqa: E731
    # rint(16 D) = 0.5 -> 0 (tie to even: invalid), 1, 32767, 32767.5 -> 32768 -> saturated, 32768, 2^31, 2^63, FLT_MAX
    assert [at(0.5 / 16), at(1 / 16), at(2047.9375), at(32767.5 / 16), at(2048.0), at(2.0 ** 27), at(2.0 ** 59), at(np.finfo(np.float32).max)] \
        == [0, 1, 32767, 32767, 32767, 32767, 32767, 32767]
    assert at(np.inf) == 32767 and at(-np.inf) == at(np.nan) == at(-np.nan) == at(-0.0) == at(1e-45) == at(-1e30) == 0
    assert at(32766.5 / 16) == 32766 and at(32766 / 16) == 32766            # the last tie below the range goes to even
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, 1000000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    assert np.array_equal(dm.d16_tap(bits), TR.d16_of(bits))
    assert got.min() == 0 and got.max() == TR.D16_MAX


SANITISED = r"""
#include <stdio.h>
#include "v3d_depth_math.h"
static float bits(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }
int main(void)
{
    float x[128];
    int n = 0;
    const uint32_t nan[] = { 0x7FC00000u, 0xFFC00000u, 0x7F800001u, 0xFF800001u, 0x7FFFFFFFu, 0xFFFFFFFFu };
    const float pos[] = { 0.0f, 1e-45f, 1.17549421e-38f, 1.17549435e-38f, 0.015625f, 0.03125f, 0.0625f, 0.09375f, 1.0f, 127.9375f, 128.0f,
                          2047.90625f, 2047.9375f, 2047.96875f, 2048.0f, 4095.96875f, 4096.0f, 65534.5f, 65535.0f, 65535.5f, 65536.0f,
                          1e9f, 134217728.0f, 2147483648.0f, 4294967296.0f, 5.76460752e17f, 9.22337204e18f, 1e30f, 3.40282347e38f, INFINITY };
    for (size_t i = 0; i < sizeof nan / sizeof *nan; i++) x[n++] = bits(nan[i]);
    for (size_t i = 0; i < sizeof pos / sizeof *pos; i++) { x[n++] = pos[i]; x[n++] = -pos[i]; }
    unsigned long long sum = 0;
    for (int i = 0; i < n; i++) {
#ifdef BARE_CAST
        sum += (unsigned)(int)v3d_d16(x[i]);                /* the conversion the helper replaces: the control of the test */
#else
        sum += (unsigned)v3d_d16_tap(x[i]);
#endif
        sum += v3d_rint_u16(x[i]);
        for (int a = 0; a < n; a++)
            for (int b = 0; b < n; b++) sum += v3d_norm_u16(x[i], x[a], x[b]);
    }
    printf("%d values, checksum %llu\n", n, sum);
    return 0;
}
"""


def test_no_out_of_range_conversion_under_the_sanitiser(tmp_path):
    """a stand-alone C program, built with -fsanitize=undefined,float-cast-overflow and run as a fresh child process (the test adds
    nothing to its environment), calls v3d_d16_tap, v3d_rint_u16 and v3d_norm_u16 (sample x lo x hi) on every class of float: no conversion of a
    value its integer type cannot hold remains in the shared arithmetic.  The same program with the bare (int)v3d_d16(x) in the
    helper's place must be caught: the control that the build really checks conversions."""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    (tmp_path / "ladder.c").write_text(SANITISED)
    flags = _make_var(mk, "CFLAGS") + ["-Werror", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-I", CSRC]
    for define, clean in (([], True), (["-DBARE_CAST"], False)):
        exe = tmp_path / ("ladder" + ("" if clean else "_bare"))
        subprocess.check_call(_make_var(mk, "CC") + flags + define + ["-o", str(exe), str(tmp_path / "ladder.c"), "-lm"])
        p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        if clean:
            assert p.returncode == 0 and "runtime error" not in p.stderr and "checksum" in p.stdout, p.stderr[-2000:]
        else:
            assert p.returncode != 0 and "outside the range of representable values" in p.stderr, (p.returncode, p.stderr[-500:])


def test_rint_u16_equals_numpy_rint_and_clip(dm):
    rng = np.random.default_rng(3)
    edge = np.float32([0.5, -0.5, 1.5, 2.5, 3.5, -1.5, 0.0, -0.0, 0.49999997, 65534.5, 65535.5, 65534.49, 65535.0, 65536.0, 65535.49,
                       -3.2, -1e9, 1e9, 3.4e38, -3.4e38, np.inf, -np.inf])
    x = np.concatenate([edge, rng.uniform(-10.0, 70000.0, 500000).astype(np.float32), (np.arange(-8, 131080) / 2.0).astype(np.float32)])
    assert np.array_equal(dm.rint_u16(x), np.clip(np.rint(x), 0, 65535).astype(np.uint16))
    assert dm.rint_u16(np.float32([np.nan]))[0] == 0


def test_ordered_codec_round_trips_and_sorts_like_the_floats(dm):
    rng = np.random.default_rng(4)
    fmax, fmin = np.finfo(np.float32).max, np.finfo(np.float32).tiny
    sub_lo, sub_hi = np.float32(1e-45), np.nextafter(fmin, np.float32(0))
    ladder = np.float32([-np.inf, -fmax, -1.0, -fmin, -sub_hi, -sub_lo, -0.0, 0.0, sub_lo, sub_hi, fmin, 1.0, fmax, np.inf])
    o = dm.f2ord(ladder)
    assert (np.diff(o.astype(np.int64)) > 0).all(), o                          # strictly increasing, -0 below +0
    assert np.array_equal(dm.ord2f(o).view(np.uint32), ladder.view(np.uint32))
    assert o.min() > 0 and o.max() < 0xFFFFFFFF                                # the empty slot {0xFFFFFFFF, 0} is no finite float or inf
    bits = rng.integers(0, 1 << 32, 1000000, dtype=np.uint64).astype(np.uint32)    # every kind of float, NaNs included
    x = bits.view(np.float32)
    ox = dm.f2ord(x)
    assert np.array_equal(dm.ord2f(ox).view(np.uint32), bits)
    a, b, oa, ob = x[::2], x[1::2], ox[::2], ox[1::2]
    ok = ~(np.isnan(a) | np.isnan(b))
    assert np.array_equal((a < b)[ok], (oa < ob)[ok] & (a != b)[ok])            # +-0 compare equal as floats, ordered as codes
    assert np.array_equal((a > b)[ok], (oa > ob)[ok] & (a != b)[ok])
