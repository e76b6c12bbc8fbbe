"""Builds and runs the stand-alone emulator driver (tests/emu/): kernel sources of csrc/ compiled as plain C++ against
tests/emu/v3d_common.h, linked with tests/emu/harness.cpp and tests/emu/driver.cpp into a program of its own, once plain and once
with -fsanitize=address,undefined.  No sanitized code is loaded into python: a case travels through files in the test's temporary
directory.  Every case runs under CONFIGS: both workgroup orders, both thread orders between rendezvous, two LDS poisons, two
poisons of the bytes around the global buffers; the caller's expectations must hold in each."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "video-3d-pipeline_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
# workgroups descending, threads descending, LDS poison, global poison
CONFIGS = [(0, 0, 0xCD, 0xA5), (1, 1, 0x32, 0xFF)]
SMEM_DECL = re.compile(r"extern __shared__ [^;]*?\b(\w+)\[\];")      # the one dynamic LDS declaration of a file, whatever its name
EXT_VECTOR = re.compile(r"typedef uint32_t (\w+) __attribute__\(\(ext_vector_type\((\d)\), aligned\(4\)\)\);")
REPORT = re.compile(r"AddressSanitizer|runtime error|LeakSanitizer|emulator:")
_built = {}


def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one as well)"
    return cxx


HEADERS = ["v3d_wave.h", "v3d_png_books.h", "v3d_depth_math.h", "v3d_temporal_math.h", "v3d_temporal_internal.h", "v3d_sgbm_internal.h"]
SMEM_TEXT = r"unsigned char* const \1 = g_lds;"                # the harness allocates it per workgroup


def stage(d, kernels):
    """copies the kernel sources (as .cpp) and the headers they are compiled with next to the stand-in for v3d_common.h -> the
    .cpp paths.  An #include "v3d_common.h" then finds the stand-in.  The sources change in their dynamic LDS declaration only
    (kernel_source), the headers in what the loop below says"""
    for h in HEADERS:
        text = open(os.path.join(CSRC, h)).read()
        # clang's ext_vector_type does not exist in the host compiler: the typedefs that use it (v3d_sgbm_internal.h's two fetch types
        # of the cost volume, which no emulated source touches) become structs of the same members.  Nothing else of a header changes
        text = EXT_VECTOR.sub(lambda m: f"struct alignas(4) {m.group(1)} {{ uint32_t {', '.join('xyzw'[:int(m.group(2))])}; }};", text)
        assert "ext_vector_type" not in text, f"{h}: an ext_vector_type declaration did not match"
        with open(os.path.join(d, h), "w") as f:
            f.write(text)
    shutil.copy(os.path.join(EMU, "v3d_common.h"), os.path.join(d, "v3d_common.h"))
    out = []
    for k in kernels:
        out.append(os.path.join(d, os.path.splitext(k)[0] + ".cpp"))
        kernel_source(os.path.join(CSRC, k), out[-1], SMEM_TEXT)
    return out


def kernel_source(path, dst, smem_text):
    """copies a kernel source as .cpp with its one `extern __shared__ ... NAME[]` declaration (if it has one) replaced; smem_text
    is a replacement template, \\1 = NAME"""
    text = open(path).read()
    n = text.count("extern __shared__")
    assert n <= 1, f"{path}: {n} dynamic LDS declarations"
    text, done = SMEM_DECL.subn(smem_text, text)
    assert done == n, f"{path}: the dynamic LDS declaration did not match"
    with open(dst, "w") as f:
        f.write(text)


def sanitizer_link_error(d):
    """None if the host compiler links the sanitizer runtimes, else the linker's message"""
    if "san" not in _built:
        src = os.path.join(d, "probe.cpp")
        with open(src, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run([_cxx()] + SAN + ["-o", os.path.join(d, "probe"), src], capture_output=True, text=True)
        _built["san"] = None if r.returncode == 0 else (r.stderr.strip() or "the sanitizer runtimes do not link")
    return _built["san"]


def build(d, name, kernels, entries, header="v3d_hip.h", extra=(), sanitized=False):
    """-> path of the driver `name` for the kernel sources `kernels` (names under csrc/) and `extra` (paths), built in directory d"""
    key = (name, sanitized)
    if key in _built:
        return _built[key]
    d = os.path.join(str(d), name + ("_san" if sanitized else "_plain"))
    os.makedirs(d)
    srcs = stage(d, kernels)
    srcs += [os.path.join(EMU, "harness.cpp"), os.path.join(EMU, "driver.cpp")] + list(extra)
    flags = ["-O1", "-std=c++17", "-w", "-ffp-contract=off", "-I", d, "-I", EMU, "-I", os.path.join(ROOT, "include"),
             f'-DEMU_ENTRY_HEADER="{header}"', "-DEMU_ENTRIES=" + " ".join(f"E({e})" for e in entries)] + (SAN if sanitized else [])
    objs = [os.path.join(d, f"o{i}.o") for i in range(len(srcs))]

    def cc(i):
        return subprocess.run([_cxx()] + flags + ["-c", "-o", objs[i], srcs[i]], capture_output=True, text=True)
    with ThreadPoolExecutor(max_workers=4) as pool:
        for r in pool.map(cc, range(len(srcs))):
            assert r.returncode == 0, r.stderr[-4000:]
    exe = os.path.join(d, "driver")
    r = subprocess.run([_cxx()] + (SAN if sanitized else []) + ["-o", exe] + objs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    _built[key] = exe
    return exe


def driver_fixture(name, kernels, entries, **kw):
    """a module-scoped fixture, parametrised over the plain and the sanitized build of one driver"""
    @pytest.fixture(scope="module", params=["plain", "sanitized"])
    def driver(request, tmp_path_factory):
        d = tmp_path_factory.getbasetemp() / "emu_build"
        d.mkdir(exist_ok=True)
        san = request.param == "sanitized"
        if san:
            err = sanitizer_link_error(str(d))
            if err:
                pytest.skip("the host compiler cannot link the sanitizer runtimes: " + err[-300:])
        return build(d, name, kernels, entries, sanitized=san, **kw)
    return driver


def query(exe, entry, *ints):
    r = subprocess.run([exe, "query", entry] + [str(int(v)) for v in ints], capture_output=True, text=True)
    assert r.returncode == 0 and not REPORT.search(r.stderr), r.stderr[-4000:]
    return int(r.stdout)


class Buf:
    """One global buffer.  image: the bytes of the allocation (uint8).  The image sits at 256 k + skew and ends on the heap block's
    last byte.  expect: the image after the call (None: a workspace, anything goes; the default: unchanged, an input).
    chunk = (lo, hi): an input whose reader may load the aligned 16-byte blocks around its payload image[lo:hi]."""

    def __init__(self, name, image, skew=0, expect="same", chunk=None):
        self.name, self.image, self.skew, self.chunk = name, np.ascontiguousarray(image, np.uint8).reshape(-1), skew, chunk
        self.expect = self.image.copy() if isinstance(expect, str) else expect


def exact(name, payload, skew, **kw):
    """payload bytes at address 256 k + skew: the allocation starts on the payload's first byte when skew = 0 and ends on its last"""
    return Buf(name, payload, skew, **kw)


def chunked(name, payload, phase, poison):
    """payload at phase (0 .. 15) of a 16-byte block, inside exactly the 16-byte blocks that hold it, the slack poisoned
    -> (Buf, offset of the payload in it)"""
    payload = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    image = np.full((phase + payload.size + 15) // 16 * 16, poison, np.uint8)
    image[phase:phase + payload.size] = payload
    return Buf(name, image, 0, chunk=(phase, phase + payload.size)), phase


def run(exe, tmp, entry, args, config, rc=0):
    """args: ints, Bufs or (Buf, byte offset).  Runs one configuration, checks the exit, the reports, the counters and every
    buffer's expectation; -> {name: image after the call}"""
    wg, thr, lds_poison, gp = config
    bufs = {}
    lines = [f"entry {entry}", f"config {wg} {thr} {lds_poison} {gp}"]
    alines = []
    for a in args:
        b, off = a if isinstance(a, tuple) else (a, 0)
        if isinstance(b, Buf):
            bufs[b.name] = b
            alines.append(f"arg p {b.name} {off}")
        else:
            alines.append(f"arg v {int(b)}")
    for b in bufs.values():
        path = os.path.join(str(tmp), f"{b.name}.bin")
        b.image.tofile(path)
        lo, hi = b.chunk or (0, 0)
        lines.append(f"buf {b.name} {path} {b.image.size} {b.skew} {lo} {hi} {1 if b.chunk else 0}")
    case = os.path.join(str(tmp), "case.txt")
    with open(case, "w") as f:
        f.write("\n".join(lines + alines) + "\n")
    r = subprocess.run([exe, "run", case], capture_output=True, text=True)
    assert r.returncode == 0 and not REPORT.search(r.stderr), f"driver exit {r.returncode}\n{r.stdout[-500:]}\n{r.stderr[-6000:]}"
    got = dict(line.split() for line in r.stdout.strip().splitlines())
    assert int(got["rc"]) == rc, f"{entry} returned {got['rc']}: {r.stderr[-500:]}"
    assert int(got["misaligned"]) == 0, f"{got['misaligned']} 16-byte / 8-byte accesses off their alignment"
    assert int(got["nopayload"]) == 0, f"{got['nopayload']} 16-byte loads of a block that holds no payload"
    after = {}
    for b in bufs.values():
        raw = np.fromfile(os.path.join(str(tmp), f"{b.name}.bin.out"), np.uint8)
        assert raw.size == b.skew + b.image.size
        assert np.all(raw[:b.skew] == gp), f"{b.name}: a store in front of the buffer"
        img = raw[b.skew:]
        if b.expect is not None:
            bad = np.flatnonzero(img != b.expect)
            assert bad.size == 0, (f"{b.name}: {bad.size} bytes differ from what is expected, first at {int(bad[0])}: "
                                   f"{int(img[bad[0]])} for {int(b.expect[bad[0]])} (config {config})")
        after[b.name] = img
    return after


def run_configs(exe, tmp, entry, make, rc=0):
    """make(global poison) -> args; runs every configuration, side by side, each in a directory of its own -> the list of
    run()'s results"""
    def one(k):
        d = os.path.join(str(tmp), f"config{k}")
        os.makedirs(d, exist_ok=True)
        return run(exe, d, entry, make(CONFIGS[k][3]), CONFIGS[k], rc)
    with ThreadPoolExecutor(max_workers=len(CONFIGS)) as pool:
        return list(pool.map(one, range(len(CONFIGS))))
