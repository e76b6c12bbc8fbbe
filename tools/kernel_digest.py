#!/usr/bin/env python3
"""Digest of every kernel in gfx950 code objects: is a kernel's machine code what it was before a source change?

  hipcc <the csrc Makefile's CXXFLAGS> --cuda-device-only --no-gpu-bundle-output -c csrc/X.hip -o X.co   (one per source)
  tools/kernel_digest.py *.co > new.txt          one line per kernel: symbol, code bytes, sha256(code), sha256(descriptor)
  tools/kernel_digest.py --compare old.txt new.txt    exit 1 and name the kernels that differ, are missing or appear twice

Bytes 16-23 of the 64-byte kernel descriptor hold the code-entry offset, which depends on link order: cut out before hashing.
"""
import hashlib, os, re, subprocess, sys

READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def digest(path):
    text = subprocess.run([READELF, "-sW", "-SW", path], check=True, capture_output=True, text=True).stdout
    blob = open(path, "rb").read()
    secs = {int(m[1]): (int(m[2], 16), int(m[3], 16))         # index -> (address, file offset)
            for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", text, re.M)}
    syms = {}                                                   # name -> (type, value, size, section)
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]{16})\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", text, re.M):
        syms[m[5]] = (m[3], int(m[1], 16), int(m[2]), int(m[4]))
    def data(name):
        _, value, size, ndx = syms[name]
        off = value - secs[ndx][0] + secs[ndx][1]
        return blob[off:off + size]
    for name, (kind, _, size, _) in sorted(syms.items()):
        kd = syms.get(name + ".kd")
        if kind != "FUNC" or not kd or kd[2] != 64: continue
        d = data(name + ".kd")
        yield name, size, hashlib.sha256(data(name)).hexdigest(), hashlib.sha256(d[:16] + d[24:]).hexdigest()


def read_listing(path):
    rows = [line.split() for line in open(path) if line.strip()]
    names = [r[0] for r in rows]
    return {r[0]: tuple(r[1:]) for r in rows}, sorted({n for n in names if names.count(n) > 1})


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        (old, dup_o), (new, dup_n) = read_listing(sys.argv[2]), read_listing(sys.argv[3])
        bad = [f"twice: {n}" for n in dup_o + dup_n] + [f"only in {sys.argv[2]}: {n}" for n in sorted(old.keys() - new.keys())]
        bad += [f"only in {sys.argv[3]}: {n}" for n in sorted(new.keys() - old.keys())]
        bad += [f"differs: {n}" for n in sorted(old.keys() & new.keys()) if old[n] != new[n]]
        print("\n".join(bad) if bad else f"{len(new)} kernels, all identical")
        sys.exit(1 if bad else 0)
    for path in sys.argv[1:]:
        for row in digest(path): print(*row)
