"""The special float32 values the non-finite tests feed every float entry, and where they put them.  Test infrastructure shared by
the CPU tests of the restatements and tests/test_nonfinite_gpu.py."""
import contextlib
import warnings

import numpy as np

FLT_MAX = np.finfo(np.float32).max
SPECIALS = {
    "nan+": np.array([0x7FC00000], np.uint32).view(np.float32)[0],          # sign bit clear
    "nan-": np.array([0xFFC00000], np.uint32).view(np.float32)[0],          # sign bit set: x86's default NaN of inf - inf
    "+inf": np.float32(np.inf),
    "-inf": np.float32(-np.inf),
    "-0.0": np.float32(-0.0),
    "denormal": np.float32(1e-45),
    "FLT_MAX": FLT_MAX,
    "2048": np.float32(2048.0),                                             # rint(16 D) = 32768: the first value above the fixed point
    "2047.9375": np.float32(2047.9375),                                     # 32767: the last one inside
    "1e9": np.float32(1e9),
}
NAMES = tuple(SPECIALS)


def positions(n):
    """flat indices of a frame of n elements: element 0, the last element of the first 16-byte group, the first element past
    one, the last element (deduplicated, inside the frame)"""
    return sorted({i for i in (0, 3, 4, n - 1) if 0 <= i < n})


def placements(n):
    """(label, {flat index: value}) cases for a frame of n elements: every special alone at every position, all specials
    together spread over the positions, and a frame made only of specials"""
    pos = positions(n)
    for name, v in SPECIALS.items():
        for p in pos:
            yield f"{name}@{p}", {p: v}
    vals = list(SPECIALS.values())
    yield "all together", {(pos[k % len(pos)] + k // len(pos)) % n: vals[k] for k in range(len(vals))}
    yield "only specials", {i: vals[i % len(vals)] for i in range(n)}


def put(frame, where):
    """a copy of `frame` with the {flat index: value} of a placement written in (bit patterns kept)"""
    out = np.array(frame, np.float32, copy=True)
    flat = out.reshape(-1)
    for i, v in where.items():
        flat[i] = v
    return out


def same_floats(a, b):
    """equal as bit patterns, modulo "is NaN" (any NaN equals any NaN)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


@contextlib.contextmanager
def cast_warnings_are_errors():
    """NumPy's "invalid value encountered in cast" (an astype of a NaN, an infinity or an out-of-range float) fails the test"""
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*invalid value encountered in cast.*")
        yield
