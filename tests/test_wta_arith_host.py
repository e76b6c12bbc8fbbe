"""The two division-free helpers of the winner-take-all tail (csrc/v3d_common.h: v3d_t1_magic / v3d_t1_ceil and
v3d_subpix_q) against exact integer division.  No GPU, no native library.

The functions below RESTATE the helpers line by line in NumPy integer arithmetic (uint32 wrap-around and the 24-bit
operand masks included); v3d_common.h and this file must stay the same few lines -- whoever changes one changes the
other.  What they replace in wta_pixel (v3d_sgbm_paths.hip), and what is the reference here:

    T1 = uq > 0 ? (minS * 100 + uq - 1) / uq : (minS * 100 > 0 ? 32768 : 0);  T1 = min(T1, 32768)     uq = 100 - uniquenessRatio
    den = max(sm + sp - 2 * minS, 1);  d16 += ((sm - sp) * 16 + den) / (den * 2)                         C division: truncates toward 0

Ranges: minS, sm, sp are aggregated costs in [0, 32767] with sm, sp >= minS (minS is the row's minimum)."""
import numpy as np
import pytest


# ---- restatement of v3d_common.h ----
def t1_magic(uq):
    c = 0
    while (1 << c) < uq:
        c += 1
    shift = 23 + c
    mul = ((1 << shift) + uq - 1) // uq                       # the host's one division, per handle
    assert mul < 1 << 32
    return mul, shift


def t1_ceil(minS, uq, mul, shift):
    n = (minS.astype(np.uint64) * np.uint64(100) + np.uint64(uq - 1)) & np.uint64(0xFFFFFF)
    return ((n * np.uint64(mul & 0xFFFFFF)) >> np.uint64(shift)).astype(np.int64)


def subpix_q(a, b):
    den = np.maximum(a + b, 1)
    num = (a - b) * 16 + den
    step = ((1 - 32 * den) & 0xFFFFFFFF).astype(np.uint32)
    R = ((np.abs(num) << 4) & 0xFFFFFFFF).astype(np.uint32)
    for bit in (3, 2, 1, 0):
        t = R + (step << np.uint32(bit))                     # uint32: wraps
        R = np.where(t < R, t, R)
    qm = (R & np.uint32(15)).astype(np.int64)
    return np.where(num < 0, -qm, qm)


# ---- restatement of the two lines of wta_pixel that use v3d_t1_ceil ----
def wta_t1(minS, uniq):
    uq = 100 - uniq
    if uq > 0:
        mul, shift = t1_magic(uq)                             # v3d_sgbm_create
        t1 = t1_ceil(minS, uq, mul, shift)
    else:
        t1 = np.minimum(minS, 1) << 15
    return np.minimum(t1, 32768)


def subpix_exact(a, b):
    den = np.maximum(a + b, 1)
    num = (a - b) * 16 + den
    return np.sign(num) * (np.abs(num) // (2 * den))          # truncation toward zero


@pytest.mark.parametrize("uniq", range(0, 101))
def test_t1_every_min_cost_and_ratio(uniq):
    minS = np.arange(32768, dtype=np.int64)
    uq, thr = 100 - uniq, minS * 100
    want = (thr + uq - 1) // uq if uq > 0 else np.where(thr > 0, 32768, 0)
    want = np.minimum(want, 32768)
    got = wta_t1(minS, uniq)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"uniquenessRatio {uniq}: minS {bad[:5]} -> {got[bad[:5]]} instead of {want[bad[:5]]}"
    if uq > 0:                                                # the uncapped quotient too, and the operand widths the kernel relies on
        mul, shift = t1_magic(uq)
        assert (1 << 23) <= mul < (1 << 24) and int(thr.max()) + uq - 1 < (1 << 22)
        assert np.array_equal(t1_ceil(minS, uq, mul, shift), (thr + uq - 1) // uq)


def test_subpixel_term_exhaustive_small_range():
    b = np.arange(2048, dtype=np.int64)
    for a0 in range(0, 2048, 256):                            # 8 slabs of 256 x 2048 pairs: every (a, b) in [0, 2047]^2
        a = np.arange(a0, a0 + 256, dtype=np.int64)[:, None] + 0 * b[None, :]
        bb = b[None, :] + 0 * a
        got, want = subpix_q(a, bb), subpix_exact(a, bb)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"(a, b) = {(a[tuple(bad[0])], bb[tuple(bad[0])])}: {got[tuple(bad[0])]} instead of {want[tuple(bad[0])]}"
        assert np.abs(got).max() <= 8


def test_subpixel_term_random_full_range():
    rng = np.random.default_rng(20240607)
    a = rng.integers(0, 32767, size=10_000_000, dtype=np.int64)        # 0 .. 32766
    b = rng.integers(0, 32767, size=10_000_000, dtype=np.int64)
    # the corners a uniform draw all but never hits
    edge = np.array([0, 1, 2, 32765, 32766], dtype=np.int64)
    a = np.concatenate([a, np.repeat(edge, edge.size)])
    b = np.concatenate([b, np.tile(edge, edge.size)])
    got, want = subpix_q(a, b), subpix_exact(a, b)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"(a, b) = {(a[bad[0]], b[bad[0]])}: {got[bad[0]]} instead of {want[bad[0]]}"
    assert got.min() >= -7 and got.max() <= 8
