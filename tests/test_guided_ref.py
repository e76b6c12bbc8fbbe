"""CPU: the float64 oracle of the guided filter against exact rational arithmetic, and the error bound of tests/gf_ref.py.

The GPU accuracy tests hold every kernel to |q - oracle| <= ulp32 + F.  That bar means something only if the oracle itself is
far closer to the exact result than F: here the oracle's error, measured against fractions.Fraction on tiny images, must stay
below F / 10 and below the oracle's own share of F."""
import math
from fractions import Fraction

import numpy as np
import pytest

import gf_ref


def _exact_guided(depth_lo, guide, r, eps):
    """the guided filter in exact rationals: bilinear weights from the float64 source coordinates the kernels and the oracle
    compute, I = g / 255, eps as the float32 the C ABI carries, clipped windows divided by their true count"""
    Hlo, Wlo = depth_lo.shape
    H, W = guide.shape
    sx, sy = Wlo / W, Hlo / H                                # float64, as in both implementations

    def taps(x, s, n):
        f = (x + 0.5) * s - 0.5
        f0 = math.floor(f)
        w = Fraction(f) - f0
        return min(max(f0, 0), n - 1), min(max(f0 + 1, 0), n - 1), w

    D = [[Fraction(float(v)) for v in row] for row in depth_lo]
    tx = [taps(x, sx, Wlo) for x in range(W)]
    p = []
    for y in range(H):
        ya, yb, wy = taps(y, sy, Hlo)
        row = []
        for (xa, xb, wx) in tx:
            top = D[ya][xa] * (1 - wx) + D[ya][xb] * wx
            bot = D[yb][xa] * (1 - wx) + D[yb][xb] * wx
            row.append(top * (1 - wy) + bot * wy)
        p.append(row)
    I = [[Fraction(int(g), 255) for g in row] for row in guide]

    def box(a):
        hs = [[sum(a[y][max(x - r, 0):min(x + r, W - 1) + 1], Fraction(0)) for x in range(W)] for y in range(H)]
        out = []
        for y in range(H):
            y0, y1 = max(y - r, 0), min(y + r, H - 1)
            out.append([sum((hs[j][x] for j in range(y0, y1 + 1)), Fraction(0))
                        / ((y1 - y0 + 1) * (min(x + r, W - 1) - max(x - r, 0) + 1)) for x in range(W)])
        return out

    e = Fraction(gf_ref.eps32(eps))
    mI, mp = box(I), box(p)
    mIp = box([[I[y][x] * p[y][x] for x in range(W)] for y in range(H)])
    mII = box([[I[y][x] * I[y][x] for x in range(W)] for y in range(H)])
    a = [[(mIp[y][x] - mI[y][x] * mp[y][x]) / (mII[y][x] - mI[y][x] ** 2 + e) for x in range(W)] for y in range(H)]
    b = [[mp[y][x] - a[y][x] * mI[y][x] for x in range(W)] for y in range(H)]
    ma, mb = box(a), box(b)
    return np.array([[float(ma[y][x] * I[y][x] + mb[y][x]) for x in range(W)] for y in range(H)])


def _tiny(seed, Wlo, Hlo, W, H, flat=False):
    rng = np.random.default_rng(seed)
    depth = (rng.uniform(0, 60, (Hlo, Wlo)) * (rng.random((Hlo, Wlo)) > 0.2)).astype(np.float32)
    guide = rng.integers(0, 256, (H, W)).astype(np.uint8)
    if flat:                                                 # flat guide patches: var = 0, the 1/eps amplification
        guide[: H // 2, : W // 2] = 200
        guide[H // 2:, W // 2:] = 201
    return depth, guide


# 9x7 .. 14x10 guides, r = 1..4, scales 2x, non-integer, identity and down; eps from 1e-6 to 1
@pytest.mark.parametrize("Wlo,Hlo,W,H,r,eps,flat", [(5, 4, 9, 7, 1, 1e-3, False), (6, 5, 11, 8, 2, 1e-6, True),
                                                     (13, 9, 13, 9, 3, 1e-3, True), (7, 5, 14, 10, 4, 1e-3, False),
                                                     (17, 12, 12, 9, 2, 1e-1, False), (4, 3, 10, 10, 1, 1.0, True)])
def test_oracle_against_exact_rationals(oracle, Wlo, Hlo, W, H, r, eps, flat):
    depth, guide = _tiny(W * 31 + H + r, Wlo, Hlo, W, H, flat)
    exact = _exact_guided(depth, guide, r, eps)
    got = gf_ref.reference(depth, guide, r, eps)
    kern, orc = gf_ref.floor(depth, guide, r, eps, parts=True)
    err = np.abs(got - exact)
    F = kern + orc
    assert (err <= orc).all(), f"oracle error {err.max():.3e} above its own share of F (min {orc.min():.3e})"
    assert (err <= F / 10).all(), f"oracle error / F = {(err / F).max():.3g}"
    # the float32 route's bound is then carried by the kernel: the oracle uses at most a small part of it
    assert (err / F).max() < 0.1


def test_eps_is_fed_as_float32():
    assert gf_ref.eps32(1e-3) == float(np.float32(1e-3)) != 1e-3
    assert abs(gf_ref.eps32(1e-3) / 1e-3 - 1) > 4e-8


def test_floor_grows_where_the_guide_is_flat():
    """F over a flat guide patch carries the 1/eps amplification of cov's rounding error; over texture it does not"""
    rng = np.random.default_rng(1)
    guide = rng.integers(0, 256, (64, 96)).astype(np.uint8)
    guide[:, :40] = 90
    depth = rng.uniform(0, 50, (32, 48)).astype(np.float32)
    F = gf_ref.floor(depth, guide, 4, 1e-3)
    P = float(depth.max())
    assert F[:, :20].min() > 10 * F[:, 60:].max()
    assert F.max() < 1e-8 * P                                 # still far below an ulp of float32 at the scale of p
    assert np.allclose(gf_ref.guide_var(np.full((5, 7), 33, np.uint8), 2), 0.0)
