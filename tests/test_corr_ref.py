"""CPU: the float64 correlation reference of tests/corr_ref.py against the fp32 C oracle, hand-computed answers, torch's bf16
conversion and a float32 emulation of the kernels' blend.

The GPU accuracy tests hold every correlation route to corr_ref.interval().  That bar means something only if the reference is
the operation the oracle computes (tap order, zeros outside the image, clamped window offsets, plane order g*9 + k, the 1/64
scale) and if its admissible warped values contain what the kernels' float32 arithmetic can produce."""
import numpy as np
import pytest
import torch

import corr_ref as R


def _oracle_out(oracle, fl, fr, flow, G, pattern):
    return oracle.corr_lookup(fl.transpose(2, 0, 1), fr.transpose(2, 0, 1), flow, G, pattern)


# ------------------------------------------------------------------ the reference is the oracle's operation

CASES = [(1, 9, 37, "random", "normal"), (2, 5, 20, "mixed", "normal"), (3, 3, 17, "mixed", "spread"),
         (1, 1, 13, "half", "normal"), (2, 2, 1, "mixed", "normal"), (1, 7, 2, "outside", "normal"),
         (1, 6, 24, "edge", "spread"), (1, 4, 19, "tiny_neg", "normal"), (1, 4, 19, "neg_frac", "normal"),
         (1, 5, 33, "large", "normal"), (2, 6, 16, "integer", "spread")]


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("G,h,w,flow,feat", CASES)
def test_reference_without_bf16_contains_the_oracle(oracle, G, h, w, flow, feat, pattern):
    """with the bf16 step left out (and the oracle's 128 float32 roundings per sum) the interval contains the fp32 oracle, and it
    is narrow: a reference with another tap order, padding, clamp, plane order or scale would not contain it"""
    rng = np.random.default_rng(G * 1000 + h * 37 + w + pattern)
    C = 64 * G
    fl, fr = R.features(feat, (h, w, C), rng), R.features(feat, (h, w, C), rng)
    fl[rng.random(fl.shape) < 0.1] = 0
    fw = R.flow_field(flow, h, w, rng)
    lo, hi, amb, zero = R.interval(fl, fr, fw, G, pattern, bf16_step=False, sum_roundings=128)
    got = _oracle_out(oracle, fl, fr, fw, G, pattern)
    R.check(got, lo, hi, amb, f"oracle G={G} {h}x{w} {flow} {feat} pattern {pattern}")
    assert (got[zero] == 0).all()
    # narrow: float32 ulps of the output's scale (a mistake in any of the above moves outputs by a fraction of it)
    rms = float(np.sqrt(np.mean(got.astype(np.float64) ** 2)))
    assert np.median(hi - lo) <= 1e-4 * rms and (hi - lo).max() <= 1e-3 * float(np.abs(got).max())


def test_plane_order_and_window_offsets_by_hand():
    """one-hot fl, fr[y, x, c] = 8 x + y + 64 g (small integers, exact in bf16), zero flow: out[g*9 + k, y, x] is the value at
    the clamped window position / 64, for both patterns"""
    h, w, G = 3, 6, 2
    fl = np.zeros((h, w, 64 * G), np.float32)
    fr = np.zeros_like(fl)
    for g in range(G):
        fl[..., 64 * g + 5] = 1
        fr[..., 64 * g + 5] = 8 * np.arange(w)[None, :] + np.arange(h)[:, None] + 64 * g
    flow = np.zeros((2, h, w), np.float32)
    for pattern in (0, 1):
        lo, hi, amb, _ = R.interval(fl, fr, flow, G, pattern)
        assert not amb.any()
        for g in range(G):
            for k in range(9):
                dy, dx = (0, k - 4) if pattern == 0 else (k // 3 - 1, k % 3 - 1)
                yy = np.clip(np.arange(h) + dy, 0, h - 1)[:, None]
                xx = np.clip(np.arange(w) + dx, 0, w - 1)[None, :]
                want = (8 * xx + yy + 64 * g) / 64.0
                assert (lo[g * 9 + k] <= want).all() and (want <= hi[g * 9 + k]).all()
                assert (hi[g * 9 + k] - lo[g * 9 + k] <= 2 * R.gamma(65) * np.abs(want) + 1e-300).all()


def test_integer_flow_and_all_outside_by_hand():
    """integer flow (+2, -1): the warped value is fr at (x + 2, y - 1), zero past the right / top border; flow (w, 0), (0, -h) and
    sample coordinates (-1 - 2^-20, y + 0.5): every tap outside, the interval is exactly [0, 0]"""
    h, w, G = 4, 9, 1
    rng = np.random.default_rng(5)
    fl = np.zeros((h, w, 64), np.float32)
    fl[..., 7] = 1
    fr = rng.integers(-100, 100, (h, w, 64)).astype(np.float32)
    flow = np.stack([np.full((h, w), 2.0), np.full((h, w), -1.0)]).astype(np.float32)
    lo, hi, amb, zero = R.interval(fl, fr, flow, G, 0)
    for k in range(9):
        xx = np.clip(np.arange(w) + k - 4, 0, w - 1)[None, :] + 2
        yy = np.arange(h)[:, None] - 1 + 0 * xx
        inside = (xx < w) & (yy >= 0)
        want = np.where(inside, fr[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1), 7], 0) / 64.0
        assert (lo[k] <= want).all() and (want <= hi[k]).all(), k
        assert (hi[k] - lo[k] <= 2 * R.gamma(65) * np.abs(want)).all()
        assert (zero[k] == ~inside).all()
    X = np.broadcast_to(np.arange(w, dtype=np.float64), (h, w))
    for fx, fy in ((np.full((h, w), w), 0), (0, np.full((h, w), -h)), (-1.0 - 2.0 ** -20 - X, 0.5)):
        flow = np.stack(np.broadcast_arrays(fx, fy, np.zeros((h, w)))[:2]).astype(np.float32)
        for pattern in (0, 1):
            lo, hi, amb, zero = R.interval(fl, fr, flow, G, pattern)
            assert (lo == 0).all() and (hi == 0).all() and zero.all()


def test_half_pixel_flow_by_hand():
    """flow (0.5, 0.5) over fr = 1: the four taps weigh 1/4 each; the interior blends to 1, the last column and last row to 1/2
    (two taps outside), the last pixel to 1/4 -- exact, so the interval is that value within E"""
    h, w = 3, 5
    fl = np.zeros((h, w, 64), np.float32)
    fl[..., 0] = 1
    fr = np.ones((h, w, 64), np.float32)
    flow = np.full((2, h, w), 0.5, np.float32)
    v, d, exact = R.blend(fr, flow)
    want = np.ones((h, w))
    want[-1, :] /= 2
    want[:, -1] /= 2
    assert exact.all() and (d == 0).all() and (v == want[..., None]).all()
    lo, hi, _, _ = R.interval(fl, fr, flow, 1, 0)
    assert (lo[4] <= want / 64).all() and (want / 64 <= hi[4]).all() and (hi[4] - lo[4] <= 2 * R.gamma(65) * want / 64).all()


# ------------------------------------------------------------------ rounding helpers

def test_bf16_matches_torch_on_every_upper_half():
    """every finite float32 upper half, with lower halves 0, 1, just below / at / just above the tie and the largest"""
    up = np.arange(1 << 16, dtype=np.uint32)
    up = up[((up >> 7) & 0xFF) != 0xFF]                     # inf / NaN are out of scope
    for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x4000, 0xC000):
        x = ((up << 16) | low).view(np.float32)
        want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
        got = R.bf16(x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), hex(low)
    x = np.random.default_rng(1).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    x = x[((x >> 23) & 0xFF) != 0xFF].view(np.float32)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.bf16(x).view(np.uint32), want.view(np.uint32))


def test_f32_directed_rounding():
    x = np.array([1.0, 1.0 + 2.0 ** -30, -1.0 - 2.0 ** -30, 2.0 ** -40 * 3, 0.0, -(2.0 ** -23) * 1.5])
    up, dn = R.f32_up(x), R.f32_down(x)
    assert (up.astype(np.float64) >= x).all() and (dn.astype(np.float64) <= x).all()
    assert (np.nextafter(up, np.float32(-np.inf)).astype(np.float64) < x).all()
    assert (np.nextafter(dn, np.float32(np.inf)).astype(np.float64) > x).all()
    assert up[0] == dn[0] == 1 and up[4] == dn[4] == 0


# ------------------------------------------------------------------ the kernels' float32 blend lies inside the interval

def _fma32(a, b, c):
    """float32 fma(a, b, c): a * b + c rounded once (a * b is exact in float64; the sum is made exact by TwoSum and its float64
    part is re-rounded to float32 unless it sits on a float32 midpoint, where the error term decides)"""
    p = a.astype(np.float64) * b.astype(np.float64)
    s, e = R.two_sum(p, c.astype(np.float64))
    r = s.astype(np.float32)
    nb = np.where(s > r.astype(np.float64), np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
    mid = (r.astype(np.float64) + nb.astype(np.float64)) / 2
    return np.where((s == mid) & (e != 0) & ((e > 0) == (nb > r)), nb, r)


def _kernel_blend(fr, flow, fma):
    """what k_corr_warp computes before the bf16 rounding: acc += bf * w over the in-image taps in tap order"""
    h, w, C = fr.shape
    ix, iy, wt = R.weights(flow)
    acc = np.zeros((h, w, C), np.float32)
    for t in range(4):
        xx, yy = ix + (t & 1), iy + (t >> 1)
        inside = ((xx >= 0) & (xx < w) & (yy >= 0) & (yy < h))[..., None]
        v = fr[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float32)
        wgt = np.broadcast_to(wt[t][..., None], v.shape)
        nxt = _fma32(v, wgt, acc) if fma else (acc + v * wgt).astype(np.float32)
        acc = np.where(inside, nxt, acc)
    return acc


@pytest.mark.parametrize("feat", ["normal", "spread"])
@pytest.mark.parametrize("flow", ["random", "mixed", "half", "tiny_neg"])
def test_emulated_kernel_blend_is_admissible(flow, feat):
    """a float32 emulation of the kernels' blend, with and without FMA, rounded to bf16, lies in [Blo, Bhi]; and the two
    emulations differ somewhere (the bound is not vacuous)"""
    rng = np.random.default_rng(len(flow) * 7 + len(feat))
    h, w, C = 8, 96, 64
    fr = R.features(feat, (h, w, C), rng)
    fw = R.flow_field(flow, h, w, rng)
    lo, hi = R.warped(fr, fw)
    lo32, hi32 = R.warped(fr, fw, bf16_step=False)
    seen = []
    for fma in (False, True):
        acc = _kernel_blend(fr, fw, fma)
        assert ((lo32 <= acc) & (acc <= hi32)).all(), f"fma={fma}: float32 blend outside [v64 - delta, v64 + delta]"
        b = R.bf16(acc).astype(np.float64)
        bad = (b < lo) | (b > hi)
        assert not bad.any(), f"fma={fma}: {int(bad.sum())} bf16 values outside [Blo, Bhi]"
        seen.append(acc)
    if flow in ("random", "mixed"):
        assert (seen[0] != seen[1]).any()
    print(f"\nREF blend {flow} {feat}: {(lo != hi).mean():.2e} of the warped values have two candidates")


def test_fma_emulation_on_midpoints():
    """_fma32 against exact rationals, on sums built to land on float32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(9)
    a = R.bf16(rng.normal(0, 1, 4000).astype(np.float32))
    b = rng.uniform(0, 1, 4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b)).astype(np.float32)      # a * b + c: the product's low bits, cancellation near zero
    c[::2] = rng.normal(0, 1, 2000).astype(np.float32)
    got = _fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))
        cand = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cand, key=lambda f: (abs(Fraction(float(f)) - exact), int(np.float32(f).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i])
