"""Every float entry on NaN (sign bit clear and set), +-inf, -0.0, a denormal, FLT_MAX and depths at and above the edge of the
fixed point (tests/nonfinite.py), against the restatements that state the contract of include/v3d_hip.h ("Non-finite input" in
DESIGN.md section 4) without ever converting a non-finite float: tests/temporal_ref.py, temporal_mc_ref.py, range_ref.py,
quality_ref.py, corr_ref.py, the f64 oracle of the guided filter and a NumPy transcription of depth.py:344-374.

Every batch has at least three frames and only the middle one carries a special: the neighbours' outputs must equal the clean
run's, which checks slot and stride indexing.  Every input is a legal buffer of legal size.

The two audio entries (v3d_xcorr, v3d_align_audio) take one pair of tracks per call: a NaN or an infinity at the first, a middle
and the last sample of either track or both, inside guard arenas."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import corr_ref as CR
import nonfinite as NF
import quality_ref as QR
import range_ref as RR
import temporal_mc_ref as MR
import temporal_ref as TR
from conftest import mismatch_report
from guard_arena import Arena

pytestmark = pytest.mark.gpu

NAN_P, NAN_N = NF.SPECIALS["nan+"], NF.SPECIALS["nan-"]


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(a, pad):
    """[T,H,W] array -> device tensor whose frames lie `pad` elements further apart than their size (dense for pad = 0)"""
    if not pad:
        return _dev(a)
    T, H, W = a.shape
    buf = torch.zeros((T, H * W + pad), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    buf[:, :H * W] = _dev(a.reshape(T, H * W))
    return buf[:, :H * W].view(T, H, W)


def _f32(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------- per-frame min/max, robust range, normalisation

def _range_base(n):
    """three clean frames of n elements: a blend's floats with invalid zeros, every frame with its own scale"""
    rng = np.random.default_rng(n)
    d = (rng.uniform(0.5, 60.0, (3, 1, n)) * np.float32([1.0, 0.5, 2.0])[:, None, None]).astype(np.float32)
    d[rng.random(d.shape) < 0.15] = 0.0
    return d


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "stride+5"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1027])
def test_range_entries(native, n, pad):
    """v3d_depth_minmax_batch as bit patterns modulo "is NaN" (a NaN of either sign anywhere -> (NaN, NaN); -0.0 below +0.0; +-inf
    ordinary extrema), v3d_depth_robust_minmax_batch at q = 5000, 9800, 10000, v3d_depth_to_u16_batch (dense) and
    v3d_depth_to_u16_range_batch against the restatements.  The stride of +5 elements takes k_rr_hist's element-wise instantiation."""
    base = _range_base(n)
    clean_mm = _f32(native.depth_minmax_batch(_strided(base, pad)))
    assert NF.same_floats(clean_mm, TR.minmax(base))
    clean_rb = {q: _f32(native.depth_robust_minmax_batch(_strided(base, pad), q)) for q in (5000, 9800, 10000)}
    clean_u16 = _u16(native.depth_to_u16_range_batch(_strided(base, pad), _dev(clean_mm)))
    with NF.cast_warnings_are_errors():
        for label, where in NF.placements(n):
            d = base.copy()
            d[1] = NF.put(d[1], where)
            dd = _strided(d, pad)
            what = f"{label} n={n} pad={pad}"
            mm = _f32(native.depth_minmax_batch(dd))
            want_mm = TR.minmax(d)
            assert NF.same_floats(mm, want_mm), (what, mm.tolist(), want_mm.tolist())
            assert np.isnan(d[1]).any() == np.isnan(mm[1]).all() == np.isnan(mm[1]).any(), what
            assert np.array_equal(mm[[0, 2]].view(np.uint32), clean_mm[[0, 2]].view(np.uint32)), what
            for q in (5000, 9800, 10000):
                rb = _f32(native.depth_robust_minmax_batch(dd, q))
                want = RR.robust_minmax(d, q)
                assert NF.same_floats(rb, want), (what, q, rb.tolist(), want.tolist())
                assert np.array_equal(rb[[0, 2]].view(np.uint32), clean_rb[q][[0, 2]].view(np.uint32)), (what, q)
            want_u16 = TR.to_u16_range(d, want_mm)
            got = _u16(native.depth_to_u16_range_batch(dd, _dev(mm)))
            assert not mismatch_report(got, want_u16, f"range_batch, own range, {what}")
            assert np.array_equal(got[[0, 2]], clean_u16[[0, 2]]), what
            if not np.isfinite(want_mm[1]).all():
                assert not got[1].any(), what                    # a NaN or an infinite bound: a frame of 0
            if not pad:
                assert np.array_equal(_u16(native.depth_to_u16_batch(dd)), want_u16), what
            # the same frames against the robust range of q = 9800 (NaN, NaN) included
            rb = RR.robust_minmax(d, 9800)
            assert np.array_equal(_u16(native.depth_to_u16_range_batch(dd, _dev(rb))), TR.to_u16_range(d, rb)), what
        # ranges handed in: unordered, NaN on either side, infinite on either side or both -> 0; the neighbours keep their bits
        d = base.copy()
        d[1] = NF.put(d[1], dict(list(NF.placements(n))[-2][1]))              # all specials together
        for lohi in ((-np.inf, np.inf), (NAN_P, 3.0), (NAN_N, 3.0), (0.0, NAN_P), (0.0, NAN_N), (np.inf, np.inf), (-np.inf, -np.inf),
                     (0.0, np.inf), (-np.inf, 10.0), (9.0, 3.0), (-0.0, 0.0), (0.0, 1e-45), (0.0, NF.FLT_MAX), (-NF.FLT_MAX, NF.FLT_MAX)):
            r = clean_mm.copy()
            r[1] = lohi
            got = _u16(native.depth_to_u16_range_batch(_strided(d, pad), _dev(r)))
            assert not mismatch_report(got, TR.to_u16_range(d, r), f"lohi {lohi} n={n} pad={pad}")
            assert np.array_equal(got[[0, 2]], clean_u16[[0, 2]])
            if not (np.isfinite(np.float32(lohi)).all() and lohi[1] > lohi[0]):
                assert not got[1].any(), lohi


# ---------------------------------------------------------------- v3d_temporal_range

def _range_cases(T, pos):
    """(cut_at, cut) for a NaN frame at `pos`: no cut, a cut before, at and after it"""
    for cut_at in (None, pos - 1, pos, pos + 1):
        cut = np.zeros(T, np.uint8)
        if cut_at is not None and 1 <= cut_at < T:
            cut[cut_at] = 1
        yield cut_at, cut


def _check_ranges(native, mm, want_mm, cut, R, pos, rng, what):
    T = len(want_mm)
    cd = _dev(cut)
    for (t0, n) in ((0, T), (pos, 1), (int(rng.integers(0, T)), None)):
        n = int(rng.integers(1, T - t0 + 1)) if n is None else n
        got = _f32(native.temporal_range(mm, cd, R, t0, n))
        want = TR.ranges(want_mm, cut, R, t0, n)
        assert NF.same_floats(got, want), (what, t0, n, got.tolist(), want.tolist())
        for j in range(n):
            lo, hi = TR.admissible(cut, T, t0 + j, R)
            assert np.isnan(got[j]).all() == (lo <= pos <= hi), (what, t0 + j)


@pytest.mark.parametrize("R", [0, 1, 2, 8])
def test_temporal_range_propagates_a_nan_bound_from_every_position(native, R):
    """v3d_temporal_range alone, on hand-made bounds: T = 9, one NaN bound (the min or the max of one frame, either sign) at every
    position 0..8, a cut before, at and after it.  A NaN bound in any admissible frame gives (NaN, NaN) for that target,
    wherever the frame sits in the target's window, and no other target changes.  (A fold with `l < lo ? l : lo` keeps a NaN only
    from the window's first frame: with R >= 1 this test fails on it at the first position that is not a window's first.)"""
    T = 9
    rng = np.random.default_rng(R)
    clean = TR.minmax(rng.uniform(0.0, 50.0, (T, 3, 37)).astype(np.float32))
    for pos in range(T):
        for cut_at, cut in _range_cases(T, pos):
            for col in (0, 1):
                want_mm = clean.copy()
                want_mm[pos, col] = NAN_N if (pos + col) % 2 else NAN_P
                _check_ranges(native, _dev(want_mm), want_mm, cut, R, pos, rng, (R, pos, cut_at, "min only" if col == 0 else "max only"))
    # infinities are ordinary extrema
    mm = clean.copy()
    mm[4] = (-np.inf, np.inf)
    got = _f32(native.temporal_range(_dev(mm), _dev(np.zeros(T, np.uint8)), R))
    assert NF.same_floats(got, TR.ranges(mm, np.zeros(T, np.uint8), R))


@pytest.mark.parametrize("R", [0, 1, 2, 8])
def test_temporal_range_of_a_clip_with_one_nan_pixel(native, R):
    """the same positions and cuts with the bounds v3d_depth_minmax_batch gives for a clip with one NaN pixel (either sign): the
    two entries chained, as the temporal stage chains them"""
    T = 9
    rng = np.random.default_rng(R)
    clip = rng.uniform(0.0, 50.0, (T, 3, 37)).astype(np.float32)
    for pos in range(T):
        for k, (cut_at, cut) in enumerate(_range_cases(T, pos)):
            for v in (NAN_P, NAN_N):
                d = clip.copy()
                d[pos, 1, (5 * pos + k) % 37] = v
                mm = native.depth_minmax_batch(_dev(d))
                want_mm = TR.minmax(d)
                assert NF.same_floats(_f32(mm), want_mm)
                _check_ranges(native, mm, want_mm, cut, R, pos, rng, (R, pos, cut_at, "pixel", bool(np.signbit(v))))


# ---------------------------------------------------------------- the filter, plain and compensated

def _filter_clip(rng, T, H, W):
    d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
    d[rng.random((T, H, W)) < 0.2] = 0.0
    base = rng.integers(0, 256, (H, W))
    g = np.clip(base[None] + rng.integers(-12, 13, (T, H, W)), 0, 255).astype(np.uint8)
    return d, g


def _special_pixels(rng, H, W):
    """{flat index: value}: every special at the four positions of tests/nonfinite.py's placements (rotated so that they do not
    collide) and at four random pixels"""
    n = H * W
    where = {}
    free = [i for i in rng.permutation(n)]
    fixed = NF.positions(n) + [W - 1, W, n - W, n - 2]
    for k, v in enumerate(NF.SPECIALS.values()):
        for p in fixed:
            where.setdefault((p + 7 * k) % n if k else p, v)
        for _ in range(4):
            where.setdefault(int(free.pop()), v)
    return where


def _guarded_out(n, H, W):
    """(out view [n,H,W], check): the output inside a larger buffer of a sentinel, 16-byte aligned like a fresh tensor"""
    pad = 1024
    buf = torch.full((2 * pad + n * H * W,), -12345.0, dtype=torch.float32, device="cuda")

    def check(what):
        edge = torch.cat([buf[:pad], buf[pad + n * H * W:]]).cpu().numpy()
        assert (edge == -12345.0).all(), f"{what}: {int((edge != -12345.0).sum())} floats written outside out"
    return buf[pad:pad + n * H * W].view(n, H, W), check


def _defined(d, gray, R, tau, cut, filt):
    """bool [T,H,W]: the pixels whose value the filter's contract defines.  The kernel decides validity on the float but does not
    clamp a valid tap's value (the fallback of DESIGN.md, "Non-finite input"): the domain is D <= 2047.9375, and a pixel whose
    window holds a tap above it with a non-zero weight has an unspecified value.  Those pixels are found with the restatement
    itself, run on an indicator clip (1.0 at the taps above the domain, invalid elsewhere, holes filled): its output is non-zero
    exactly where such a tap has weight."""
    with np.errstate(over="ignore", invalid="ignore"):
        above = (np.rint(d * np.float32(16)) > TR.D16_MAX).astype(np.float32)          # False for NaN
    return filt(above, gray, R, tau, cut, 1) == 0


@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("size", [(260, 12), (63, 5)], ids=["260x12", "63x5"])
def test_temporal_filter_and_mc(native, size, R):
    """specials at the centre tap only, at every non-centre tap only and at all taps of the middle target's window.  NaN, -inf,
    -0.0 and a denormal are invalid taps; 2047.9375 is the largest valid one.  FLT_MAX, 2048.0, 1e9 and +inf lie above the domain:
    a pixel that takes such a tap with a non-zero weight is unspecified (_defined), every other pixel of every target equals the
    restatement bit for bit, the output is finite, and nothing outside `out` is written.  The compensated entry with all-zero
    fields equals the plain one on every pixel, specified or not (one kernel); with a constant (3, -2) field its displaced loads
    carry the specials (tests/temporal_mc_ref.py)."""
    W, H = size
    T = 2 * R + 4
    rng = np.random.default_rng(1000 * R + W)
    depth, gray = _filter_clip(rng, T, H, W)
    where = _special_pixels(rng, H, W)
    t = T // 2
    BH, BW = -(-H // 16), -(-W // 16)
    zero = np.zeros((T, BH, BW, 2), np.int16)
    const = np.broadcast_to(np.int16([3, -2]), (T, BH, BW, 2)).copy()
    cut = np.zeros(T, np.uint8)
    gd, cd = _dev(gray), _dev(cut)
    mc_ref = lambda d, g, R_, tau, c, fill: MR.filter_clip(d, g, R_, tau, c, const, const, fill)   # noqa: E731
    with NF.cast_warnings_are_errors():
        for i, place in enumerate(("centre", "non-centre", "all")):
            d = depth.copy()
            for u in range(T):
                if abs(u - t) <= R and ((place == "centre") == (u == t) or place == "all"):
                    d[u] = NF.put(d[u], where)
            tau, fill = (1, 12, 255)[(i + R) % 3], (i + R) % 2
            what = f"{W}x{H} R={R} tau={tau} fill={fill} specials at {place} taps"
            dd = _dev(d)
            want, ok = TR.filter_clip(d, gray, R, tau, cut, fill), _defined(d, gray, R, tau, cut, TR.filter_clip)
            assert ok.mean() > 0.5 and not ok.all(), what
            out, check = _guarded_out(T, H, W)
            got = _f32(native.temporal_filter_batch(dd, gd, R, tau, cd, fill, out=out))
            check(what)
            assert np.isfinite(got).all(), what
            rep = mismatch_report((got * 16).astype(np.int64)[ok], (want * 16).astype(np.int64)[ok], what)
            assert not rep and np.array_equal(got[ok], want[ok]), rep
            out, check = _guarded_out(T, H, W)
            got0 = _f32(native.temporal_filter_mc_batch(dd, gd, R, tau, cd, _dev(zero), _dev(zero), fill, out=out))
            check(f"zero fields, {what}")
            assert np.array_equal(got0, got), f"zero fields, {what}"
            out, check = _guarded_out(T, H, W)
            gotc = _f32(native.temporal_filter_mc_batch(dd, gd, R, tau, cd, _dev(const), _dev(const), fill, out=out))
            check(f"(3,-2) field, {what}")
            wantc, okc = MR.filter_clip(d, gray, R, tau, cut, const, const, fill), _defined(d, gray, R, tau, cut, mc_ref)
            assert np.isfinite(gotc).all() and okc.mean() > 0.5, what
            rep = mismatch_report((gotc * 16).astype(np.int64)[okc], (wantc * 16).astype(np.int64)[okc], f"(3,-2) field, {what}")
            assert not rep and np.array_equal(gotc[okc], wantc[okc]), rep
        # only the specials inside the domain: every pixel of every target is defined and exact
        inside = {p: v for p, v in where.items() if TR.d16_loop(v) < TR.D16_MAX or v == np.float32(2047.9375)}
        assert len(inside) > len(where) // 2
        d = depth.copy()
        for u in range(max(t - R, 0), min(t + R, T - 1) + 1):
            d[u] = NF.put(d[u], inside)
        for fill in (0, 1):
            got = _f32(native.temporal_filter_batch(_dev(d), gd, R, 12, cd, fill))
            assert np.array_equal(got, TR.filter_clip(d, gray, R, 12, cut, fill)), f"{W}x{H} R={R} fill={fill} specials inside the domain"
        # a sub-range of targets and strided frames: slot indexing with specials in the buffer
        d = depth.copy()
        d[t] = NF.put(d[t], where)
        got = _f32(native.temporal_filter_batch(_strided(d, 4), _strided(gray, 4), R, 12, cd, 1, t - 1, 3))
        ok = _defined(d, gray, R, 12, cut, TR.filter_clip)[t - 1:t + 2]
        assert np.array_equal(got[ok], TR.filter_clip(d, gray, R, 12, cut, 1, t - 1, 3)[ok])


# ---------------------------------------------------------------- the streaming driver

@pytest.mark.timeout(300)
def test_streaming_driver_is_step_independent_with_a_nan_and_an_inf(native):
    """an 11-frame 320x64 clip whose frame 4 holds one NaN and whose frame 7 holds one +inf, pushed in steps of 1, 2, 3, 5 and 11:
    every step size gives the whole-clip restatement (a range that depended on where the NaN frame sits in a window would show
    here as a step-dependent output)"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HipStereoBackend
    from video_3d_pipeline.temporal import TemporalStabilizer
    W, H, T = 320, 64, 11
    L, Rr, _ = syn.temporal_clip(W, H, T, cut_at=6)
    m = native.StereoSGBM(W, H, T)
    depth = native.disp_to_depth(m.compute(_dev(L), _dev(Rr))).cpu().numpy()
    m.close()
    depth[4, 20, 101] = NAN_N
    depth[7, 33, 250] = np.inf
    be = HipStereoBackend()
    dd, gd = _dev(depth), _dev(L)
    for R in (1, 2, 8):
        with NF.cast_warnings_are_errors():
            want = TR.stabilize(depth, L, R)
        cut = TR.cuts(L, 20)
        for t in range(T):
            lo, hi = TR.admissible(cut, T, t, R)
            assert want[t].any() == (not (lo <= 4 <= hi or lo <= 7 <= hi)), (R, t)   # a NaN or infinite range: a frame of 0
        whole = _u16(be.temporal_stabilize(dd, gd, 0, T, R, 12, 20, True))
        assert not mismatch_report(whole, want, f"whole clip R={R}")
        for step in (1, 2, 3, 5, 11):
            st = TemporalStabilizer(be, R)
            parts = []
            for i in range(0, T, step):
                out = st.push(dd[i:i + step].clone(), gd[i:i + step].clone())
                if out is not None:
                    parts.append(_u16(out))
            out = st.finish()
            if out is not None:
                parts.append(_u16(out))
            assert np.array_equal(np.concatenate(parts), want), (R, step)


# ---------------------------------------------------------------- the hybrid blend

def _blend_numpy(oracle, d16, mono):
    """depth.py:344-374 in NumPy float32 on the oracle's resize, the way tests/golden/make_golden.py blend() writes it
    -> (blend, resized map)"""
    H, W = d16.shape
    with np.errstate(invalid="ignore", over="ignore"):
        r = mono if mono.shape == (H, W) else oracle.resize_linear_f32(mono, W, H)       # depth.py:352: same size is not resized
        disp = d16.astype(np.float32) / 16.0
        if r.max() > r.min():                                                            # False with a NaN anywhere: stereo only
            disp = 0.7 * disp + 0.3 * ((r - r.min()) / (r.max() - r.min()) * 64)
        disp = disp.astype(np.float32)
        disp[disp <= 0] = 0
    return disp, r


@pytest.mark.parametrize("mw,mh", [(97, 333), (48, 48), (203, 77)], ids=["down", "up", "identity"])
def test_mono_blend_batch(native, oracle, mw, mh):
    """one special per frame of a batch of 3, judged by what reaches the resized map r.  A NaN in r gives a stereo-only frame --
    and an infinity under a bilinear tap of weight 0 becomes one (inf * 0); +inf in r gives e = 0 at the finite pixels and a NaN
    where r is +inf; -inf in r makes (r - min) infinite everywhere, so every pixel of the frame is NaN: in each case what the
    NumPy expression of depth.py gives, NaN positions compared as positions (a down-scaling resize reads two of every 4.3 rows: a
    special on a row it skips changes nothing)"""
    W, H = 203, 77
    rng = np.random.default_rng(mw)
    d16 = rng.integers(0, 64 * 16, (3, H, W)).astype(np.int16)
    d16[rng.random((3, H, W)) < 0.25] = -16
    base = (rng.random((3, mh, mw)) * 30 - 4).astype(np.float32)
    dd = _dev(d16)
    clean = _f32(native.mono_blend(dd, _dev(base)))
    for f in range(3):
        assert np.array_equal(clean[f], oracle.mono_blend(d16[f], base[f]))
    names = list(NF.NAMES)
    spots = NF.positions(mh * mw) + [mw - 1, (mh // 2) * mw + mw // 2]
    reached = set()
    for k in range(0, len(names), 3):
        for p in spots:
            mono = base.copy()
            used = [names[(k + f) % len(names)] for f in range(3)]
            for f in range(3):
                mono[f].reshape(-1)[(p + f) % (mh * mw)] = NF.SPECIALS[used[f]]
            got = _f32(native.mono_blend(dd, _dev(mono)))
            for f in range(3):
                want, r = _blend_numpy(oracle, d16[f], mono[f])
                what = f"{used[f]} at {(p + f) % (mh * mw)} of a {mw}x{mh} map, frame {f}"
                assert NF.same_floats(got[f], want), (what, int((np.isnan(got[f]) != np.isnan(want)).sum()))
                if np.isfinite(r).all():
                    assert np.array_equal(got[f], oracle.mono_blend(d16[f], mono[f])), what     # finite: the oracle's C is defined
                    continue
                if np.isnan(r).any():                     # a NaN, or an infinity under a tap of weight 0 (inf * 0): stereo only
                    reached.add("nan")
                    assert np.array_equal(got[f], oracle.disp_to_depth(d16[f])), what
                elif (r == np.inf).any():
                    reached.add("+inf")
                    ok = ~np.isnan(got[f])
                    assert np.array_equal(~ok, r == np.inf) and 0 < (~ok).sum() < W * H // 4, what
                    assert np.array_equal(got[f][ok], (np.float32(0.7) * oracle.disp_to_depth(d16[f]))[ok]), what   # e = 0
                else:
                    reached.add("-inf")
                    assert (r == -np.inf).any() and np.isnan(got[f]).all(), what
    assert reached == {"nan", "+inf", "-inf"}


# ---------------------------------------------------------------- the guided filter's float route

GF_ROUTES = {"fused": {"gf_fused": 1, "gf_tiled": 0}, "sweeps": {"gf_fused": 0, "gf_tiled": 0}, "tiled": {"gf_fused": 1, "gf_tiled": 1}}
# the float route's domain is finite and |v| <= 65535 (test_guided_accuracy_gpu.py): FLT_MAX and 1e9 lie outside it and are no
# input of this entry; the non-finite specials are mapped to 0 by its loads
GF_SPECIALS = ("nan+", "nan-", "+inf", "-inf", "-0.0", "denormal", "2048", "2047.9375")


@contextlib.contextmanager
def _options(native, opts):
    saved = {k: native.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            native.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            native.set_option(k, v)


GF_TX, GF_RUN, GF_BAND = 64, 8, 16          # v3d_guided.hip: the tiled kernel's tile width and run length; the band height this test sets


def _gf_spots(r, Wlo, Hlo):
    """low-resolution (row, column) spots of an exact 2x upscale, derived from the kernels' geometry.  Output row y reads low rows
    around y / 2.  The tiled kernel (every route at r = 1 and 16, route "tiled" at r = 8) works on tiles of 64 columns x 16 rows
    (8 rows for r > 8) and sums horizontally in runs of 8 outputs; the fused and the two-sweep kernels (r = 8) slide their window
    sums down bands of GF_BAND rows (set by the test) and along the whole 96-column strip.  So: the low rows that feed a tile's /
    band's last and next first row, the low columns on both sides of a run's end and of a tile's edge, and the four corners."""
    ty = 16 if r <= 8 else 8
    rows = sorted({0, ty // 2 - 1, ty // 2, GF_BAND // 2 - 1, GF_BAND // 2, 2 * (GF_BAND // 2) - 1, 2 * (GF_BAND // 2), Hlo - 1})
    cols = sorted({0, GF_RUN // 2 - 1, GF_RUN // 2, GF_TX // 2 - 1, GF_TX // 2, Wlo - 1})
    corners = [(0, 0), (0, Wlo - 1), (Hlo - 1, 0), (Hlo - 1, Wlo - 1)]
    return corners + [(y, cols[(3 * i + 1) % len(cols)]) for i, y in enumerate(rows)] + [(rows[(2 * j + 1) % len(rows)], x) for j, x in enumerate(cols)]


@pytest.mark.parametrize("route", list(GF_ROUTES))
@pytest.mark.parametrize("r", [1, 8, 16])
def test_guided_upscale_float_route(native, oracle, r, route):
    """48x27 -> 96x54, bands of 16 rows: specials at the corners, on the low rows that feed a tile's or a band's first and last
    row, and on the columns where a horizontal run and a tile end (_gf_spots).  A non-finite sample counts as 0 (an invalid depth):
    the output equals the f64 oracle on the input with those samples replaced by 0, within the project's 1e-3 relative bar, and is
    finite everywhere -- a NaN let into a sliding window sum would poison the rest of its strip"""
    Wlo, Hlo, W, H = 48, 27, 96, 54
    rng = np.random.default_rng(7)
    lo = rng.uniform(1.0, 60.0, (3, Hlo, Wlo)).astype(np.float32)
    lo[rng.random(lo.shape) < 0.1] = 0.0
    from scipy.ndimage import gaussian_filter
    guide = np.stack([np.clip(gaussian_filter(rng.integers(0, 256, (H, W)).astype(np.float32), 1.5) * 2 - 128, 0, 255) for _ in range(3)]).astype(np.uint8)
    spots = _gf_spots(r, Wlo, Hlo)
    assert len(set(spots)) >= 12
    gd = _dev(guide)
    with _options(native, dict(GF_ROUTES[route], gf_band=GF_BAND, gf_band1=GF_BAND, gf_band2=GF_BAND)):
        clean = _f32(native.guided_upscale_batch(_dev(lo), gd, r, 1e-3))
        cases = [[(s, GF_SPECIALS[k % len(GF_SPECIALS)])] for k, s in enumerate(spots)] + [[(s, GF_SPECIALS[(k + 3) % len(GF_SPECIALS)]) for k, s in enumerate(spots)]]
        for case in cases:
            x = lo.copy()
            for (yy, xx), name in case:
                x[1, yy, xx] = NF.SPECIALS[name]
            got = _f32(native.guided_upscale_batch(_dev(x), gd, r, 1e-3))
            assert np.isfinite(got).all(), (case, int((~np.isfinite(got)).sum()))
            assert np.array_equal(got[[0, 2]], clean[[0, 2]]), case
            z = np.where(np.isfinite(x[1]), x[1], np.float32(0))
            want = oracle.guided_upscale(z, guide[1], r, 1e-3)
            rel = np.abs(got[1].astype(np.float64) - want) / np.maximum(np.abs(want), 1e-6 * np.abs(want).max())
            assert rel.max() <= 1e-3, (case, rel.max())


# ---------------------------------------------------------------- flicker

@pytest.mark.parametrize("W,H,T", [(7, 3, 3), (64, 5, 2), (253, 77, 3), (320, 180, 4)])
def test_quality_flicker(native, W, H, T):
    """the 10 % NaN clip of test_quality_gpu.py with NaNs of both signs, +-inf, 1e9, FLT_MAX and the edge of the fixed point:
    NaN and -inf are invalid, +inf and every depth above the range count as 32767"""
    rng = np.random.default_rng(13 * W + H)
    base = rng.integers(1, 1024, (1, H, W))
    d = (np.clip(base + rng.integers(-40, 41, (T, H, W)), -30, 32767) / 16).astype(np.float32)
    d += (rng.random((T, H, W)) < 0.3) * np.float32(1 / 64)
    d[rng.random((T, H, W)) < 0.1] = np.nan
    for v in NF.SPECIALS.values():
        d[rng.random((T, H, W)) < 0.03] = v
    g = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-5, 6, (T, H, W)), 0, 255).astype(np.uint8)
    dd, gd = _dev(d), _dev(g)
    with NF.cast_warnings_are_errors():
        for still, jump in ((4, 16), (0, 0), (255, 32766), (255, 32767)):
            got = native.quality_flicker_batch(dd, gd, still, jump).cpu().numpy()
            want = QR.flicker(d, g, still, jump)
            assert np.array_equal(got, want), f"{W}x{H}x{T} still {still} jump {jump}:\n got {got.tolist()}\nwant {want.tolist()}"
    # still pixels that move from 1/16 to +inf: 32766 each; to NaN or -inf: not counted
    pair = np.full((2, H, W), 1 / 16, np.float32)
    pair[1].reshape(-1)[:3] = (np.inf, np.nan, -np.inf)
    zeros = np.zeros((2, H, W), np.uint8)
    got = native.quality_flicker_batch(_dev(pair), _dev(zeros), 0, 0).cpu().numpy()
    assert got.tolist() == QR.flicker(pair, zeros, 0, 0).tolist() == [[0, W * H - 2, 32766, 1]]


# ---------------------------------------------------------------- the correlation lookup inside a guard arena

CORR_ROUTES = {"fused": {"corr_fused": 1, "corr_gather": 0}, "warp-gemm": {"corr_fused": 0, "corr_gather": 0},
               "gather": {"corr_fused": 1, "corr_gather": 1}}


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("route", list(CORR_ROUTES))
def test_corr_lookup_with_non_finite_flow(native, route, pattern):
    """C = 128, 6 x 20, fl, fr, flow, out and ws inside guard arenas; the flow holds NaN, +-inf, +-1e30, +-2^31 and w - 0.5 at
    scattered pixels.  A tap whose coordinate is not inside the plane contributes 0 (tests/corr_ref.py decides that on the floats);
    the guards stay intact, the outputs whose window holds such a pixel lie in the reference's interval, every other output has
    the clean run's bits"""
    Cc, h, w, G = 128, 6, 20, 2
    rng = np.random.default_rng(5 + pattern)
    fl, fr = CR.features("normal", (h, w, Cc), rng), CR.features("normal", (h, w, Cc), rng)
    flow = rng.uniform(-3, 3, (2, h, w)).astype(np.float32)
    bad = flow.copy()
    vals = [NAN_P, NAN_N, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31]
    touched = np.zeros((h, w), bool)
    for k, v in enumerate(vals):
        for c in (0, 1):                                             # each value once in x and once in y, at pixels of their own
            y, x = (3 * k + c) % h, (7 * k + 11 * c + 2) % w
            assert not touched[y, x]
            bad[c, y, x] = v
            touched[y, x] = True
    for y, x in ((0, 0), (h - 1, w - 1), (2, 13)):                   # sample coordinate w - 0.5: the tap x0 + 1 is the first outside
        assert not touched[y, x]
        bad[0, y, x] = np.float32(w - 0.5 - x)
        touched[y, x] = True
    # an output is affected iff a position of its window is a touched pixel
    affected = np.zeros((G * 9, h, w), bool)
    for k in range(9):
        dy, dx = CR.window(pattern, k)
        yy = np.clip(np.arange(h) + dy, 0, h - 1)[:, None]
        xx = np.clip(np.arange(w) + dx, 0, w - 1)[None, :]
        affected[k::9] = touched[yy, xx]
    bits = lambda a: torch.from_numpy(a).bfloat16().view(torch.int16).numpy().view(np.uint16).reshape(h, w * Cc)   # noqa: E731
    lib = native.lib()
    outs = {}
    for name, f in (("clean", flow), ("bad", bad)):
        for poison in (0xA5, 0x00):
            a = Arena("cuda", poison)
            bl = a.buf("fl", "in", np.uint16, (h, w * Cc), align=16).set(bits(fl))
            br = a.buf("fr", "in", np.uint16, (h, w * Cc), align=16).set(bits(fr))
            bf = a.buf("flow", "in", np.float32, (2 * h, w)).set(f.reshape(2 * h, w))
            bo = a.buf("out", "out", np.float32, (G * 9, h * w))
            ws = a.buf("ws", "ws", np.uint8, (max(int(lib.v3d_corr_ws_bytes(Cc, h, w)), 1),), align=16)
            a.fill()
            a.snapshot()
            P = lambda b: C.c_void_p(b.ptr)                          # noqa: E731
            with _options(native, CORR_ROUTES[route]):
                rc = lib.v3d_corr_lookup(P(bl), P(br), P(bf), Cc, h, w, G, pattern, P(bo), P(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc
            torch.cuda.synchronize()
            a.check()
            got = bo.get().reshape(G * 9, h, w)
            if name in outs:
                assert np.array_equal(got.view(np.uint32), outs[name].view(np.uint32)), "the poison byte changed the output"
            outs[name] = got
    clean, got = outs["clean"], outs["bad"]
    assert np.array_equal(got[~affected].view(np.uint32), clean[~affected].view(np.uint32)), "an unaffected output changed"
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite outputs, at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    with NF.cast_warnings_are_errors():
        lo, hi, amb, zero = CR.interval(fl, fr, bad, G, pattern)
    assert (got[zero] == 0).all()
    CR.check(got.astype(np.float64), lo, hi, amb, f"{route} pattern {pattern} non-finite flow")


# ---------------------------------------------------------------- end to end

@pytest.mark.timeout(300)
def test_extractor_with_a_provider_that_returns_a_nan_and_an_inf(native, oracle, tmp_path):
    """HybridStereoDepthExtractor at 256x72, 3 frames: the provider's map is clean for frame 0, holds one NaN for frame 1 and one
    +inf for frame 2.  What the product writes, as depth.py would: frame 1 is the stereo-only map (the blend is skipped: max > min
    is false); frame 2's blend has NaN pixels, so its own range is (NaN, NaN) and the PNG is a frame of 0 (DESIGN.md section 4,
    "Non-finite input")"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.utils import read_png16
    frames = np.stack([syn.sbs_frame(256, 72, i) for i in range(3)])
    clip = tmp_path / "clip.npy"
    np.save(clip, frames)
    seen = []

    def net(rgb):
        g = rgb.astype(np.float32).mean(axis=2)[::2, ::3].copy()      # a luma "network": deterministic in the input
        k = len(seen)
        if k % 3 == 1:
            g[11, 40] = NAN_N
        if k % 3 == 2:
            g[30, 7] = np.inf
        return g

    def provider(left_rgb_frames):
        out = []
        for rgb in left_rgb_frames:
            out.append(torch.from_numpy(net(rgb)).cuda())
            seen.append(rgb)
        return out

    ex = HybridStereoDepthExtractor(work_dir=str(tmp_path / "w"), cache_dir=str(tmp_path / "w"), batch_size=2, mono_provider=provider)
    outdir = ex.process_video_sbs(str(clip))
    assert len(seen) == 3
    for i in range(3):
        d16 = oracle.sgbm_compute(*oracle.sbs_to_gray(frames[i], True))
        l, _ = oracle.split_sbs(frames[i], True)
        g = np.ascontiguousarray(l[..., ::-1]).astype(np.float32).mean(axis=2)[::2, ::3].copy()
        if i == 1:
            g[11, 40] = NAN_N
        if i == 2:
            g[30, 7] = np.inf
        blend, _ = _blend_numpy(oracle, d16, g)
        with NF.cast_warnings_are_errors():
            want = TR.to_u16_range(blend[None], TR.minmax(blend[None]))[0]
        got = read_png16(outdir / f"depth_{i:06d}.png")
        assert not mismatch_report(got, want, f"frame {i}")
        if i == 0:
            assert np.array_equal(want, oracle.depth_to_u16(oracle.mono_blend(d16, g))) and want.any()
        if i == 1:
            assert np.array_equal(want, oracle.depth_to_u16(oracle.disp_to_depth(d16))) and want.any()   # stereo only
        if i == 2:
            assert np.isnan(blend).any() and not want.any()                                               # an all-zero frame


# ---------------------------------------------------------------- the audio entries inside a guard arena

AUDIO_N1, AUDIO_N2 = 3000, 3500


def _audio_arena(lib, out_dtype, out_n, poison):
    a = Arena("cuda", poison)
    b1 = a.buf("a1", "in", np.float32, (AUDIO_N1,))
    b2 = a.buf("a2", "in", np.float32, (AUDIO_N2,))
    bo = a.buf("out", "out", out_dtype, (out_n,), align=8)
    ws = a.buf("ws", "ws", np.uint8, (int(lib.v3d_xcorr_ws_bytes(AUDIO_N1, AUDIO_N2)),), align=16)
    return a, b1, b2, bo, ws


def _audio_cases():
    """(label, a1, a2, finite1, finite2): a NaN, +inf or -inf at the first, a middle and the last sample of a1, of a2, of both"""
    rng = np.random.default_rng(21)
    base = rng.standard_normal(AUDIO_N2 + 400).astype(np.float32)
    c2 = base[:AUDIO_N2].copy()
    c1 = (base[137:137 + AUDIO_N1] + 0.05 * rng.standard_normal(AUDIO_N1)).astype(np.float32)
    yield "clean", c1, c2, True, True
    for k, name in enumerate(("nan+", "nan-", "+inf", "-inf")):
        for pos in ("first", "middle", "last"):
            for in1, in2 in ((True, False), (False, True), (True, True)):
                a1, a2 = c1.copy(), c2.copy()
                for on, a in ((in1, a1), (in2, a2)):
                    if on:
                        a[{"first": 0, "middle": a.size // 2 + k, "last": a.size - 1}[pos]] = NF.SPECIALS[name]
                yield f"{name} at the {pos} sample of {'a1' if in1 else ''}{' and ' if in1 and in2 else ''}{'a2' if in2 else ''}", a1, a2, not in1, not in2


@pytest.mark.parametrize("poison", [0xA5, 0x00])
def test_audio_entries_with_non_finite_samples(native, poison):
    """v3d_xcorr and v3d_align_audio at (3000, 3500), tracks, out / result and ws inside guard arenas.  Both return V3D_OK and
    write nothing outside out / result / ws.  v3d_xcorr: every output is NaN (a transform spreads a NaN over every bin, and an
    infinity meets 0 * inf or inf - inf on the way).  v3d_align_audio: a NaN never wins the block maxima's `v > best`, so no lag is
    nominated: lag = 0, c = 0 and strength = 0 exactly, and result[3] is the finite track's std, NaN when neither is finite."""
    lib = native.lib()
    P = lambda b: C.c_void_p(b.ptr)                                  # noqa: E731
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    ax, x1, x2, xo, xw = _audio_arena(lib, np.float32, AUDIO_N1 + AUDIO_N2 - 1, poison)
    aa, r1, r2, ro, rw = _audio_arena(lib, np.float64, 4, poison)
    for label, a1, a2, fin1, fin2 in _audio_cases():
        x1.set(a1), x2.set(a2), r1.set(a1), r2.set(a2)
        ax.fill().snapshot()
        assert lib.v3d_xcorr(P(x1), a1.size, P(x2), a2.size, P(xo), P(xw), st()) == 0, label
        torch.cuda.synchronize()
        ax.check()
        aa.fill().snapshot()
        assert lib.v3d_align_audio(P(r1), a1.size, P(r2), a2.size, P(ro), P(rw), st()) == 0, label
        torch.cuda.synchronize()
        aa.check()
        out, res = xo.get(), ro.get()
        sd = [float(np.std(a.astype(np.float64))) if fin else None for a, fin in ((a1, fin1), (a2, fin2))]
        if fin1 and fin2:
            assert np.isfinite(out).all() and res[0] == 137 and res[2] > 0.9 and abs(res[3] - min(sd)) <= 1e-9 * min(sd), label
            continue
        assert np.isnan(out).all(), (label, int((~np.isnan(out)).sum()), np.flatnonzero(~np.isnan(out))[:4].tolist())
        assert res[0] == 0 and res[1] == 0 and res[2] == 0, (label, res.tolist())
        want = sd[0] if fin1 else sd[1] if fin2 else None
        assert np.isnan(res[3]) if want is None else abs(res[3] - want) <= 1e-9 * want, (label, res.tolist(), want)
