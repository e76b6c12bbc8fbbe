"""v3d_plane_profiles_batch, v3d_profile_match_scores and v3d_warp_u16_batch against the NumPy restatement
(tests/register_ref.py), bit for bit, at the shapes where a kernel takes another path and at the edges of their domains, and
their refusals."""
import ctypes as C

import numpy as np
import pytest

import register_ref as RR
from conftest import mismatch_report

pytestmark = pytest.mark.gpu
P = C.c_void_p
TOP = (1 << 21) - 1                                             # the largest sample a profile of an 8192-pixel side holds


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- profiles ----
# 1x1; 15x3 / 17x37: one partial 16-byte group, two groups; 64x36: vector loads; 257x300: several bands of a frame;
# 8192x2: eight segments per row, two row phases
@pytest.mark.parametrize("W,H", [(1, 1), (15, 3), (17, 37), (64, 36), (257, 300), (8192, 2)])
def test_profiles_bit_exact(native, W, H):
    g = np.random.default_rng(W * 3 + H).integers(0, 256, (2, H, W), dtype=np.uint8)
    g[1, :, W // 2:] = 255
    col, row = native.plane_profiles_batch(native.to_device(g))
    wc, wr = RR.profiles(g)
    rep = mismatch_report(_u32(col), wc, f"col {W}x{H}") or mismatch_report(_u32(row), wr, f"row {W}x{H}")
    assert not rep, rep


def test_profiles_padded_pitch_stride_and_odd_base(native):
    """253 x 77, n = 3 inside a larger allocation: pitch 260, stride 77 * 260 + 11, odd base pointer -> the byte path; the padding
    holds 255s that must not reach a sum"""
    import torch
    W, H, n, pitch = 253, 77, 3, 260
    stride = H * pitch + 11
    g = np.random.default_rng(5).integers(0, 256, (n, H, W), dtype=np.uint8)
    buf = np.full(1 + n * stride, 255, np.uint8)
    for f in range(n):
        for y in range(H):
            buf[1 + f * stride + y * pitch:1 + f * stride + y * pitch + W] = g[f, y]
    d = native.to_device(buf)
    col = torch.empty((n, W), dtype=torch.int32, device="cuda")
    row = torch.empty((n, H), dtype=torch.int32, device="cuda")
    L = native.lib()
    ws = torch.empty(L.v3d_plane_profiles_ws_bytes(n, W, H), dtype=torch.uint8, device="cuda")
    rc = L.v3d_plane_profiles_batch(P(d.data_ptr() + 1), n, W, H, pitch, stride, P(col.data_ptr()), P(row.data_ptr()), P(ws.data_ptr()),
                                    native._stream())
    assert rc == 0, L.v3d_last_error()
    wc, wr = RR.profiles(g)
    rep = mismatch_report(_u32(col), wc, "padded col") or mismatch_report(_u32(row), wr, "padded row")
    assert not rep, rep


def profile_plan(n, W, H):
    """v3d_register.hip's cut of n planes of W x H, restated: nseg segments of 1024 columns per row, ny row phases per workgroup,
    L rows per lane, bands of R = L * ny rows"""
    nseg = -(-W // 1024)
    ny = 16 // nseg
    L = min(max(-(-H * n // (ny * 1024)), 8), 256)
    return dict(nseg=nseg, ny=ny, L=L, R=L * ny, bands=-(-H // (L * ny)))


def _profiles_strided(native, g, pitch, stride, base):
    """g u8 [n,H,W] laid out with rows `pitch` and frames `stride` bytes apart from byte `base` of an allocation, 255s in all the
    slack, through the entry itself -> (col, row) u32"""
    import torch
    n, H, W = g.shape
    buf = torch.full((base + n * stride,), 255, dtype=torch.uint8, device="cuda")
    buf[base:].unflatten(0, (n, stride))[:, :H * pitch].unflatten(1, (H, pitch))[:, :, :W].copy_(native.to_device(g))
    col = torch.empty((n, W), dtype=torch.int32, device="cuda")
    row = torch.empty((n, H), dtype=torch.int32, device="cuda")
    L = native.lib()
    ws = torch.empty(L.v3d_plane_profiles_ws_bytes(n, W, H), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rc = L.v3d_plane_profiles_batch(P(buf.data_ptr() + base), n, W, H, pitch, stride, P(col.data_ptr()), P(row.data_ptr()), P(ws.data_ptr()),
                                    native._stream())
    assert rc == 0, L.v3d_last_error()
    return _u32(col), _u32(row)


# every segment count; the last segment holds one column, a partial 16-byte group, or is full.  H = R + 5 ny + 1: the first band
# takes the four-row loop twice per phase, the second is ragged: the first phase has 4 + 2 rows, the others 4 + 1.  Each shape on the
# vector route (aligned base, pitch and stride multiples of 16) and on the byte route (base + 1, pitch W + 3, stride padded)
@pytest.mark.parametrize("nseg", [1, 2, 3, 4, 5, 6, 7, 8])
def test_profiles_every_segment_count(native, nseg):
    L = native.lib()
    ny, n = 16 // nseg, 2
    H = 8 * ny + 5 * ny + 1
    for W in (1024 * (nseg - 1) + 1, 1024 * nseg - 15, 1024 * nseg):
        p = profile_plan(n, W, H)
        assert (p["nseg"], p["ny"], p["L"], p["R"], p["bands"]) == (nseg, ny, 8, 8 * ny, 2)
        assert H - p["R"] == 5 * ny + 1 and L.v3d_plane_profiles_ws_bytes(n, W, H) == 4 * n * p["bands"] * W
        g = np.random.default_rng(W).integers(0, 256, (n, H, W), dtype=np.uint8)
        g[1, :, W // 2:] = 255
        wc, wr = RR.profiles(g)
        pitch = (W + 15) // 16 * 16
        for route, (pt, st, base) in (("vector", (pitch, H * pitch + 32, 0)), ("bytes", (W + 3, H * (W + 3) + 11, 1))):
            col, row = _profiles_strided(native, g, pt, st, base)
            rep = mismatch_report(col, wc, f"col {W}x{H} {route}") or mismatch_report(row, wr, f"row {W}x{H} {route}")
            assert not rep, rep
        if W % 16 == 0:                                             # the contiguous tensor of the binding is the vector route too
            col, row = native.plane_profiles_batch(native.to_device(g))
            assert np.array_equal(_u32(col), wc) and np.array_equal(_u32(row), wr)


def test_profiles_more_than_eight_rows_per_lane(native):
    """1025 x 8192, n = 9, random: two segments, eight phases, L = 9 rows per lane, 114 bands of 72 rows, the last with 56"""
    import torch
    n, W, H = 9, 1025, 8192
    p = profile_plan(n, W, H)
    assert (p["nseg"], p["ny"], p["L"], p["R"], p["bands"]) == (2, 8, 9, 72, 114) and H - 113 * 72 == 56
    assert native.lib().v3d_plane_profiles_ws_bytes(n, W, H) == 4 * n * 114 * W
    g = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    col, row = native.plane_profiles_batch(g)
    col, row = _u32(col), _u32(row)
    for f in range(n):                                              # per frame: the reference widens its input to int64
        wc, wr = RR.profiles(g[f:f + 1].cpu().numpy())
        rep = mismatch_report(col[f:f + 1], wc, f"col frame {f}") or mismatch_report(row[f:f + 1], wr, f"row frame {f}")
        assert not rep, rep


def test_profiles_headroom(native):
    """all-255 planes: 64 x 8192 reaches the largest column sum, 255 * 8192, through many bands; 512 planes of 1 x 8192 make a
    lane sum 256 rows, 255 * 256 = 65280, in a packed 16-bit field before it is widened"""
    import torch
    g = torch.full((1, 8192, 64), 255, dtype=torch.uint8, device="cuda")
    col, row = native.plane_profiles_batch(g)
    assert (_u32(col) == 255 * 8192).all() and (_u32(row) == 255 * 64).all()
    g = torch.full((512, 8192, 1), 255, dtype=torch.uint8, device="cuda")
    col, row = native.plane_profiles_batch(g)
    assert (_u32(col) == 255 * 8192).all() and (_u32(row) == 255).all()


def test_profiles_product_shape(native):
    """3840 x 2160, n = 2: the 4K luma (four segments, four row phases, 16-byte loads)"""
    import torch
    g = torch.randint(0, 256, (2, 2160, 3840), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    col, row = native.plane_profiles_batch(g)
    wc, wr = RR.profiles(g.cpu().numpy())
    rep = mismatch_report(_u32(col), wc, "col 3840x2160") or mismatch_report(_u32(row), wr, "row 3840x2160")
    assert not rep, rep


def test_profiles_refusals(native):
    import torch
    L = native.lib()
    g = torch.zeros(4 * 128 * 72, dtype=torch.uint8, device="cuda")
    col = torch.full((2, 128), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    row = torch.full((2, 72), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    st = native._stream()

    def call(n, W, H, pitch, stride, gp=g.data_ptr(), cp=col.data_ptr(), rp=row.data_ptr(), wp=ws.data_ptr()):
        return L.v3d_plane_profiles_batch(P(gp), n, W, H, pitch, stride, P(cp), P(rp), P(wp), st)
    for W, H in ((8193, 36), (64, 8193)):
        assert call(1, W, H, W, W * H) == -3 and L.v3d_plane_profiles_ws_bytes(1, W, H) == 0           # V3D_ERR_UNSUPPORTED
    assert call(1, 0, 72, 128, 0) == -1 and call(1, 128, 0, 128, 0) == -1
    assert call(1, 128, 72, 127, 128 * 72) == -1 and b"pitch" in L.v3d_last_error()
    assert call(2, 128, 72, 128, 128 * 72 - 1) == -1 and b"stride" in L.v3d_last_error()
    assert call(0, 128, 72, 128, 128 * 72) == -1 and call(65536, 128, 72, 128, 128 * 72) == -1
    assert L.v3d_plane_profiles_ws_bytes(0, 128, 72) == 0 and L.v3d_plane_profiles_ws_bytes(65536, 128, 72) == 0
    for kw in ("gp", "cp", "rp", "wp"):
        assert call(1, 128, 72, 128, 0, **{kw: None}) == -1
    assert call(1, 128, 72, 128, 0, wp=ws.data_ptr() + 8) == -1                                       # ws 16 bytes
    torch.cuda.synchronize()
    assert (col.cpu().numpy() == 0x5A5A5A5A).all() and (row.cpu().numpy() == 0x5A5A5A5A).all()
    assert call(1, 128, 72, 128, 0) == 0                                                              # n == 1 ignores the stride
    torch.cuda.synchronize()


# ---- match ----
def _profiles(K, n, seed, kind):
    """kind random / top / alt: samples up to TOP, inside the record's headroom; random32 / top32 / alt32: up to 2^32 - 1"""
    top = 0xFFFFFFFF if kind.endswith("32") else TOP
    if kind.startswith("top"):
        return np.full((K, n), top, np.uint32)
    if kind.startswith("alt"):
        return np.tile(np.where(np.arange(n) % 2 == 0, 0, top).astype(np.uint32), (K, 1))
    return np.random.default_rng(seed).integers(0, top + 1, (K, n)).astype(np.uint32)


def _candidates(na, nb):
    """the nominal map and its neighbours (all bins valid), shifted and scaled maps (some), maps wholly outside the source (none)
    and the corners of the (a, b) domain"""
    nom = RR.rhu(RR.Fraction(na * RR.Q, nb))
    c = [(nom, 0), (max(nom - 1, RR.A_MIN), 0), (nom, 12345), (nom, -54321), (nom * 3 // 4 + 1, na * RR.Q // 8), (min(nom * 5 // 4, RR.A_MAX), -na * RR.Q // 7),
         (nom, na * RR.Q), (nom, -RR.B_MAX), (nom, RR.B_MAX), (RR.A_MIN, 0), (RR.A_MIN, RR.B_MAX), (RR.A_MIN, -RR.B_MAX),
         (RR.A_MAX, 0), (RR.A_MAX, RR.B_MAX), (RR.A_MAX, -RR.B_MAX), (RR.A_MIN, 7 * RR.Q + 1), (nom, 1), (nom, -1)]
    c = [(min(max(a, RR.A_MIN), RR.A_MAX), b) for a, b in c]
    return np.array(c, dtype=np.int64)


# every (na, nb) x bins of {(23, 31), (256, 512), (8192, 8192)} x {8, 512, 1024} the entry accepts (nb >= bins)
@pytest.mark.parametrize("na,nb,bins", [(23, 31, 8), (256, 512, 8), (256, 512, 512), (8192, 8192, 8), (8192, 8192, 512), (8192, 8192, 1024)])
def test_match_bit_exact(native, na, nb, bins):
    cand = _candidates(na, nb)
    # random; 2^21 - 1 everywhere in both (the largest prefix sums) and in the source alone; alternating 0 / 2^21 - 1 (the largest differences)
    for kind, kind_b in (("random", "random"), ("top", "top"), ("top", "random"), ("alt", "alt")):
        a, b = _profiles(2, na, na + bins, kind), _profiles(2, nb, nb + 7 * bins, kind_b)
        got = native.profile_match_scores(native.to_device(a.view(np.int32)), native.to_device(b.view(np.int32)), cand, bins).cpu().numpy()
        want = RR.match_scores(a, b, cand, bins)
        assert got.shape == want.shape == (2, len(cand), 6)
        assert np.array_equal(got, want), f"{kind} {na}->{nb} bins {bins}: records {np.argwhere((got != want).any(axis=2)).tolist()[:6]} differ"
        n_pairs = want[0, :, 0]
        if kind == "random":
            assert n_pairs.max() == bins - 1 and n_pairs.min() == 0 and ((n_pairs > 0) & (n_pairs < bins - 1)).any()


# samples of 2^21 and above "are legal memory-wise and wrap in the record": da and db reach +-(2^32 - 1), their products 2^64
@pytest.mark.parametrize("na,nb,bins", [(23, 31, 8), (256, 512, 512)])
def test_match_wraps_with_full_range_samples(native, na, nb, bins):
    cand = _candidates(na, nb)
    for kind, kind_b in (("random32", "random32"), ("top32", "top32"), ("top32", "random32"), ("alt32", "alt32"), ("alt32", "random32")):
        a, b = _profiles(2, na, na + bins, kind), _profiles(2, nb, nb + 7 * bins, kind_b)
        got = native.profile_match_scores(native.to_device(a.view(np.int32)), native.to_device(b.view(np.int32)), cand, bins).cpu().numpy()
        want = RR.match_scores_wrapping(a, b, cand, bins)
        assert np.array_equal(got, want), f"{kind} {na}->{nb} bins {bins}: records {np.argwhere((got != want).any(axis=2)).tolist()[:6]} differ"


def test_match_refuses_candidates_outside_the_domain(native):
    """a host-side list is refused before anything is enqueued; a device-side list (which the entry cannot read) gets the in-band
    refusal (-1, 0, 0, 0, 0, 0) per offending candidate, the others their record"""
    import torch
    a, b = _profiles(2, 64, 1, "random"), _profiles(2, 64, 2, "random")
    A, B = native.to_device(a.view(np.int32)), native.to_device(b.view(np.int32))
    bad = np.array([(RR.Q, 0), (RR.A_MIN - 1, 0), (RR.A_MAX + 1, 0), (RR.Q, RR.B_MAX + 1), (RR.Q, -RR.B_MAX - 1), (-RR.Q, 0),
                    (1 << 62, 1 << 62)], dtype=np.int64)
    with pytest.raises(ValueError):
        native.profile_match_scores(A, B, bad, 8)
    got = native.profile_match_scores(A, B, torch.from_numpy(bad).cuda(), 8).cpu().numpy()
    assert np.array_equal(got[:, 0], RR.match_scores(a, b, bad[:1], 8)[:, 0])
    assert (got[:, 1:, 0] == -1).all() and (got[:, 1:, 1:] == 0).all()


def test_match_refusals(native):
    import torch
    L = native.lib()
    p = torch.zeros((2, 64), dtype=torch.int32, device="cuda")
    cand = torch.tensor([[65536, 0]], dtype=torch.int64, device="cuda")
    out = torch.full((2, 1, 6), 7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    st = native._stream()

    def call(na=64, nb=64, K=2, Cn=1, bins=8, ap=p.data_ptr(), bp=p.data_ptr(), cp=cand.data_ptr(), op=out.data_ptr(), wp=ws.data_ptr()):
        return L.v3d_profile_match_scores(P(ap), na, P(bp), nb, K, P(cp), Cn, bins, P(op), P(wp), st)
    for kw in (dict(K=0), dict(K=4097), dict(Cn=0), dict(Cn=65536), dict(na=0), dict(nb=0), dict(bins=7), dict(bins=1025),
               dict(nb=63, bins=64), dict(ap=None), dict(bp=None), dict(cp=None), dict(op=None), dict(wp=None),
               dict(wp=ws.data_ptr() + 8), dict(cp=cand.data_ptr() + 4), dict(op=out.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    assert call(na=8193) == -3 and call(nb=8193, bins=8) == -3
    assert L.v3d_profile_match_ws_bytes(0, 64, 64) == 0 and L.v3d_profile_match_ws_bytes(1, 8193, 64) == 0
    assert L.v3d_profile_match_ws_bytes(2, 64, 32) == 2 * (64 + 32 + 2) * 8
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all()


# ---- warp ----
def _planes(n, H, W, seed):
    s = np.random.default_rng(seed).integers(0, 65536, (n, H, W)).astype(np.uint16)
    s[0, 0, 0], s[-1, -1, -1] = 65535, 0
    return s


def _warp(native, s, m, Wo, Ho, fill=0):
    return native.warp_u16_batch(native.to_device(s.view(np.int16)), *m, Wo, Ho, fill).cpu().numpy().view(np.uint16)


def _maps(Ws, Hs, Wo, Ho):
    Q = RR.Q
    return {"identity": (Q, 0, Q, 0), "integer shift": (Q, 3 * Q, Q, -2 * Q), "half-pixel shift": (Q, Q // 2, Q, -Q // 2),
            "fit": (RR.rhu(RR.Fraction(Ws * Q, Wo)), RR.rhu(RR.Fraction((Ws - Wo) * Q, 2 * Wo)), RR.rhu(RR.Fraction(Hs * Q, Ho)), RR.rhu(RR.Fraction((Hs - Ho) * Q, 2 * Ho))),
            "outside": (Q, Ws * Q, Q, 0), "outside rows": (Q, 0, Q, -(Ho + 1) * Q), "ax min": (RR.A_MIN, 5 * Q + 77, Q // 3, 99),
            "ax max": (RR.A_MAX, -3 * Q, RR.A_MAX, -Q), "last column": (Q, (Ws - Wo) * Q, Q, (Hs - Ho) * Q),
            "one past": (Q, (Ws - Wo) * Q + 1, Q, (Hs - Ho) * Q + 1), "far": (Q, RR.WARP_B_MAX, Q, -RR.WARP_B_MAX)}


@pytest.mark.parametrize("Ws,Hs,Wo,Ho", [(1, 1, 1, 1), (17, 5, 9, 4), (130, 70, 131, 69), (9, 4, 17, 5)])
def test_warp_bit_exact(native, Ws, Hs, Wo, Ho):
    s = _planes(2, Hs, Ws, Ws + Hs)
    for name, m in _maps(Ws, Hs, Wo, Ho).items():
        got, want = _warp(native, s, m, Wo, Ho, 4242), RR.warp(s, *m, 4242, Wo, Ho)
        rep = mismatch_report(got, want, f"warp {Ws}x{Hs} -> {Wo}x{Ho} {name}")
        assert not rep, rep
        if name.startswith(("outside", "far")):
            assert (got == 4242).all()


def test_warp_identity_is_a_copy(native):
    s = _planes(3, 70, 131, 9)
    assert np.array_equal(_warp(native, s, (RR.Q, 0, RR.Q, 0), 131, 70), s)


def test_warp_padded_stride_at_an_odd_element_offset(native):
    """n = 3, frames 130 x 70 at an odd element offset and 130 * 70 + 7 elements apart, the output at an odd element offset as
    well; the padding holds 65535s"""
    import torch
    Ws, Hs, Wo, Ho, n = 130, 70, 131, 69, 3
    stride = Ws * Hs + 7
    s = _planes(n, Hs, Ws, 21)
    buf = np.full(1 + n * stride, 65535, np.uint16)
    for f in range(n):
        buf[1 + f * stride:1 + f * stride + Ws * Hs] = s[f].reshape(-1)
    d = native.to_device(buf.view(np.int16))
    out = torch.full((1 + n * Ho * Wo + 1,), 0x5A5A, dtype=torch.int16, device="cuda")
    m = _maps(Ws, Hs, Wo, Ho)["fit"]
    L = native.lib()
    rc = L.v3d_warp_u16_batch(P(d.data_ptr() + 2), n, Ws, Hs, stride, *m, 7, P(out.data_ptr() + 2), Wo, Ho, native._stream())
    assert rc == 0, L.v3d_last_error()
    o = out.cpu().numpy().view(np.uint16)
    rep = mismatch_report(o[1:-1].reshape(n, Ho, Wo), RR.warp(s, *m, 7, Wo, Ho), "padded warp")
    assert not rep, rep
    assert o[0] == 0x5A5A and o[-1] == 0x5A5A


# a workgroup holds a lead group of 0 .. 3 pixels and 255 (blockIdx.x > 0: 256) groups of four: 1020 is the widest row of one
# workgroup at lead 0, 1021 .. 1023 are with a lead, 1024 and 1025 need the second workgroup at every lead, 2047 a third, 3840 is
# the product's.  Dense: rows at 8-byte multiples where Wo is a multiple of 4; at element offset 1 the lead takes all of 0 .. 3 over
# the rows of the odd widths
@pytest.mark.parametrize("Wo", [1020, 1021, 1022, 1023, 1024, 1025, 2047, 3840])
def test_warp_workgroup_seams(native, Wo):
    import torch
    Ho, n, Ws, Hs = 3, 2, (Wo + 1) // 2, 2
    s = _planes(n, Hs, Ws, Wo)
    d = native.to_device(s.view(np.int16))
    L, maps = native.lib(), _maps(Ws, Hs, Wo, Ho)
    for off in (4, 1):
        out = torch.empty((off + n * Ho * Wo + 4,), dtype=torch.int16, device="cuda")
        assert out.data_ptr() % 8 == 0
        if off == 1 and Wo % 2:
            assert {((out.data_ptr() + 2 * (off + r * Wo)) % 8) // 2 for r in range(n * Ho)} == {0, 1, 2, 3}
        for name in ("fit", "half-pixel shift", "one past"):
            out.fill_(0x5A5A)
            rc = L.v3d_warp_u16_batch(P(d.data_ptr()), n, Ws, Hs, Ws * Hs, *maps[name], 4242, P(out.data_ptr() + 2 * off), Wo, Ho, native._stream())
            assert rc == 0, L.v3d_last_error()
            o = out.cpu().numpy().view(np.uint16)
            rep = mismatch_report(o[off:-4].reshape(n, Ho, Wo), RR.warp(s, *maps[name], 4242, Wo, Ho), f"warp -> {Wo}x{Ho} {name} offset {off}")
            assert not rep, rep
            assert (o[:off] == 0x5A5A).all() and (o[-4:] == 0x5A5A).all()


def test_warp_refusals(native):
    import torch
    L = native.lib()
    s = torch.zeros(4 * 64 * 36, dtype=torch.int16, device="cuda")
    out = torch.full((2, 36, 64), 0x5A5A, dtype=torch.int16, device="cuda")
    st, Q = native._stream(), RR.Q

    def call(n=2, Ws=64, Hs=36, stride=64 * 36, m=(Q, 0, Q, 0), Wo=64, Ho=36, sp=s.data_ptr(), op=out.data_ptr()):
        return L.v3d_warp_u16_batch(P(sp), n, Ws, Hs, stride, *m, 0, P(op), Wo, Ho, st)
    for kw in (dict(n=0), dict(n=65536), dict(Ws=0), dict(Hs=0), dict(Wo=0), dict(Ho=0), dict(stride=64 * 36 - 1), dict(sp=None), dict(op=None),
               dict(m=(RR.A_MIN - 1, 0, Q, 0)), dict(m=(RR.A_MAX + 1, 0, Q, 0)), dict(m=(Q, 0, RR.A_MIN - 1, 0)), dict(m=(Q, 0, RR.A_MAX + 1, 0)),
               dict(m=(Q, RR.WARP_B_MAX + 1, Q, 0)), dict(m=(Q, 0, Q, -RR.WARP_B_MAX - 1)),
               dict(op=s.data_ptr() + 2 * 64 * 36), dict(n=1, op=s.data_ptr() + 2 * (64 * 36 - 1))):            # out overlaps src
        assert call(**kw) == -1, kw
    for kw in (dict(Ws=8193), dict(Wo=8193), dict(Hs=65536), dict(Ho=65536)):
        assert call(**kw) == -3, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all()
    assert call(n=1, stride=0) == 0                                                                   # n == 1 ignores the stride
    torch.cuda.synchronize()
