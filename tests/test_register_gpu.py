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
    if kind == "top":
        return np.full((K, n), TOP, np.uint32)
    if kind == "alt":
        return np.tile(np.where(np.arange(n) % 2 == 0, 0, TOP).astype(np.uint32), (K, 1))
    return np.random.default_rng(seed).integers(0, TOP + 1, (K, n)).astype(np.uint32)


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
