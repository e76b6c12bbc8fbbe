"""csrc/v3d_register.hip itself, without a GPU: the kernel source runs in the stand-alone emulator driver (tests/emu_case.py),
plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal tests/register_ref.py bit for bit.  What the file
has that no other emulated source has: workgroups of 1024 threads, LDS atomics, a 4096-word `rowp` sized exactly to R * nseg,
packed 16-bit column sums that hold exactly 256 * 255, and 8-byte stores on rows that are only 2-byte aligned.  Shapes, candidate
lists and maps are those of tests/test_register_gpu.py, kept small: the emulator runs 1024 fibers per workgroup."""
import numpy as np
import pytest

import emu_case as E
import register_ref as RR
import test_register_gpu as G

PROFILES, MATCH, WARP = "v3d_plane_profiles_batch", "v3d_profile_match_scores", "v3d_warp_u16_batch"
driver = E.driver_fixture("register", ["v3d_register.hip"],
                          [PROFILES, MATCH, WARP, "v3d_plane_profiles_ws_bytes", "v3d_profile_match_ws_bytes"])


def _u8(a, dtype):
    return np.ascontiguousarray(a, dtype).reshape(-1).view(np.uint8)


def _out(name, want, dtype, skew, gp):
    """an output that starts on its first byte and ends on its last, poisoned; `want` after the call"""
    w = _u8(want, dtype)
    return E.exact(name, np.full(w.size, gp, np.uint8), skew, expect=w)


# ---- profiles ----
def _profiles_case(driver, tmp, g, layout):
    """g u8 [n,H,W].  vector: base, pitch and stride multiples of 16, the plane in exactly its 16-byte blocks; bytes: base + 1, pitch
    W + 3, stride padded by 11, the plane ending on its last payload byte.  The slack holds the global poison (0xFF in one config)"""
    n, H, W = g.shape
    p = G.profile_plan(n, W, H)
    assert E.query(driver, "v3d_plane_profiles_ws_bytes", n, W, H) == 4 * n * p["bands"] * W
    pitch, pad = ((W + 15) // 16 * 16, 16) if layout == "vector" else (W + 3, 11)
    stride = H * pitch + pad
    wc, wr = RR.profiles(g)

    def make(gp):
        img = np.full((n - 1) * stride + (H - 1) * pitch + W, gp, np.uint8)
        for f in range(n):
            for y in range(H):
                img[f * stride + y * pitch:f * stride + y * pitch + W] = g[f, y]
        gray = E.chunked("gray", img, 0, gp) if layout == "vector" else (E.exact("gray", img, 1), 0)
        ws = E.exact("ws", np.full(4 * n * p["bands"] * W, gp, np.uint8), 0, expect=None)
        return [gray, n, W, H, pitch, stride, _out("col", wc, np.uint32, 4, gp), _out("row", wr, np.uint32, 12, gp), ws, 0]
    E.run_configs(driver, tmp, PROFILES, make)


# the last segment holds one whole 16-byte group and one byte of the next; H: one full band, in which every phase takes the
# four-row loop twice, and a ragged one in which the first phase has 4 + 2 rows and the others 4 + 1.  16 / nseg leaves idle waves at
# 3, 5, 6 and 7, and at nseg = 5 .. 8 rowp's index k * nseg + sx walks through all of R * nseg words
@pytest.mark.parametrize("layout", ["vector", "bytes"])
@pytest.mark.parametrize("nseg", [1, 2, 3, 5, 6, 7, 8])
def test_profiles_every_segment_count(driver, tmp_path, nseg, layout):
    W, ny = 1024 * (nseg - 1) + 17, 16 // nseg
    H = 8 * ny + 5 * ny + 1
    p = G.profile_plan(2, W, H)
    assert (p["nseg"], p["ny"], p["L"], p["R"], p["bands"]) == (nseg, ny, 8, 8 * ny, 2)
    g = np.random.default_rng(nseg).integers(0, 256, (2, H, W), dtype=np.uint8)
    g[1, :, W // 2:] = 255
    _profiles_case(driver, tmp_path, g, layout)


def test_profiles_more_than_eight_rows_per_lane(driver, tmp_path):
    """L is set by H * n alone: ceil(H n / (1024 ny)), at least 8.  17 planes of 17 x 8192 give L = 9, bands of 144 rows and a last
    one of 128, on random data with an all-255 half.  L = 256 (a lane's packed 16-bit sums at 256 * 255, rowp filled to its last
    word) needs 4096 * 1021 rows however they are cut into planes: over a thousand workgroups of 1024 fibers, measured at 150 s in
    the plain build and 400 s in the sanitized one, so that plan stays with tests/test_register_gpu.py's test_profiles_headroom"""
    n, H, W = 17, 8192, 17
    p = G.profile_plan(n, W, H)
    assert (p["nseg"], p["ny"], p["L"], p["R"], p["bands"]) == (1, 16, 9, 144, 57) and H - 56 * 144 == 128
    g = np.random.default_rng(17).integers(0, 256, (n, H, W), dtype=np.uint8)
    g[1, :, W // 2:] = 255
    _profiles_case(driver, tmp_path, g, "vector")


# ---- match ----
BAD = [(RR.A_MIN - 1, 0), (RR.A_MAX + 1, 0), (RR.Q, RR.B_MAX + 1), (RR.Q, -RR.B_MAX - 1), (-RR.Q, 0), (1 << 62, 1 << 62)]


# in-headroom samples (nothing wraps) and full-range u32 samples (the products and the sums wrap mod 2^64); the domain's corners are
# in _candidates, the candidates outside it get the in-band refusal
@pytest.mark.parametrize("kind", ["random", "top", "alt", "random32", "top32", "alt32"])
@pytest.mark.parametrize("na,nb,bins", [(23, 31, 8), (64, 100, 64)])
def test_match(driver, tmp_path, na, nb, bins, kind):
    K = 2
    good = G._candidates(na, nb)
    cand = np.concatenate([good[:5], np.array(BAD[:3], np.int64), good[5:], np.array(BAD[3:], np.int64)])
    ok = np.array([tuple(c) not in BAD for c in cand.tolist()])
    a, b = G._profiles(K, na, na + bins, kind), G._profiles(K, nb, nb + 7 * bins, kind)
    want = np.zeros((K, len(cand), RR.FIELDS), np.int64)
    want[:, ~ok, 0] = -1
    want[:, ok] = RR.match_scores_wrapping(a, b, cand[ok], bins)
    if not kind.endswith("32"):
        assert np.array_equal(want[:, ok], RR.match_scores(a, b, cand[ok], bins))
    need = K * (na + nb + 2) * 8
    assert E.query(driver, "v3d_profile_match_ws_bytes", K, na, nb) == need

    def make(gp):
        ws = E.exact("ws", np.full(need, gp, np.uint8), 0, expect=None)
        return [E.exact("a", _u8(a, np.uint32), 4), na, E.exact("b", _u8(b, np.uint32), 12), nb, K, E.exact("cand", _u8(cand, np.int64), 8),
                len(cand), bins, _out("out", want, np.int64, 24, gp), ws, 0]
    E.run_configs(driver, tmp_path, MATCH, make)


# ---- warp ----
# 9 and 131 columns: one workgroup, rows whose lead group takes every length; 1029: the groups of blockIdx.x = 1.  The source ends on
# its last payload byte and starts on its first; the output's skew makes `lead` differ from row to row at the odd widths.  The
# kernel's 8-byte store is a plain store, not st_stream: off its alignment it is UndefinedBehaviorSanitizer's finding in the sanitized
# build ("store to misaligned address"), the driver's `misaligned` counter does not see it
@pytest.mark.parametrize("Ws,Hs,Wo,Ho", [(17, 5, 9, 4), (130, 70, 131, 69), (515, 2, 1029, 3)])
def test_warp(driver, tmp_path, Ws, Hs, Wo, Ho):
    n, fill = 2, 4242
    s = G._planes(n, Hs, Ws, Ws + Hs)
    for k, (name, m) in enumerate(G._maps(Ws, Hs, Wo, Ho).items()):
        want = RR.warp(s, *m, fill, Wo, Ho)
        stride, skews = Ws * Hs + 7 * (k % 2), ((2, 6), (6, 2))[k % 2]

        def make(gp):
            img = np.full((n - 1) * stride + Ws * Hs, gp * 257, np.uint16)
            for f in range(n):
                img[f * stride:f * stride + Ws * Hs] = s[f].reshape(-1)
            return [E.exact("src", _u8(img, np.uint16), skews[0]), n, Ws, Hs, stride, *m, fill, _out("out", want, np.uint16, skews[1], gp),
                    Wo, Ho, 0]
        E.run_configs(driver, tmp_path, WARP, make)
        if name.startswith(("outside", "far")):
            assert (want == fill).all()


# ---- refusals ----
def test_refused_calls_write_nothing(driver, tmp_path):
    """every buffer is expected back as it was"""
    def poisoned(name, nbytes, skew, gp):
        return E.exact(name, np.full(nbytes, gp, np.uint8), skew)

    def profiles(W, H, pitch, n=1, ws_off=0):
        def make(gp):
            return [poisoned("gray", 64, 0, gp), n, W, H, pitch, 64, poisoned("col", 64, 4, gp), poisoned("row", 64, 4, gp),
                    (poisoned("ws", 64, 0, gp), ws_off), 0]
        return make
    for make, rc in ((profiles(8193, 2, 8193), -3), (profiles(2, 8193, 2), -3), (profiles(8, 2, 7), -1), (profiles(0, 2, 8), -1),
                     (profiles(8, 2, 8, n=0), -1), (profiles(8, 2, 8, ws_off=8), -1), (profiles(8, 9, 8, n=2), -1)):       # stride 64 < 9 * 8
        E.run_configs(driver, tmp_path, PROFILES, make, rc=rc)

    def match(na=16, nb=16, K=1, Cn=1, bins=8, cand_off=0):
        def make(gp):
            cand = E.exact("cand", _u8(np.array([[RR.Q, 0], [RR.Q, 0]]), np.int64), 8)
            return [poisoned("a", 64, 4, gp), na, poisoned("b", 64, 4, gp), nb, K, (cand, cand_off), Cn, bins, poisoned("out", 48, 8, gp),
                    poisoned("ws", 512, 0, gp), 0]
        return make
    for make, rc in ((match(bins=7), -1), (match(nb=15, bins=16), -1), (match(K=0), -1), (match(Cn=0), -1), (match(cand_off=4), -1),
                     (match(na=8193), -3), (match(nb=8193), -3)):
        E.run_configs(driver, tmp_path, MATCH, make, rc=rc)

    def warp(m=(RR.Q, 0, RR.Q, 0), n=1, Ws=4, Hs=4, Wo=4, Ho=4, stride=16):
        def make(gp):
            return [poisoned("src", 64, 2, gp), n, Ws, Hs, stride, *m, 7, poisoned("out", 64, 6, gp), Wo, Ho, 0]
        return make
    Q = RR.Q
    for make, rc in ((warp(m=(RR.A_MIN - 1, 0, Q, 0)), -1), (warp(m=(Q, 0, RR.A_MAX + 1, 0)), -1), (warp(m=(Q, RR.WARP_B_MAX + 1, Q, 0)), -1),
                     (warp(m=(Q, 0, Q, -RR.WARP_B_MAX - 1)), -1), (warp(n=2, stride=15), -1), (warp(Wo=0), -1), (warp(Ws=8193), -3),
                     (warp(Wo=8193), -3), (warp(Ho=65536), -3)):
        E.run_configs(driver, tmp_path, WARP, make, rc=rc)
