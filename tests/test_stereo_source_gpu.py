"""v3d_render_stereo_source_batch (the DIBR step with the disocclusions sampled from the SBS frame's stored eye) on the MI355X,
bit for bit against the NumPy restatement (tests/stereo_source_ref.py), both renderers, and its argument checks.

Frame sizes: the smallest frames, a run that ends inside a thread, the half layouts' even sizes, more than one thread run, and one
width for each of the wider pixels-per-thread instantiations (16 above 2048, 32 above 4096), plus tests/stereo_ref.py's scene whose
holes are longer than a wave's run.  Eye sources of 6 x 2, 322 x 45 and 960 x 270 (Ws x Hs); maps that enlarge, that reduce
(ax > 65536) and whose offsets clamp on every side."""
import ctypes as C

import numpy as np
import pytest
import torch

import stereo_pack_ref as P
import stereo_ref as R
import stereo_source_ref as X
import test_stereo_gpu as T

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 3), (255, 5), (254, 6), (1000, 4), (2050, 3), (4100, 2)]
SOURCES = [(6, 2), (322, 45), (960, 270)]
# enlarge, reduce, left / top clamp with a fractional scale, right / bottom clamp at the extremes of the legal map
MAPS = [(21845, -9000, 30000, 77), (200000, 3 << 16, 150000, -(2 << 16)), (65536, -(900 << 16), 4096, -(1 << 40)),
        (1 << 20, 1 << 40, 1 << 20, 1 << 40), (65536, 0, 65536, 0)]


def _sbs(Ws, Hs, seed):
    return np.random.default_rng(seed).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)


def _gpu(native, F, D, gains, packing, sub, sbs, fill, m):
    f = torch.from_numpy(np.ascontiguousarray(F)[None]).cuda()
    d = torch.from_numpy(np.ascontiguousarray(D).view(np.int16)[None]).cuda()
    s = None if sbs is None else torch.from_numpy(sbs[None]).cuda()
    return native.render_stereo_source_batch(f, d, *gains, packing, s, fill, *m, subpixel=sub)[0].cpu().numpy()


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_fills_sources_and_maps(native, W, H, sub):
    F = np.random.default_rng(W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    packs = [p for p in P.PACKINGS if not (p == P.HALF_SBS and W % 2) and not (p == P.HALF_TB and H % 2)]
    k = SIZES.index((W, H))
    for fill in range(4):
        gains = [R.stereo_gains(24, 0.5, 0.5), R.stereo_gains(48, 0.5, 0.0), R.stereo_gains(510, 0.5, 0.5),
                 (W * 256 + 77, -(W * 256 + 77), 0)][(fill + k) % 4]
        D = T._depth(("planar", "noise")[(fill + k) % 2], H, W, W + H + fill)
        sbs = _sbs(*SOURCES[(fill + k) % 3], fill + k)
        m = MAPS[(fill + k + int(sub)) % len(MAPS)]
        packing = packs[(fill + 2 * k + int(sub)) % len(packs)]
        got = _gpu(native, F, D, gains, packing, sub, sbs, fill, m)
        T._check(got, X.render(F, D, *gains, packing, sub, sbs, fill, *m), f"{W}x{H} {P.NAMES[packing]} sub={sub} fill={fill} map={m}")


@pytest.mark.parametrize("sub", [False, True])
def test_every_packing(native, sub):
    """all seven packings at 254 x 6, both eyes filled"""
    W, H = 254, 6
    F = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    D, sbs, gains = T._depth("planar", H, W, 9), _sbs(322, 45, 1), R.stereo_gains(60, 0.5, 0.5)
    EL, ER = X.eyes(F, D, *gains, sub, sbs, 3, *MAPS[0])
    assert (EL != P.eyes(F, D, *gains, sub)[0]).any()          # the fill does change the eyes
    for packing in P.PACKINGS:
        T._check(_gpu(native, F, D, gains, packing, sub, sbs, 3, MAPS[0]), P.pack(EL, ER, packing), f"{P.NAMES[packing]} sub={sub}")


# ---- every instantiation of the march with a source: pixels per thread (8 up to 2048, 16 up to 4096, 32 above) x renderer x what
# becomes of the eye colours.  test_every_packing has the 8-pixel ones; the wide ones run at H = 6 (a band of four rows and a ragged
# one holding one row pair), which allows every packing
K_OF = {P.FULL_SBS: "sbs", P.HALF_SBS: "sbs", P.FULL_TB: "tb", P.HALF_TB: "htb", P.ROWS: "rows", P.ANAGLYPH_COLOUR: "ana",
        P.ANAGLYPH_DUBOIS: "ana"}
WIDE_SIZES = [(2050, 6), (4100, 6)]
# (packing, fill_eyes): both eyes filled in all seven packings, one eye in two packings each
WIDE_CASES = [(p, 3) for p in P.PACKINGS] + [(P.FULL_SBS, 1), (P.ANAGLYPH_COLOUR, 1), (P.HALF_TB, 2), (P.ROWS, 2)]


def _ppt(W):
    return 8 if W <= 2048 else 16 if W <= 4096 else 32


def test_every_source_instantiation_is_launched():
    """the 3 x 2 x 5 = 30 instantiations k_render_stereo<PPT, SUB, K, StSource> against the cases of test_every_packing (254 x 6,
    all seven packings, both renderers) and of test_every_wide_instantiation"""
    cases = {(_ppt(254), sub, K_OF[p]) for sub in (False, True) for p in P.PACKINGS}
    cases |= {(_ppt(W), sub, K_OF[p]) for W, _ in WIDE_SIZES for sub in (False, True) for p, _ in WIDE_CASES}
    assert cases == {(ppt, sub, k) for ppt in (8, 16, 32) for sub in (False, True) for k in ("sbs", "tb", "htb", "rows", "ana")}
    assert len(cases) == 30
    for W, H in WIDE_SIZES:                                        # every packing is legal at the wide sizes
        for p, _ in WIDE_CASES:
            P.output_size(p, W, H)


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("W,H", WIDE_SIZES)
def test_every_wide_instantiation(native, W, H, sub):
    F = np.random.default_rng(W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    D, sbs, gains = T._depth("planar", H, W, W + 9), _sbs(322, 45, 1), R.stereo_gains(60, 0.5, 0.5)
    plain = P.eyes(F, D, *gains, sub)
    eyes = {fill: X.eyes(F, D, *gains, sub, sbs, fill, *MAPS[0]) for fill in (1, 2, 3)}
    for fill, (EL, ER) in eyes.items():                            # the fill changes the eyes it names, and only those
        assert (EL != plain[0]).any() == bool(fill & 1) and (ER != plain[1]).any() == bool(fill & 2)
    for packing, fill in WIDE_CASES:
        T._check(_gpu(native, F, D, gains, packing, sub, sbs, fill, MAPS[0]), P.pack(*eyes[fill], packing),
                 f"{W}x{H} {P.NAMES[packing]} sub={sub} fill={fill}")


# ---- the widest row at the worst alignment: the row staging in LDS is sized to the byte for 8192 pixels whose BGR row starts at
# byte 15 of a 16-byte block (1537 chunks) and whose depth row starts at byte 14 (1025 chunks), the parked words right behind.
# 3 * 8192 and 2 * 8192 are multiples of 16: every row of every frame has these offsets
@pytest.mark.parametrize("source", [False, True])
@pytest.mark.parametrize("sub", [False, True])
def test_widest_row_at_the_worst_alignment(native, sub, source):
    W, n = 8192, 2
    rng = np.random.default_rng(15 + sub)
    sbs, gains = np.stack([_sbs(322, 45, 5 + i) for i in range(n)]), R.stereo_gains(60, 0.5, 0.5)
    s = torch.from_numpy(sbs).cuda()
    # FULL_SBS: dynamic LDS; HALF_SBS; HALF_TB at H = 6: parks packed rows; ANAGLYPH_DUBOIS: the largest static LDS
    for packing, H in ((P.FULL_SBS, 5), (P.HALF_SBS, 5), (P.HALF_TB, 6), (P.ANAGLYPH_DUBOIS, 5)):
        F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        D = np.stack([T._depth(("planar", "noise")[i], H, W, 100 + i + H) for i in range(n)])
        per = H * W * 3
        cap = torch.full((n + 1, per + 48), 7, dtype=torch.uint8, device="cuda")
        frames = cap.flatten()[15:15 + n * (per + 48)].unflatten(0, (n, per + 48))[:, :per].unflatten(1, (H, W, 3))
        frames.copy_(torch.from_numpy(F).cuda())
        dcap = torch.zeros(n * H * W + 16, dtype=torch.int16, device="cuda")
        depth = dcap[7:7 + n * H * W].unflatten(0, (n, H, W))
        depth.copy_(torch.from_numpy(D.view(np.int16)).cuda())
        assert cap.data_ptr() % 16 == 0 and frames.data_ptr() % 16 == 15 and frames.stride(0) == per + 48 and frames.stride(1) == 3 * W
        assert dcap.data_ptr() % 16 == 0 and depth.data_ptr() % 16 == 14 and depth.is_contiguous()
        if source:
            got = native.render_stereo_source_batch(frames, depth, *gains, packing, s, 3, *MAPS[0], subpixel=sub).cpu().numpy()
        else:
            got = native.render_stereo_packed_batch(frames, depth, *gains, packing, subpixel=sub).cpu().numpy()
        for i in range(n):
            want = (X.render(F[i], D[i], *gains, packing, sub, sbs[i], 3, *MAPS[0]) if source else P.render(F[i], D[i], *gains, packing, sub))
            T._check(got[i], want, f"8192x{H} {P.NAMES[packing]} sub={sub} source={source} frame {i}")


@pytest.mark.parametrize("sub", [False, True])
def test_holes_longer_than_a_waves_run(native, sub):
    F, D, gains = R.far_key_scene()
    sbs = _sbs(960, 270, 2)
    for fill, m in ((1, MAPS[0]), (2, MAPS[1]), (3, (15360, -3000, 1 << 20, 0))):
        T._check(_gpu(native, F, D, gains, P.FULL_SBS, sub, sbs, fill, m), X.render(F, D, *gains, P.FULL_SBS, sub, sbs, fill, *m),
                 f"far keys sub={sub} fill={fill}")


@pytest.mark.parametrize("Hs", [32768, 32769, 40000])
def test_rows_beyond_2_to_the_31_in_q16(native, Hs):
    """Hs has no bound, and (Hs - 1) << 16 passes 2^31 from Hs = 32769 on: the bottom clamp at by = 2^40 and a blend of the last
    rows, on an SBS frame two pixels wide"""
    rng = np.random.default_rng(Hs)
    W, H = 255, 5
    F = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    sbs = rng.integers(0, 256, (Hs, 2, 3), dtype=np.uint8)
    gains = R.stereo_gains(510, 0.5, 0.5)
    for sub in (False, True):
        D = T._depth("noise", H, W, Hs + sub)
        for m in ((65536, 0, 65536, 1 << 40), (4096, 0, 1 << 20, ((Hs - 6) << 16) + 32768)):
            T._check(_gpu(native, F, D, gains, P.FULL_SBS, sub, sbs, 3, m), X.render(F, D, *gains, P.FULL_SBS, sub, sbs, 3, *m),
                     f"Hs={Hs} sub={sub} map={m}")


def test_no_eye_filled_is_the_packed_entry_and_needs_no_source(native):
    H, W, n = 6, 334, 2
    rng = np.random.default_rng(8)
    f = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).cuda()
    d = torch.from_numpy(np.stack([T._depth("planar", H, W, 100 + i) for i in range(n)]).view(np.int16)).cuda()
    s = torch.from_numpy(np.stack([_sbs(6, 2, i) for i in range(n)])).cuda()
    gains = R.stereo_gains(80, 0.4, 0.3)
    for sub in (False, True):
        for packing in P.PACKINGS:
            want = native.render_stereo_packed_batch(f, d, *gains, packing, subpixel=sub)
            assert torch.equal(native.render_stereo_source_batch(f, d, *gains, packing, s, 0, *MAPS[0], subpixel=sub), want)
            assert torch.equal(native.render_stereo_source_batch(f, d, *gains, packing, None, 0, *MAPS[0], subpixel=sub), want)


def test_batch_equals_single_calls_and_padded_strides(native):
    H, W, n, Ws, Hs = 6, 333, 3, 322, 45
    rng = np.random.default_rng(8)
    F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([T._depth("noise" if i % 2 else "planar", H, W, 100 + i) for i in range(n)])
    sbs = np.stack([_sbs(Ws, Hs, 40 + i) for i in range(n)])
    f, d, s = torch.from_numpy(F).cuda(), torch.from_numpy(D.view(np.int16)).cuda(), torch.from_numpy(sbs).cuda()
    gains, m = R.stereo_gains(80, 0.4, 0.3), MAPS[0]
    per, pitch = H * W * 3, Ws * 3 + 5
    cap = torch.full((n + 2, per + 45), 7, dtype=torch.uint8, device="cuda")       # frames at an odd byte offset, a padded stride
    frames = cap[:n, 5:5 + per].unflatten(1, (H, W, 3))
    frames.copy_(f)
    scap = torch.full((n + 1, Hs * pitch + 9), 7, dtype=torch.uint8, device="cuda")  # SBS: odd offset, pitched rows, padded frames
    src = scap[:n, 3:3 + Hs * pitch].unflatten(1, (Hs, pitch))[:, :, :Ws * 3].unflatten(2, (Ws, 3))
    src.copy_(s)
    assert frames.stride(0) == per + 45 and src.stride(1) == pitch and src.stride(0) == Hs * pitch + 9 and src.data_ptr() % 2
    for k, packing in enumerate((P.FULL_SBS, P.HALF_TB, P.ANAGLYPH_DUBOIS, P.ROWS)):
        sub, fill = bool(k % 2), (3, 2, 1, 3)[k]
        batch = native.render_stereo_source_batch(f, d, *gains, packing, s, fill, *m, subpixel=sub).cpu().numpy()
        for i in range(n):
            single = native.render_stereo_source_batch(f[i:i + 1], d[i:i + 1].contiguous(), *gains, packing, s[i:i + 1], fill, *m,
                                                       subpixel=sub)
            T._check(batch[i], single[0].cpu().numpy(), f"{P.NAMES[packing]} frame {i} batch vs single")
            T._check(batch[i], X.render(F[i], D[i], *gains, packing, sub, sbs[i], fill, *m), f"{P.NAMES[packing]} frame {i} vs reference")
        T._check(native.render_stereo_source_batch(frames, d, *gains, packing, src, fill, *m, subpixel=sub).cpu().numpy(), batch,
                 f"{P.NAMES[packing]} strided frames")


def test_bad_arguments_return_their_code_without_launching(native):
    L = native.lib()
    H, W, Ws, Hs = 4, 16, 6, 2
    f = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
    sb = torch.zeros((2, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((2, 2 * H, 2 * W, 3), 99, dtype=torch.uint8, device="cuda")    # room for every packing
    fp, dp, sp, op = (C.c_void_p(t.data_ptr()) for t in (f, d, sb, out))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fr=fp, fs=H * W * 3, de=dp, dst=H * W, n=2, w=W, h=H, gl=0, gr=0, conv=0, sub=0, packing=P.FULL_TB, src=sp,
             ss=Hs * Ws * 3, ws=Ws, hs=Hs, pitch=Ws * 3, fill=2, ax=65536, bx=0, ay=65536, by=0, o=op):
        return L.v3d_render_stereo_source_batch(fr, fs, de, dst, n, w, h, gl, gr, conv, sub, packing, src, ss, ws, hs, pitch, fill,
                                                ax, bx, ay, by, o, s)

    packed = [dict(fr=None), dict(de=None), dict(o=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(h=-3),
              dict(fs=H * W * 3 - 1), dict(dst=H * W - 1), dict(packing=7), dict(packing=-1), dict(sub=2), dict(sub=-1),
              dict(packing=P.HALF_SBS, w=15, fs=H * 15 * 3, dst=H * 15), dict(packing=P.HALF_TB, h=3, fs=3 * W * 3, dst=3 * W),
              dict(gl=1 << 24), dict(gr=-(1 << 24)), dict(gl=-(1 << 24)), dict(conv=-1), dict(conv=65536)]
    own = [dict(src=None), dict(src=None, fill=1), dict(ws=5), dict(ws=0), dict(ws=1), dict(ws=-2), dict(hs=0), dict(hs=-1),
           dict(pitch=Ws * 3 - 1), dict(ss=Hs * Ws * 3 - 1), dict(fill=4), dict(fill=-1), dict(ax=4095), dict(ax=(1 << 20) + 1),
           dict(ay=4095), dict(ay=(1 << 20) + 1), dict(ax=-65536), dict(bx=(1 << 40) + 1), dict(bx=-(1 << 40) - 1),
           dict(by=(1 << 40) + 1), dict(by=-(1 << 40) - 1)]
    for sub in (0, 1):
        for fill in (0, 2):
            for kw in packed + own:
                kw = dict(dict(sub=sub, fill=fill), **kw)
                if kw["fill"] == 0 and kw.get("src", sp) is None and len(kw) == 3:
                    continue                                   # a null source is legal when no eye is filled
                assert call(**kw) == -1, kw
                assert b"v3d_render_stereo_source_batch" in L.v3d_last_error()
        assert call(sub=sub, w=8194, fs=H * 8194 * 3, dst=H * 8194) == -3              # V3D_ERR_UNSUPPORTED
        assert call(sub=sub, ws=2 * 8193, pitch=6 * 8193, ss=Hs * 6 * 8193) == -3
        for kw in (dict(fr=None), dict(n=0), dict(packing=7), dict(gl=1 << 24), dict(fill=4), dict(ax=4095)):
            assert call(sub=sub, ws=2 * 8193, pitch=6 * 8193, ss=Hs * 6 * 8193, **kw) == -1, kw     # a bad argument comes first
            assert call(sub=sub, w=8194, fs=H * 8194 * 3, dst=H * 8194, **kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((out == 99).all())                                                # nothing was enqueued
    for fill in (0, 3):                                                           # the extremes are legal, and exactly the frame is written
        out.fill_(99)
        assert call(gl=(1 << 24) - 1, gr=-((1 << 24) - 1), conv=65535, fill=fill, ax=4096, bx=1 << 40, ay=1 << 20, by=-(1 << 40)) == 0
        assert call(n=1, ss=0, fs=0, dst=0, fill=fill) == 0                       # one frame: the strides are not looked at
        torch.cuda.synchronize()
        flat = out.flatten()
        assert bool((flat[2 * 2 * H * W * 3:] == 99).all()) and not bool((flat[:2 * 2 * H * W * 3] == 99).any()), fill
    for fill in (4, -1, True, 2.0):
        with pytest.raises(ValueError):
            native.render_stereo_source_batch(f, d, 0, 0, 0, P.FULL_TB, sb, fill, 65536, 0, 65536, 0)
    with pytest.raises(native.NativeError):
        native.render_stereo_source_batch(f, d, 0, 0, 0, P.FULL_TB, None, 2, 65536, 0, 65536, 0)
    with pytest.raises(native.NativeError):
        native.render_stereo_source_batch(f, d, 0, 0, 0, P.FULL_TB, sb[:1], 2, 65536, 0, 65536, 0)
