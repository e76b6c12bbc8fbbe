"""v3d_quality_reproj_batch and v3d_quality_flicker_batch against the NumPy restatement (tests/quality_ref.py), bit for bit: at the
sizes where the kernels take another path (one pixel, one partial group, exactly one / one more than one group, odd widths on
the byte loads, widths of 8 k and 16 k on the vector loads, more than one row band, the widest plane), over the disparity and depth
patterns of the contract, at the two saturation extremes, inside a strided batch, and at every refusal the header states."""
import ctypes as C

import numpy as np
import pytest

import quality_ref as QR

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (7, 3, 2), (64, 5, 1), (65, 2, 3), (253, 77, 3), (320, 180, 3), (1037, 9, 2), (4112, 4, 1), (8192, 2, 1)]
IDS = [f"{w}x{h}x{n}" for w, h, n in SIZES]


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and got.shape == want.shape, what
    assert np.array_equal(got, want), f"{what}:\n got {got.tolist()}\nwant {want.tolist()}"


def _grays(n, H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, H, W), dtype=np.uint8), rng.integers(0, 256, (n, H, W), dtype=np.uint8)


def _disparities(n, H, W, seed):
    """pattern name -> int16 [n,H,W]"""
    rng = np.random.default_rng(seed)
    near = rng.integers(-40, 16 * W + 40, (n, H, W))
    rand = np.where(rng.random((n, H, W)) < 0.5, rng.integers(-32768, 32768, (n, H, W)), np.clip(near, -32768, 32767)).astype(np.int16)
    flat = rand.reshape(-1)
    for k, v in enumerate((0, -16, 32767, -32768, 1)):
        if k < flat.size:
            flat[(k * 7919) % flat.size] = v
    x, y = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    return {
        "random": rand,
        "invalid": np.where(rng.random((n, H, W)) < 0.5, 0, -16).astype(np.int16),
        "d16": np.full((n, H, W), 16, np.int16),
        "phases": np.broadcast_to(32 + ((x + y) & 15), (n, H, W)).astype(np.int16),
    }


@pytest.mark.parametrize("W,H,n", SIZES, ids=IDS)
def test_reproj_bit_exact(native, W, H, n):
    L, R = _grays(n, H, W, 3 * W + H)
    lg, rg = native.to_device(L), native.to_device(R)
    for name, d in _disparities(n, H, W, W + 5 * H).items():
        for thr in ((16,) if name != "random" else (0, 16, 255)):
            got = native.quality_reproj_batch(lg, rg, native.to_device(d), thr)
            want = QR.reproj(L, R, d, thr)
            _same(got, want, f"reproj {W}x{H}x{n} {name} thr {thr}")
            if name == "invalid":
                assert not want.any()
            if W == 1:
                assert not want[:, 1:].any()                     # W = 1: every valid pixel is out of view


def _depths(T, H, W, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 1024, (1, H, W))
    d = (np.clip(base + rng.integers(-40, 41, (T, H, W)), -30, 32767) / 16).astype(np.float32)
    d += (rng.random((T, H, W)) < 0.3) * np.float32(1 / 64)       # off the 1/16 grid: rint at work
    d[rng.random((T, H, W)) < 0.1] = np.nan
    d[rng.random((T, H, W)) < 0.1] = -3.5
    d[rng.random((T, H, W)) < 0.05] = 0.0
    d.reshape(-1)[0] = 0.03125                                    # 16 D = 0.5: rounds to 0 (half to even), invalid
    g = np.clip(rng.integers(0, 256, (1, H, W)) + rng.integers(-5, 6, (T, H, W)), 0, 255).astype(np.uint8)
    g[T // 2:, : max(H // 2, 1)] = 255 - g[T // 2:, : max(H // 2, 1)]          # a large luma step over half the plane
    return d, g


@pytest.mark.parametrize("W,H,k", [(w, h, k) for k, (w, h, _) in enumerate(SIZES)], ids=IDS)
def test_flicker_bit_exact(native, W, H, k):
    T = 2 + k % 4                                                 # T = 2 .. 5 over the sizes
    depth, gray = _depths(T, H, W, 11 * W + H)
    dd, gd = native.to_device(depth), native.to_device(gray)
    for still, jump in ((4, 16), (0, 0), (255, 32767)):
        _same(native.quality_flicker_batch(dd, gd, still, jump), QR.flicker(depth, gray, still, jump), f"flicker {W}x{H}x{T} still {still} jump {jump}")
    same_d, same_g = np.repeat(depth[:1], T, axis=0), np.repeat(gray[:1], T, axis=0)
    got = native.quality_flicker_batch(native.to_device(same_d), native.to_device(same_g), 0, 0).cpu().numpy()
    nv = int((QR.d16_of(depth[0]) >= 1).sum())
    assert got.tolist() == [[0, nv, 0, 0]] * (T - 1), "identical frames: flicker 0 and n_still = the valid count"


def test_reproj_saturation_1080p(native):
    """L = 255, R = 0, d = 16 everywhere at 1920 x 1080 x 2: e = 4080 on every compared pixel, ssd = 3.45e13 per frame -- far
    beyond a 32-bit partial anywhere between the lane and the record"""
    import torch
    n, H, W = 2, 1080, 1920
    lg = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")
    rg = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")
    d = torch.full((n, H, W), 16, dtype=torch.int16, device="cuda")
    c = H * (W - 1)
    want = [H * W, c, 4080 * c, 4080 ** 2 * c, c, 4080 * c, 4080 ** 2 * c, c]
    assert want[3] == 16646400 * 2072520 > 2 ** 44           # 3.45e13
    assert native.quality_reproj_batch(lg, rg, d, 16).cpu().numpy().tolist() == [want] * n
    assert QR.reproj_frame(lg[0, :3].cpu().numpy(), rg[0, :3].cpu().numpy(), d[0, :3].cpu().numpy(), 16).tolist() == [v * 3 // H for v in want]


def test_flicker_saturation_1080p(native):
    """a luma step of 255 under still = 255 and d16 jumping 1 <-> 32767 on every pixel of a 1920 x 1080 pair: flicker = 6.8e10"""
    import torch
    H, W = 1080, 1920
    depth = torch.empty((2, H, W), dtype=torch.float32, device="cuda")
    depth[0], depth[1] = 1 / 16, 32767 / 16
    depth[1, ::2], depth[0, ::2] = 1 / 16, 32767 / 16             # both directions of the jump
    gray = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda")
    gray[1] = 255
    px = H * W
    assert 32766 * px == 32766 * 2073600 > 2 ** 35              # 6.8e10
    assert native.quality_flicker_batch(depth, gray, 255, 32765).cpu().numpy().tolist() == [[255 * px, px, 32766 * px, px]]
    assert native.quality_flicker_batch(depth, gray, 255, 32766).cpu().numpy().tolist() == [[255 * px, px, 32766 * px, 0]]
    assert native.quality_flicker_batch(depth, gray, 254, 0).cpu().numpy().tolist() == [[255 * px, 0, 0, 0]]
    small = QR.flicker(depth[:, :2].cpu().numpy(), gray[:, :2].cpu().numpy(), 255, 32765)
    assert small.tolist() == [[255 * 2 * W, 2 * W, 32766 * 2 * W, 2 * W]]


@pytest.mark.parametrize("W,H,pad", [(253, 77, 11), (320, 180, 48), (320, 180, 7)])
def test_record_alone_equals_record_in_a_strided_batch(native, W, H, pad):
    """a frame's record at n = 1 and as frame 1 of 3 inside allocations with `pad` elements between the frames (48: the vector
    loads stay in play; 7 and 11: the byte loads); the padding holds values that would change every sum"""
    import torch
    n = 3
    L, R = _grays(n, H, W, 77)
    d = _disparities(n, H, W, 78)["random"]

    def strided(a, fill):
        t = torch.full((n, H * W + pad), fill, dtype=torch.from_numpy(a[:1]).dtype, device="cuda")
        v = t[:, :H * W].view(n, H, W)
        v.copy_(torch.from_numpy(a))
        assert v.stride(0) == H * W + pad
        return v
    lg, rg, dd = strided(L, 255), strided(R, 0), strided(d, 16)
    want = QR.reproj(L, R, d, 16)
    _same(native.quality_reproj_batch(lg, rg, dd, 16), want, "strided batch")
    for f in range(n):
        _same(native.quality_reproj_batch(lg[f:f + 1], rg[f:f + 1], dd[f:f + 1], 16), want[f:f + 1], f"frame {f} alone")
    depth, gray = _depths(n, H, W, 79)
    fd, fg = strided(depth, 7.0), strided(gray, 255)
    want = QR.flicker(depth, gray, 4, 16)
    _same(native.quality_flicker_batch(fd, fg, 4, 16), want, "strided clip")
    _same(native.quality_flicker_batch(fd[1:], fg[1:], 4, 16), want[1:], "the last pair alone")


def test_refusals(native):
    """every V3D_ERR_ARG / V3D_ERR_UNSUPPORTED case of the header, before anything is enqueued; the size functions give 0"""
    import torch
    lib = native.lib()
    P, st = C.c_void_p, native._stream()
    W, H, n = 64, 8, 2
    g = torch.zeros(4 * W * H + 64, dtype=torch.uint8, device="cuda")
    d = torch.zeros(4 * W * H, dtype=torch.int16, device="cuda")
    f = torch.zeros(4 * W * H, dtype=torch.float32, device="cuda")
    out = torch.full((64,), 7, dtype=torch.int64, device="cuda")
    ws = torch.full((1 << 16,), 9, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and out.data_ptr() % 8 == 0

    def reproj(l=g.data_ptr(), r=g.data_ptr(), n=n, W=W, H=H, pitch=W, fs=W * H, dp=d.data_ptr(), ds=W * H, thr=16, o=out.data_ptr(), w=ws.data_ptr()):
        nul = lambda v: None if v is None else P(v)
        return lib.v3d_quality_reproj_batch(nul(l), nul(r), n, W, H, pitch, fs, nul(dp), ds, thr, nul(o), nul(w), st)

    def flick(dp=f.data_ptr(), ds=W * H, gp=g.data_ptr(), gs=W * H, T=n, W=W, H=H, still=4, jump=16, o=out.data_ptr(), w=ws.data_ptr()):
        nul = lambda v: None if v is None else P(v)
        return lib.v3d_quality_flicker_batch(nul(dp), ds, nul(gp), gs, T, W, H, still, jump, nul(o), nul(w), st)

    ARG, UNS = -1, -3
    for kw in (dict(l=None), dict(r=None), dict(dp=None), dict(o=None), dict(w=None), dict(n=0), dict(n=65536), dict(W=0), dict(H=0),
               dict(pitch=W - 1), dict(fs=W * H - 1), dict(ds=W * H - 1), dict(thr=-1), dict(thr=256),
               dict(w=ws.data_ptr() + 8), dict(o=out.data_ptr() + 4)):
        assert reproj(**kw) == ARG, kw
        assert lib.v3d_last_error()
    for kw in (dict(W=8193, pitch=8193), dict(H=65536)):
        assert reproj(**kw) == UNS, kw
    for kw in (dict(dp=None), dict(gp=None), dict(o=None), dict(w=None), dict(T=1), dict(T=0), dict(T=65536), dict(W=0), dict(H=0),
               dict(ds=W * H - 1), dict(gs=W * H - 1), dict(still=-1), dict(still=256), dict(jump=-1), dict(jump=32768),
               dict(w=ws.data_ptr() + 8), dict(o=out.data_ptr() + 4)):
        assert flick(**kw) == ARG, kw
    for kw in (dict(W=8193), dict(H=65536)):
        assert flick(**kw) == UNS, kw
    assert reproj(n=1, fs=0, ds=0) == 0                           # a single frame ignores the strides
    assert reproj() == 0 and flick() == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:8] == [0, 0, 0, 0, 0, 0, 0, 0]).all() and (o[16:] == 7).all()

    rb, fb = lib.v3d_quality_reproj_ws_bytes, lib.v3d_quality_flicker_ws_bytes
    assert rb(1, 1, 1) == 64 and fb(2, 1, 1) == 32 and rb(34, 1920, 1080) % 64 == 0 and 0 < rb(34, 1920, 1080) <= 1 << 20
    for a in ((0, W, H), (65536, W, H), (1, 0, H), (1, W, 0), (1, 8193, H), (1, W, 65536)):
        assert rb(*a) == 0, a
    for a in ((1, W, H), (65536, W, H), (2, 0, H), (2, W, 0), (2, 8193, H), (2, W, 65536)):
        assert fb(*a) == 0, a
    with pytest.raises(ValueError):
        native.quality_reproj_batch(g[:W * H].view(1, H, W), g[:W * H].view(1, H, W), d[:W * H].view(1, H, W), 256)
    with pytest.raises(native.NativeError):
        native.quality_flicker_batch(f[:W * H].view(1, H, W), g[:W * H].view(1, H, W), 4, 16)


def test_temporal_filter_reduces_flicker_at_equal_populations(native):
    """the use the measure is for: the device disparity of synthetic.temporal_clip(320, 120, 9) through v3d_temporal_filter_batch
    (R = 2, tau = 12, fill = 0), flicker at still = 2 over the 8 pairs before and after.  fill = 0 keeps the populations equal
    (n_still does not change), so the sums compare; on the CPU oracle they are 95307 = 95307 and 132613 < 209170.  (With fill = 1
    the filled pixels join the population and the inequality reverses: 293394.)"""
    import torch
    from video_3d_pipeline import synthetic as syn
    L, R, _ = syn.temporal_clip(320, 120, 9)
    lg, rg = native.to_device(L), native.to_device(R)
    m = native.StereoSGBM(320, 120, 9)
    depth = native.disp_to_depth(m.compute(lg, rg))
    assert m.sync_errors() == 0
    m.close()
    cut = torch.zeros(9, dtype=torch.uint8, device="cuda")
    filt = native.temporal_filter_batch(depth, lg, 2, 12, cut, fill=False)
    raw = native.quality_flicker_batch(depth, lg, 2, 16).cpu().numpy().sum(axis=0)
    out = native.quality_flicker_batch(filt, lg, 2, 16).cpu().numpy().sum(axis=0)
    print(f"flicker raw {raw.tolist()} filtered {out.tolist()}")
    assert raw[1] == out[1] > 0
    assert out[2] < raw[2]
