"""v3d_render_stereo_batch (DIBR: 4K frame + 4K depth -> side-by-side 3D) on the MI355X, bit for bit against the NumPy
restatement of the contract (tests/stereo_ref.py), and its argument checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import stereo_ref as R

pytestmark = pytest.mark.gpu

GMAX = (1 << 24) - 1


def _depth(kind, H, W, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":                                             # dense collisions and cracks
        return rng.integers(0, 65536, (H, W)).astype(np.uint16)
    x = np.arange(W)[None, :]                                       # piecewise planar: ramps with steps between them
    cuts = np.sort(rng.integers(0, max(W, 1), 3))
    seg = (x >= cuts[0]).astype(int) + (x >= cuts[1]) + (x >= cuts[2])
    base = rng.integers(0, 65536, 4)[seg]
    slope = rng.integers(-400, 400, 4)[seg]
    d = base + slope * x + rng.integers(-3000, 3000, (H, 1))
    return np.clip(d, 0, 65535).astype(np.uint16)


def _gpu(native, F, D, gl, gr, conv, layout):
    f = torch.from_numpy(np.ascontiguousarray(F)[None]).cuda()
    d = torch.from_numpy(np.ascontiguousarray(D).view(np.int16)[None]).cuda()
    return native.render_stereo_batch(f, d, gl, gr, conv, layout)[0].cpu().numpy()


def _params(W):
    """(gain_left, gain_right, conv): zero, the defaults, eye_split 0 and 1, +-255 px, shifts >= W, conv at both ends"""
    return [(0, 0, 32768), R.stereo_gains(), R.stereo_gains(48, 0.5, 0.0), R.stereo_gains(48, 0.5, 1.0),
            R.stereo_gains(510, 0.5, 0.5), R.stereo_gains(510, 0.0, 0.5), R.stereo_gains(510, 1.0, 0.5),
            (GMAX, -GMAX, 0), (-GMAX, GMAX, 65535), (W * 256 + 77, -(W * 256 + 77), 0)]


def _check(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} "
                             f"want {want[tuple(bad[0])]}")


@pytest.mark.timeout(600)
@pytest.mark.parametrize("W, H", [(1, 1), (7, 3), (6, 3), (255, 5), (1000, 4), (8192, 2)])
def test_small_sizes_bit_exact(native, W, H):
    F = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    layouts = [R.FULL_SBS] + ([R.HALF_SBS] if W % 2 == 0 else [])
    for kind in ("noise", "planar"):
        D = _depth(kind, H, W, W + H)
        for (gl, gr, conv) in _params(W):
            for layout in layouts:
                _check(_gpu(native, F, D, gl, gr, conv, layout), R.render(F, D, gl, gr, conv, layout),
                       f"{W}x{H} {kind} g=({gl},{gr}) conv={conv} layout={layout}")


# both sides of every change of pixels per thread (8 up to 2048, 16 up to 4096, 32 above), and widths that end inside a thread's
# run; a band of 4 rows plus a band of 1
@pytest.mark.parametrize("W", [2047, 2048, 2049, 4090, 4096, 4097, 8190])
def test_route_change_and_ragged_widths_bit_exact(native, W):
    H = 5
    F = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    layouts = [R.FULL_SBS] + ([R.HALF_SBS] if W % 2 == 0 else [])
    for i, (gl, gr, conv) in enumerate(_params(W)):
        kind = ("noise", "planar")[i % 2]
        D = _depth(kind, H, W, W + H + i)
        for layout in layouts:
            _check(_gpu(native, F, D, gl, gr, conv, layout), R.render(F, D, gl, gr, conv, layout),
                   f"{W}x{H} {kind} g=({gl},{gr}) conv={conv} layout={layout}")


def test_nearest_key_beyond_a_wave_or_absent(native):
    """holes and row ends 600 targets wide at 8 targets per thread: the scan's answer comes from another wave or is 'none'"""
    F, D, (gl, gr, conv) = R.far_key_scene()
    for layout in (R.FULL_SBS, R.HALF_SBS):
        _check(_gpu(native, F, D, gl, gr, conv, layout), R.render(F, D, gl, gr, conv, layout), f"far keys, layout {layout}")


def _frame_4k():
    from video_3d_pipeline import synthetic as syn
    g = syn.guide_frame(1920, 1080, 0).astype(np.int32)                          # 3840 x 2160 luma of the left view
    F = np.stack([g, 255 - g, (g * 7 + 40) % 256], axis=-1).astype(np.uint8)
    d = syn.gt_disparity(3840, 2160)                                            # piecewise planar, as the depth maps are
    D = np.rint((d - d.min()) / (d.max() - d.min()) * 65535).astype(np.uint16)
    return F, D


@pytest.mark.timeout(600)
def test_4k_frame_bit_exact(native):
    F, D = _frame_4k()
    for (gl, gr, conv) in (R.stereo_gains(), R.stereo_gains(200, 0.3, 0.0)):
        for layout in (R.FULL_SBS, R.HALF_SBS):
            _check(_gpu(native, F, D, gl, gr, conv, layout), R.render(F, D, gl, gr, conv, layout), f"4K layout {layout} g={gl},{gr}")
    noisy = (D.astype(np.int64) + np.random.default_rng(5).integers(-20000, 20000, D.shape)).clip(0, 65535).astype(np.uint16)
    _check(_gpu(native, F, noisy, *R.stereo_gains(), R.FULL_SBS), R.render(F, noisy, *R.stereo_gains()), "4K noisy depth")


@pytest.mark.timeout(300)
def test_batch_equals_single_calls_and_strided_frames(native):
    H, W, n = 37, 1000, 5
    rng = np.random.default_rng(8)
    F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([_depth("noise" if i % 2 else "planar", H, W, 100 + i) for i in range(n)])
    gl, gr, conv = R.stereo_gains(80, 0.4, 0.3)
    f = torch.from_numpy(F).cuda()
    d = torch.from_numpy(D.view(np.int16)).cuda()
    for layout in (R.FULL_SBS, R.HALF_SBS):
        batch = native.render_stereo_batch(f, d, gl, gr, conv, layout).cpu().numpy()
        for i in range(n):
            single = native.render_stereo_batch(f[i:i + 1], d[i:i + 1].contiguous(), gl, gr, conv, layout)[0].cpu().numpy()
            _check(batch[i], single, f"frame {i} batch vs single")
            _check(batch[i], R.render(F[i], D[i], gl, gr, conv, layout), f"frame {i} vs reference")
        # frames inside a larger capacity buffer, at an odd byte offset (rows not 16-byte aligned) and a padded stride
        per = H * W * 3
        cap = torch.full((n + 2, per + 45), 7, dtype=torch.uint8, device="cuda")
        frames = cap[:n, 5:5 + per].unflatten(1, (H, W, 3))
        frames.copy_(f)
        assert frames.stride(0) == per + 45
        _check(native.render_stereo_batch(frames, d, gl, gr, conv, layout).cpu().numpy(), batch, "strided frames")


@pytest.mark.timeout(120)
def test_bad_arguments_return_their_code_without_launching(native):
    L = native.lib()
    H, W = 4, 16
    f = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
    out = torch.full((2, H, 2 * W, 3), 99, dtype=torch.uint8, device="cuda")
    fp, dp, op = C.c_void_p(f.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fr=fp, fs=H * W * 3, de=dp, dst=H * W, n=2, w=W, h=H, gl=0, gr=0, conv=0, layout=0, o=op):
        return L.v3d_render_stereo_batch(fr, fs, de, dst, n, w, h, gl, gr, conv, layout, o, s)

    bad = [dict(fr=None), dict(de=None), dict(o=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(h=-3),
           dict(fs=H * W * 3 - 1), dict(dst=H * W - 1), dict(layout=2), dict(layout=-1), dict(layout=1, w=15, fs=H * 15 * 3, dst=H * 15),
           dict(gl=1 << 24), dict(gr=-(1 << 24)), dict(gl=-(1 << 24)), dict(conv=-1), dict(conv=65536)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"v3d_render_stereo_batch" in L.v3d_last_error()
    assert call(w=8193, fs=H * 8193 * 3, dst=H * 8193) == -3                      # V3D_ERR_UNSUPPORTED
    assert call(gl=(1 << 24) - 1, gr=-((1 << 24) - 1), conv=65535) == 0           # the extremes are legal
    torch.cuda.synchronize()
    assert not out.any()                                                          # ... and only that call wrote
    out.fill_(99)
    for kw in bad:
        call(**kw)
    torch.cuda.synchronize()
    assert bool((out == 99).all())
    with pytest.raises(ValueError):
        native.render_stereo_batch(f, d, 0, 0, 0, layout=3)
    with pytest.raises(native.NativeError):
        native.render_stereo_batch(f, d[:1], 0, 0, 0)
