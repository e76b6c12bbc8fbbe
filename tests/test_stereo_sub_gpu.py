"""v3d_render_stereo_subpixel_batch (sub-pixel DIBR) on the MI355X, bit for bit against the NumPy restatement of the contract
(tests/stereo_sub_ref.py), and its argument checks.  The scenes and parameters are that module's (scene_depth, scene_params):
tests/test_stereo_sub_ref.py shows on the CPU that they reach every case class of the contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import stereo_sub_ref as S

pytestmark = pytest.mark.gpu

# the widths at which the kernel changes its pixels-per-thread (2048, 4096) or a thread's run ends, each with one of the band
# remainders (4 rows per workgroup)
SIZES = [(1, 1), (2, 4), (7, 5), (255, 9), (256, 1), (257, 4), (2047, 5), (2048, 9), (2049, 1), (3840, 4), (4097, 5), (8192, 9),
         (7, 9), (257, 5)]


def _gpu(native, F, D, gl, gr, conv, layout):
    f = torch.from_numpy(np.ascontiguousarray(F)[None]).cuda()
    d = torch.from_numpy(np.ascontiguousarray(D).view(np.int16)[None]).cuda()
    return native.render_stereo_batch(f, d, gl, gr, conv, layout, subpixel=True)[0].cpu().numpy()


def _check(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} "
                             f"want {want[tuple(bad[0])]}")


@pytest.mark.parametrize("W, H", SIZES)
def test_sizes_bit_exact(native, W, H):
    F = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    layouts = [S.FULL_SBS] + ([S.HALF_SBS] if W % 2 == 0 else [])
    for kind in S.SCENES:
        D = S.scene_depth(kind, H, W, W + H)
        for (gl, gr, conv) in S.scene_params(W):
            for layout in layouts:
                _check(_gpu(native, F, D, gl, gr, conv, layout), S.render(F, D, gl, gr, conv, layout),
                       f"{W}x{H} {kind} g=({gl},{gr}) conv={conv} layout={layout}")


def test_nearest_key_beyond_a_wave_or_absent(native):
    """holes and row ends 600 targets wide at 8 targets per thread: the scan's answer comes from another wave or is 'none'"""
    from stereo_ref import far_key_scene
    F, D, (gl, gr, conv) = far_key_scene()
    for layout in (S.FULL_SBS, S.HALF_SBS):
        _check(_gpu(native, F, D, gl, gr, conv, layout), S.render(F, D, gl, gr, conv, layout), f"far keys, layout {layout}")


def test_half_sbs_at_odd_run_edges(native):
    """even widths next to the boundaries (half SBS needs them): 254, 2046, 2050, 4094, 4098"""
    for W in (254, 2046, 2050, 4094, 4098):
        F = np.random.default_rng(W).integers(0, 256, (4, W, 3), dtype=np.uint8)
        for kind in ("planar", "steep"):
            D = S.scene_depth(kind, 4, W, W)
            gl, gr, conv = S.stereo_gains()
            _check(_gpu(native, F, D, gl, gr, conv, S.HALF_SBS), S.render(F, D, gl, gr, conv, S.HALF_SBS), f"half {W} {kind}")


def test_subpixel_differs_from_the_integer_entry_and_agrees_where_it_must(native):
    """the flag selects another kernel: a fractional constant shift renders differently, a whole-pixel one identically"""
    import stereo_ref as R
    H, W = 5, 300
    F = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    gl, gr, conv = 6144, -6144, 32768
    f = torch.from_numpy(F[None]).cuda()
    for d, same in ((conv + 8192, True), (conv + 5000, False)):                   # s16 = 48 (3 px) and 29 (1 13/16 px)
        D = np.full((H, W), d, np.uint16)
        dd = torch.from_numpy(D.view(np.int16)[None]).cuda()
        sub = native.render_stereo_batch(f, dd, gl, gr, conv, subpixel=True)[0].cpu().numpy()
        integer = native.render_stereo_batch(f, dd, gl, gr, conv)[0].cpu().numpy()
        _check(integer, R.render(F, D, gl, gr, conv), "integer entry")
        _check(sub, S.render(F, D, gl, gr, conv), "sub-pixel entry")
        assert np.array_equal(sub, integer) == same


def test_batch_equals_single_calls_and_strided_frames(native):
    H, W, n = 9, 1000, 5
    rng = np.random.default_rng(8)
    F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([S.scene_depth(S.SCENES[i % len(S.SCENES)], H, W, 100 + i) for i in range(n)])
    gl, gr, conv = S.stereo_gains(80, 0.4, 0.3)
    f = torch.from_numpy(F).cuda()
    d = torch.from_numpy(D.view(np.int16)).cuda()
    for layout in (S.FULL_SBS, S.HALF_SBS):
        batch = native.render_stereo_batch(f, d, gl, gr, conv, layout, subpixel=True).cpu().numpy()
        for i in range(n):
            single = native.render_stereo_batch(f[i:i + 1], d[i:i + 1].contiguous(), gl, gr, conv, layout, subpixel=True)[0].cpu().numpy()
            _check(batch[i], single, f"frame {i} batch vs single")
            _check(batch[i], S.render(F[i], D[i], gl, gr, conv, layout), f"frame {i} vs reference")
        # the same frames in another order: a frame's bytes do not depend on its place in the batch
        perm = [3, 0, 4, 2, 1]
        _check(native.render_stereo_batch(f[perm].contiguous(), d[perm].contiguous(), gl, gr, conv, layout, subpixel=True).cpu().numpy(),
               batch[perm], "permuted batch")
        # frames inside a larger capacity buffer, at an odd byte offset (rows not 16-byte aligned) and a padded stride
        per = H * W * 3
        cap = torch.full((n + 2, per + 45), 7, dtype=torch.uint8, device="cuda")
        frames = cap[:n, 5:5 + per].unflatten(1, (H, W, 3))
        frames.copy_(f)
        assert frames.stride(0) == per + 45
        _check(native.render_stereo_batch(frames, d, gl, gr, conv, layout, subpixel=True).cpu().numpy(), batch, "strided frames")


def test_bad_arguments_return_their_code_without_launching(native):
    L = native.lib()
    H, W = 4, 16
    f = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
    out = torch.full((2, H, 2 * W, 3), 99, dtype=torch.uint8, device="cuda")
    fp, dp, op = C.c_void_p(f.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fr=fp, fs=H * W * 3, de=dp, dst=H * W, n=2, w=W, h=H, gl=0, gr=0, conv=0, layout=0, o=op):
        return L.v3d_render_stereo_subpixel_batch(fr, fs, de, dst, n, w, h, gl, gr, conv, layout, o, s)

    bad = [dict(fr=None), dict(de=None), dict(o=None), dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=0), dict(h=-3),
           dict(fs=H * W * 3 - 1), dict(dst=H * W - 1), dict(layout=2), dict(layout=-1), dict(layout=1, w=15, fs=H * 15 * 3, dst=H * 15),
           dict(gl=1 << 24), dict(gr=-(1 << 24)), dict(gl=-(1 << 24)), dict(gr=1 << 24), dict(conv=-1), dict(conv=65536)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"v3d_render_stereo_subpixel_batch" in L.v3d_last_error()
    assert call(w=8193, fs=H * 8193 * 3, dst=H * 8193) == -3                      # V3D_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 99).all())                                                # no refused call wrote
    assert call(gl=(1 << 24) - 1, gr=-((1 << 24) - 1), conv=65535) == 0           # the extremes are legal
    torch.cuda.synchronize()
    assert not out.any()
    with pytest.raises(ValueError):
        native.render_stereo_batch(f, d, 0, 0, 0, layout=3, subpixel=True)
    with pytest.raises(native.NativeError):
        native.render_stereo_batch(f, d[:1], 0, 0, 0, subpixel=True)
