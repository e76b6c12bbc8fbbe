"""v3d_render_stereo_packed_batch (the DIBR step with the eyes packed top-bottom, row-interleaved or as an anaglyph) on the
MI355X, bit for bit against the NumPy restatement (tests/stereo_pack_ref.py), both renderers, and its argument checks.

Sizes: the smallest frames, a run that ends inside a thread, more than one thread run, and both sides of every change of pixels
per thread (8 up to 2048, 16 up to 4096, 32 above) at H = 6 (a band of 4 rows plus a ragged band that holds one row pair) and, for
the packings that allow an odd height, at H = 5 (a band of 1 whose only row is a left-eye row of the row-interleaved frame).
Depth kinds and gain sets are those of tests/test_stereo_gpu.py, cycled over the sizes a packing allows: every gain set meets
every packing at some size."""
import ctypes as C

import numpy as np
import pytest
import torch

import stereo_pack_ref as P
import stereo_ref as R
import test_stereo_gpu as T

pytestmark = pytest.mark.gpu

NEW = (P.FULL_TB, P.HALF_TB, P.ROWS, P.ANAGLYPH_COLOUR, P.ANAGLYPH_DUBOIS)
ROUTE_W = (2047, 2048, 2049, 4096, 4097, 8190, 8192)
SIZES = [(1, 1), (1, 2), (7, 3), (6, 4), (255, 5), (254, 6), (1000, 6)] + [(W, 6) for W in ROUTE_W] + [(W, 5) for W in ROUTE_W]
NGAINS = len(T._params(1))


def _plan():
    """{(W, H): [(packing, subpixel, gain index, depth kind)]}: a packing's j-th allowed size takes gain set j (j + 5 for the
    sub-pixel renderer), so its first ten sizes see them all"""
    plan = {s: [] for s in SIZES}
    for packing in NEW:
        allowed = [(W, H) for (W, H) in SIZES if not (packing == P.HALF_TB and H % 2)]
        assert len(allowed) >= NGAINS
        for j, s in enumerate(allowed):
            plan[s].append((packing, False, j % NGAINS, ("noise", "planar")[j % 2]))
            plan[s].append((packing, True, (j + 5) % NGAINS, ("planar", "noise")[j % 2]))
    return plan


PLAN = _plan()


def _gpu(native, F, D, gl, gr, conv, packing, subpixel):
    f = torch.from_numpy(np.ascontiguousarray(F)[None]).cuda()
    d = torch.from_numpy(np.ascontiguousarray(D).view(np.int16)[None]).cuda()
    return native.render_stereo_packed_batch(f, d, gl, gr, conv, packing, subpixel=subpixel)[0].cpu().numpy()


def test_every_gain_set_meets_every_packing():
    for packing in NEW:
        for sub in (False, True):
            seen = {g for cases in PLAN.values() for (p, s, g, _) in cases if p == packing and s == sub}
            assert seen == set(range(NGAINS))


@pytest.mark.parametrize("W,H", SIZES)
def test_packings_bit_exact(native, W, H):
    F = np.random.default_rng(W + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for packing, sub, gi, kind in PLAN[(W, H)]:
        gl, gr, conv = T._params(W)[gi]
        D = T._depth(kind, H, W, W + H + gi)
        got = _gpu(native, F, D, gl, gr, conv, packing, sub)
        assert got.shape == P.output_size(packing, W, H)[::-1] + (3,)
        T._check(got, P.render(F, D, gl, gr, conv, packing, sub),
                 f"{W}x{H} {P.NAMES[packing]} sub={sub} {kind} g=({gl},{gr}) conv={conv}")


@pytest.mark.parametrize("subpixel", [False, True])
def test_nearest_key_beyond_a_wave_or_absent(native, subpixel):
    F, D, (gl, gr, conv) = R.far_key_scene()
    EL, ER = P.eyes(F, D, gl, gr, conv, subpixel)
    for packing in P.PACKINGS:
        T._check(_gpu(native, F, D, gl, gr, conv, packing, subpixel), P.pack(EL, ER, packing), f"far keys, {P.NAMES[packing]}")


def _batch(n, H, W):
    rng = np.random.default_rng(8)
    F = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    D = np.stack([T._depth("noise" if i % 2 else "planar", H, W, 100 + i) for i in range(n)])
    return F, D, torch.from_numpy(F).cuda(), torch.from_numpy(D.view(np.int16)).cuda()


def test_codes_0_and_1_equal_the_older_entries(native):
    H, W, n = 6, 334, 2
    _, _, f, d = _batch(n, H, W)
    gl, gr, conv = R.stereo_gains(80, 0.4, 0.3)
    for sub in (False, True):
        for layout in (P.FULL_SBS, P.HALF_SBS):
            old = native.render_stereo_batch(f, d, gl, gr, conv, layout, subpixel=sub)
            new = native.render_stereo_packed_batch(f, d, gl, gr, conv, layout, subpixel=sub)
            assert old.shape == new.shape and torch.equal(old, new), (layout, sub)


def test_batch_equals_single_calls_and_strided_frames(native):
    H, W, n = 6, 333, 3
    F, D, f, d = _batch(n, H, W)
    gl, gr, conv = R.stereo_gains(80, 0.4, 0.3)
    per = H * W * 3
    cap = torch.full((n + 2, per + 45), 7, dtype=torch.uint8, device="cuda")       # frames at an odd byte offset, a padded stride
    frames = cap[:n, 5:5 + per].unflatten(1, (H, W, 3))
    frames.copy_(f)
    assert frames.stride(0) == per + 45
    for k, packing in enumerate(NEW):
        sub = bool(k % 2)
        batch = native.render_stereo_packed_batch(f, d, gl, gr, conv, packing, subpixel=sub).cpu().numpy()
        for i in range(n):
            single = native.render_stereo_packed_batch(f[i:i + 1], d[i:i + 1].contiguous(), gl, gr, conv, packing, subpixel=sub)
            T._check(batch[i], single[0].cpu().numpy(), f"{P.NAMES[packing]} frame {i} batch vs single")
            T._check(batch[i], P.render(F[i], D[i], gl, gr, conv, packing, sub), f"{P.NAMES[packing]} frame {i} vs reference")
        T._check(native.render_stereo_packed_batch(frames, d, gl, gr, conv, packing, subpixel=sub).cpu().numpy(), batch,
                 f"{P.NAMES[packing]} strided frames")


def test_bad_arguments_return_their_code_without_launching(native):
    L = native.lib()
    H, W = 4, 16
    f = torch.zeros((2, H, W, 3), dtype=torch.uint8, device="cuda")
    d = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
    out = torch.full((2, 2 * H, 2 * W, 3), 99, dtype=torch.uint8, device="cuda")    # room for every packing
    fp, dp, op = C.c_void_p(f.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fr=fp, fs=H * W * 3, de=dp, dst=H * W, n=2, w=W, h=H, gl=0, gr=0, conv=0, sub=0, packing=P.FULL_TB, o=op):
        return L.v3d_render_stereo_packed_batch(fr, fs, de, dst, n, w, h, gl, gr, conv, sub, packing, o, s)

    bad = [dict(fr=None), dict(de=None), dict(o=None), dict(n=0), dict(n=-1), dict(w=0), dict(h=0), dict(h=-3),
           dict(fs=H * W * 3 - 1), dict(dst=H * W - 1), dict(packing=7), dict(packing=-1), dict(sub=2), dict(sub=-1),
           dict(packing=P.HALF_SBS, w=15, fs=H * 15 * 3, dst=H * 15), dict(packing=P.HALF_TB, h=3, fs=3 * W * 3, dst=3 * W),
           dict(gl=1 << 24), dict(gr=-(1 << 24)), dict(gl=-(1 << 24)), dict(conv=-1), dict(conv=65536)]
    for sub in (0, 1):
        for kw in bad:
            kw = dict(dict(sub=sub), **kw)
            assert call(**kw) == -1, kw
            assert b"v3d_render_stereo_packed_batch" in L.v3d_last_error()
        for packing in P.PACKINGS:
            assert call(sub=sub, packing=packing, w=8194, fs=H * 8194 * 3, dst=H * 8194) == -3          # V3D_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 99).all())                                                # nothing was enqueued
    for packing in P.PACKINGS:                                                    # the extremes are legal, and exactly the frame is written
        out.fill_(99)
        assert call(gl=(1 << 24) - 1, gr=-((1 << 24) - 1), conv=65535, packing=packing) == 0
        torch.cuda.synchronize()
        oW, oH = P.output_size(packing, W, H)
        flat = out.flatten()
        assert not flat[:2 * oH * oW * 3].any() and bool((flat[2 * oH * oW * 3:] == 99).all()), packing
    for packing in (7, -1, True, 2.0):
        with pytest.raises(ValueError):
            native.render_stereo_packed_batch(f, d, 0, 0, 0, packing)
    with pytest.raises(ValueError):
        native.render_stereo_packed_batch(f[:, :3].contiguous(), d[:, :3].contiguous(), 0, 0, 0, P.HALF_TB)
    with pytest.raises(ValueError):
        native.render_stereo_packed_batch(f, d, 0, 0, 0, P.FULL_TB, subpixel=2)
    with pytest.raises(native.NativeError):
        native.render_stereo_packed_batch(f, d[:1], 0, 0, 0, P.FULL_TB)
    for packing in P.PACKINGS:
        assert native.stereo_output_size(packing, W, H) == P.output_size(packing, W, H)
