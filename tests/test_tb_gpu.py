"""k_split_tb on the MI355X: v3d_tb_to_gray, v3d_split_tb and v3d_tb_to_gray_batch bit for bit against tests/tb_ref.py, through the
binding (dense frames) and through the raw entries (padded pitch and frame stride), and every refusal of the header.
Shapes W x H: 322 x 46 (rows of no multiple of 4 bytes, a partial last pixel group), 1030 x 18 and 2050 x 6 (two and three workgroups
across, the last one a partial group; eyes of 9 and 3 rows), 64 x 8, 5 x 2 and 7 x 4 (less than two pixel groups; eyes of 1 and 2 rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tb_ref

pytestmark = pytest.mark.gpu
SHAPES = [(322, 46), (1030, 18), (2050, 6), (64, 8), (5, 2), (7, 4)]
POISON = 0xA5


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _pitched(frames, pitch, stride):
    """[n,H,W,3] -> a device buffer with rows `pitch` and frames `stride` bytes apart, the padding poisoned"""
    n, H, W, _ = frames.shape
    buf = np.full(n * stride, POISON, np.uint8)
    for f in range(n):
        rows = buf[f * stride:f * stride + H * pitch].reshape(H, pitch)
        rows[:, :W * 3] = frames[f].reshape(H, W * 3)
    return torch.from_numpy(buf).cuda()


def _outs(shape):
    return (torch.full(shape, POISON, dtype=torch.uint8, device="cuda"), torch.full(shape, POISON, dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("unsqueeze", [True, False])
@pytest.mark.parametrize("W,H", SHAPES)
def test_the_three_entries_are_bit_exact(native, W, H, unsqueeze):
    tb = tb_ref.content(1, H, W, 31 * W + H)
    want_gray, want_bgr = tb_ref.to_gray(tb[0], unsqueeze), tb_ref.split(tb[0], unsqueeze)
    oh = H if unsqueeze else H // 2
    dev = native.to_device(tb[0])
    for got, want in zip(native.tb_to_gray(dev, unsqueeze), want_gray):                   # the binding: dense
        assert tuple(got.shape) == (oh, W) and np.array_equal(got.cpu().numpy(), want)
    for got, want in zip(native.split_tb(dev, unsqueeze), want_bgr):
        assert tuple(got.shape) == (oh, W, 3) and np.array_equal(got.cpu().numpy(), want)
    for got, want in zip(native.tb_to_gray_batch(dev[None], unsqueeze), want_gray):
        assert np.array_equal(got[0].cpu().numpy(), want)
    lib = native.lib()
    for pad in (4, 5, 16 - 3 * W % 16):                                                   # the raw entries: padded pitch
        pitch = 3 * W + pad
        src = _pitched(tb, pitch, H * pitch)
        L, R = _outs((oh, W))
        assert lib.v3d_tb_to_gray(_ptr(src), W, H, pitch, int(unsqueeze), _ptr(L), _ptr(R), _stream()) == 0
        assert np.array_equal(L.cpu().numpy(), want_gray[0]) and np.array_equal(R.cpu().numpy(), want_gray[1]), pad
        L, R = _outs((oh, W, 3))
        assert lib.v3d_split_tb(_ptr(src), W, H, pitch, int(unsqueeze), _ptr(L), _ptr(R), _stream()) == 0
        assert np.array_equal(L.cpu().numpy(), want_bgr[0]) and np.array_equal(R.cpu().numpy(), want_bgr[1]), pad


@pytest.mark.parametrize("unsqueeze", [True, False])
def test_batch_with_a_stride_pad(native, unsqueeze):
    n, W, H = 3, 322, 18
    tb = tb_ref.content(n, H, W, 9)
    want = tb_ref.to_gray_batch(tb, unsqueeze)
    oh = H if unsqueeze else H // 2
    lib = native.lib()
    for pad, spad in ((0, 7), (2, 40), (5, 0)):
        pitch = 3 * W + pad
        stride = H * pitch + spad
        L, R = _outs((n, oh, W))
        rc = lib.v3d_tb_to_gray_batch(_ptr(_pitched(tb, pitch, stride)), n, W, H, pitch, stride, int(unsqueeze), _ptr(L), _ptr(R), _stream())
        assert rc == 0 and np.array_equal(L.cpu().numpy(), want[0]) and np.array_equal(R.cpu().numpy(), want[1]), (pad, spad)
    got = native.tb_to_gray_batch(native.to_device(tb), unsqueeze)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])


def test_refusals_enqueue_nothing(native):
    """every V3D_ERR_ARG of the header; the poisoned outputs are untouched afterwards"""
    W, H, n = 16, 8, 2
    pitch, stride = 3 * W, H * 3 * W
    src = _pitched(tb_ref.content(n, H, W, 1), pitch, stride)
    L, R = _outs((n, H, W, 3))
    lib, st, null = native.lib(), _stream(), C.c_void_p(None)
    s, l, r = _ptr(src), _ptr(L), _ptr(R)
    single = lambda fn: [fn(null, W, H, pitch, 1, l, r, st), fn(s, W, H, pitch, 1, null, r, st), fn(s, W, H, pitch, 1, l, null, st),
                         fn(s, W, H - 1, pitch, 1, l, r, st), fn(s, W, 0, pitch, 1, l, r, st), fn(s, W, -2, pitch, 1, l, r, st),
                         fn(s, 0, H, pitch, 1, l, r, st), fn(s, W, H, 3 * W - 1, 1, l, r, st)]
    batch = [lib.v3d_tb_to_gray_batch(null, n, W, H, pitch, stride, 1, l, r, st), lib.v3d_tb_to_gray_batch(s, n, W, H, pitch, stride, 1, null, r, st),
             lib.v3d_tb_to_gray_batch(s, n, W, H, pitch, stride, 1, l, null, st), lib.v3d_tb_to_gray_batch(s, 0, W, H, pitch, stride, 1, l, r, st),
             lib.v3d_tb_to_gray_batch(s, n, W, H + 1, pitch, stride, 1, l, r, st), lib.v3d_tb_to_gray_batch(s, n, W, 0, pitch, stride, 1, l, r, st),
             lib.v3d_tb_to_gray_batch(s, n, 0, H, pitch, stride, 1, l, r, st), lib.v3d_tb_to_gray_batch(s, n, W, H, 3 * W - 1, stride, 1, l, r, st),
             lib.v3d_tb_to_gray_batch(s, n, W, H, pitch, stride - 1, 1, l, r, st)]
    assert b"stride" in lib.v3d_last_error()                                              # the batch's last refusal
    assert single(lib.v3d_tb_to_gray) + single(lib.v3d_split_tb) + batch == [-1] * (8 + 8 + 9)
    torch.cuda.synchronize()
    assert (L.cpu().numpy() == POISON).all() and (R.cpu().numpy() == POISON).all()
    assert lib.v3d_tb_to_gray_batch(s, 1, W, H, pitch, 0, 1, l, r, st) == 0               # n == 1 ignores the stride
    with pytest.raises(ValueError, match="top-bottom frame height must be even"):
        native.tb_to_gray(torch.zeros((7, 8, 3), dtype=torch.uint8, device="cuda"))
