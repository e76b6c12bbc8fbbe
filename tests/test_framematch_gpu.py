"""v3d_frame_signature_batch and v3d_signature_scores against the NumPy restatement (tests/framematch_ref.py), bit for bit, at
the shapes where the kernel takes another path, their refusals, and framematch.refine on the device against the restatement's
whole refinement."""
import ctypes as C

import numpy as np
import pytest

import framematch_ref as FR
from conftest import mismatch_report

pytestmark = pytest.mark.gpu


def _frames(n, H, W, seed):
    """random frames, then one all-255 and one all-0 frame"""
    g = np.random.default_rng(seed).integers(0, 256, (n + 2, H, W), dtype=np.uint8)
    g[n], g[n + 1] = 255, 0
    return g


def _sig(native, gray_dev):
    return native.frame_signature_batch(gray_dev).cpu().numpy().view(np.uint16)


# 64x36: one pixel per cell; 65x37: cells of 1 and 2; 322x182: byte path, partial last group; 8190x36 / 8192x40: the widest
# cells, two column groups per lane row; 1920x36: vector path with n = 3
@pytest.mark.parametrize("W,H,n", [(64, 36, 1), (65, 37, 1), (322, 182, 1), (8190, 36, 1), (8192, 40, 1), (1920, 36, 1)])
def test_signature_bit_exact(native, W, H, n):
    g = _frames(n, H, W, W * 7 + H)
    got = _sig(native, native.to_device(g))
    assert got.shape == (n + 2, FR.G)
    rep = mismatch_report(got, FR.signature(g), f"signature {W}x{H}")
    assert not rep, rep
    assert (got[n] == 65280).all() and (got[n + 1] == 0).all()


def test_signature_product_shape(native):
    """3840 x 2160, n = 2: the 4K luma of the pipeline (60 x 60 pixel cells, 16-byte loads, four row phases)"""
    import torch
    g = torch.randint(0, 256, (2, 2160, 3840), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    got = _sig(native, g)
    rep = mismatch_report(got, FR.signature(g.cpu().numpy()), "signature 3840x2160")
    assert not rep, rep


def test_signature_padded_pitch_stride_and_odd_base(native):
    """253 x 77, n = 3 inside a larger allocation: pitch 260, stride 77 * 260 + 11, base pointer odd -> the byte path; the
    padding holds 255s that must not reach a sum"""
    import torch
    W, H, n, pitch = 253, 77, 3, 260
    stride = H * pitch + 11
    g = _frames(n - 2, H, W, 5)
    buf = np.full(1 + n * stride, 255, np.uint8)
    for f in range(n):
        for y in range(H):
            buf[1 + f * stride + y * pitch:1 + f * stride + y * pitch + W] = g[f, y]
    d = native.to_device(buf)
    out = torch.empty((n, FR.G), dtype=torch.int16, device="cuda")
    rc = native.lib().v3d_frame_signature_batch(C.c_void_p(d.data_ptr() + 1), n, W, H, pitch, stride, C.c_void_p(out.data_ptr()),
                                                native._stream())
    assert rc == 0, native.lib().v3d_last_error()
    rep = mismatch_report(out.cpu().numpy().view(np.uint16), FR.signature(g), "padded signature")
    assert not rep, rep


def test_signature_refusals(native):
    import torch
    L = native.lib()
    g = torch.zeros(4 * 8200 * 40, dtype=torch.uint8, device="cuda")
    out = torch.full((2, FR.G), 0x5A5A, dtype=torch.int16, device="cuda")
    P, st = C.c_void_p, native._stream()
    call = lambda n, W, H, pitch, stride, gp=g.data_ptr(), op=out.data_ptr(): L.v3d_frame_signature_batch(P(gp), n, W, H, pitch, stride, P(op), st)
    for W, H in ((63, 36), (64, 35), (8193, 36), (64, 8193)):
        assert call(1, W, H, W, W * H) == -3, (W, H)                                  # V3D_ERR_UNSUPPORTED
    assert call(1, 128, 72, 127, 128 * 72) == -1 and b"pitch" in L.v3d_last_error()
    assert call(2, 128, 72, 128, 128 * 72 - 1) == -1 and b"stride" in L.v3d_last_error()       # overlapping frames
    assert call(0, 128, 72, 128, 128 * 72) == -1 and call(65536, 128, 72, 128, 128 * 72) == -1
    assert call(1, 128, 72, 128, 0, gp=None) == -1 and call(1, 128, 72, 128, 0, op=None) == -1
    assert call(1, 128, 72, 128, 0) == 0                                             # n == 1 ignores the stride
    torch.cuda.synchronize()
    assert (out[1].cpu().numpy() == 0x5A5A).all()


def _signatures(n, seed):
    s = np.random.default_rng(seed).integers(0, 65281, (n, FR.G)).astype(np.uint16)
    s[0] = 65280                                                     # the all-65280 signature: zero variance
    if n > 1:
        s[1] = np.where(np.arange(FR.G) % 2 == 0, 0, 65280)          # alternating 0 / 65280: the largest terms
    if n > 2:
        s[2] = 12345                                                 # another zero-variance row
    return s


@pytest.mark.parametrize("na,nb", [(1, 1), (5, 9), (48, 56)])
def test_scores_bit_exact(native, na, nb):
    a, b = _signatures(na, na), _signatures(nb, 100 + nb)
    got = native.signature_scores(native.to_device(a.view(np.int16)), native.to_device(b.view(np.int16)))
    for name, g, w in zip(("num", "var_a", "var_b"), got, FR.scores(a, b)):
        g = g.cpu().numpy()
        assert g.dtype == np.int64 and np.array_equal(g, w), f"{name} {na}x{nb}: {int((g != w).sum())} differ"
    assert got[1][0].item() == 0


def test_scores_refusals(native):
    import torch
    L = native.lib()
    s = torch.zeros((2, FR.G), dtype=torch.int16, device="cuda")
    o = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    P, st = C.c_void_p, native._stream()
    for na, nb in ((0, 1), (1, 0), (4097, 1), (1, 4097)):
        assert L.v3d_signature_scores(P(s.data_ptr()), na, P(s.data_ptr()), nb, P(o.data_ptr()), P(o.data_ptr()), P(o.data_ptr()), st) == -1
    assert L.v3d_signature_scores(None, 1, P(s.data_ptr()), 1, P(o.data_ptr()), P(o.data_ptr()), P(o.data_ptr()), st) == -1
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == 7).all()


def test_refine_on_the_device_equals_the_restatement(native, tmp_path):
    """256 x 144 clips as .npy stacks: the SBS side carries the left view in both halves unsqueezed by the device, so the
    restatement gets the device's own left gray planes; every integer, the decision and M(d) (1e-12: a handful of float64
    operations on values of magnitude <= 1, possibly in another order) must agree"""
    from video_3d_pipeline import framematch as FM
    from video_3d_pipeline.pipeline import HipPipelineBackend
    left, guide = FR.match_clips(256, 144, 24, speed=6, delay=3)
    sbs = np.repeat(np.concatenate([left, left], axis=2)[..., None], 3, axis=3)            # [n,144,512,3], squeezed eyes = left
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "g.npy", np.repeat(guide[..., None], 3, axis=3))
    be = HipPipelineBackend("cuda")
    res = FM.refine(str(tmp_path / "sbs.npy"), str(tmp_path / "g.npy"), 0, search=4, window=12, probes=3, unsqueeze=False,
                    min_score=0.5, min_margin=0.01, backend=be)
    lg = native.sbs_to_gray_batch(native.to_device(sbs), False)[0].cpu().numpy()           # what the device matched
    gg = np.stack([native.bgr_to_gray(native.to_device(np.repeat(f[..., None], 3, axis=2))).cpu().numpy() for f in guide])
    want = FR.refine_ref(lg, gg, 0, search=4, window=12, probes=3, min_score=0.5, min_margin=0.01)
    print(f"device refine: {res['status']} shift {res['shift']} M(d*) {res['score']:.6f} margin {res['margin']:.6f}")
    assert len(res["ints"]) == len(want["ints"]) == 3
    for got3, want3 in zip(res["ints"], want["ints"]):
        for g, w in zip(got3, want3):
            assert np.array_equal(g, w)
    for key in ("status", "shift", "best_shift", "probe_shifts"):
        assert res[key] == want[key], key
    assert (res["status"], res["shift"], res["guide_start_frame"]) == ("refined", 3, 3)
    assert np.allclose(res["M"], want["M"], rtol=0, atol=1e-12, equal_nan=True)
    assert abs(res["score"] - want["score"]) <= 1e-12 and abs(res["margin"] - want["margin"]) <= 1e-12
