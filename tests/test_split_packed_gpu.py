"""The unsqueeze branch of k_split_sbs (csrc/v3d_pre.hip) on the MI355X: aligned-dword LDS window, v_perm_b32 pairs,
v_dot2_i32_i16 sums, one 16-bit store per output pair.  Every case is small and is held bit for bit to oracle.sbs_to_gray /
oracle.split_sbs on both eyes, through the C-ABI with the frame and the planes at the pitch and the byte offsets the case
names; the planes lie between guard bytes, so a store wider than the thread's outputs shows.

Geometry: W = 2056 (ow % 4 == 0, partial last block), 322 (ow % 4 == 2), 1030 (the last block holds six outputs), 64 and 16 (one
partial block; at 16 the eye is 8 pixels wide, narrower than a thread's 9-pixel window: every window holds replicated border
pixels); H = 9 is a band of 8 rows and a band of one, H = 3 a partial band.  (The widths are those at which a kernel that
stores four outputs as a dword changes its path, so that a later change of the outputs per thread meets them.)
Saturation: stripes of 1, 2 and 3 source pixels of 0 / 255 overshoot at every edge, in every channel; flat 0, flat 255, and one
channel at 255 beside two at 0 (a channel taken from the wrong byte of a pair selector shows there)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 16, 0x5A


def _frame(W, H, seed):
    sbs = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    sbs[:, W // 8:W // 6] = 255                                     # hard edges: the overshoot clamps
    sbs[:, W // 6:W // 5] = 0
    return sbs


@functools.lru_cache(maxsize=None)
def _want(key):
    """(frame, oracle gray pair, oracle BGR pair) of a named frame, computed once"""
    from oracle import oracle as O
    kind, W, H = key
    if kind == "random":
        sbs = _frame(W, H, W * 3 + H)
    elif kind.startswith("stripes"):
        p = int(kind[-1])
        sbs = np.empty((H, W, 3), np.uint8)
        sbs[:] = (((np.arange(W) // p) & 1) * 255).astype(np.uint8)[None, :, None]
    elif kind.startswith("flat"):
        sbs = np.full((H, W, 3), int(kind[4:]), np.uint8)
    else:                                                           # "only0" .. "only2": one channel at 255
        sbs = np.zeros((H, W, 3), np.uint8)
        sbs[:, :, int(kind[-1])] = 255
    return sbs, O.sbs_to_gray(sbs, True), O.split_sbs(sbs, True)


def _split(N, sbs, gray, pad=0, in_off=0, out_off=0):
    """v3d_sbs_to_gray / v3d_split_sbs, unsqueeze = 1: rows at pitch W * 3 + pad, the frame in_off and either plane out_off
    bytes behind a 256-byte boundary -> (left, right); the bytes around the planes must come back untouched"""
    import torch
    H, W, _ = sbs.shape
    pitch = W * 3 + pad
    src = np.full(in_off + (H - 1) * pitch + W * 3, 0xA5, np.uint8)
    for y in range(H):
        src[in_off + y * pitch:in_off + y * pitch + W * 3] = sbs[y].reshape(-1)
    buf = N.to_device(src)
    n_out = H * W * (1 if gray else 3)
    lead = GUARD + out_off
    planes = [torch.full((lead + n_out + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=buf.device) for _ in range(2)]
    assert buf.data_ptr() % 4 == 0 and all(p.data_ptr() % 4 == 0 for p in planes)
    N._call("v3d_sbs_to_gray" if gray else "v3d_split_sbs", buf.device, C.c_void_p(buf.data_ptr() + in_off), W, H, pitch, 1,
            C.c_void_p(planes[0].data_ptr() + lead), C.c_void_p(planes[1].data_ptr() + lead))
    got = []
    for p in planes:
        p = p.cpu().numpy()
        assert (p[:lead] == GUARD_BYTE).all() and (p[lead + n_out:] == GUARD_BYTE).all(), "a store left the output plane"
        got.append(p[lead:lead + n_out].reshape((H, W) if gray else (H, W, 3)))
    return got


def _check(N, key, **where):
    from conftest import mismatch_report
    sbs, want_gray, want_bgr = _want(key)
    for gray, want in ((True, want_gray), (False, want_bgr)):
        got = _split(N, sbs, gray, **where)
        for eye in (0, 1):
            msg = mismatch_report(got[eye], want[eye], f"{key} {'gray' if gray else 'bgr'} eye {eye} {where}")
            assert not msg, msg


@pytest.mark.parametrize("H", [9, 3])
@pytest.mark.parametrize("W", [2056, 322, 1030, 64, 16])
def test_geometry(native, W, H):
    _check(native, ("random", W, H))


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_pitch_and_base(native, off, pad):
    """W = 1076: rows of 3228 bytes, a multiple of 4, and ow % 4 == 0.  pad 5 makes the pitch odd: the byte staging plan.  A frame
    off bytes into its word stages aligned dwords from an unaligned base (pad 0); planes 1 or 3 bytes into theirs fail the
    alignment test of the wide stores and leave as bytes, which must equal the wide path's (off 0 and 2)"""
    _check(native, ("random", 1076, 9), pad=pad, in_off=off, out_off=off)


def test_planes_off_their_word_under_an_aligned_frame(native):
    """only the stores differ from the all-aligned case: the same staged dwords, byte stores at 1 and 3"""
    for off in (1, 2, 3):
        _check(native, ("random", 1076, 9), out_off=off)


@pytest.mark.parametrize("kind", ["stripes1", "stripes2", "stripes3", "flat255", "flat0", "only0", "only1", "only2"])
def test_saturating_patterns(native, kind):
    for W in (136, 138):                                            # ow % 4 == 0 and 2
        key = (kind, W, 3)
        _, _, want_bgr = _want(key)
        if kind.startswith("stripes"):                              # both ends of the clamp are met, in every channel
            both = np.concatenate(want_bgr, axis=1)
            for c in range(3):
                assert (both[..., c] == 0).any() and (both[..., c] == 255).any()
        _check(native, key)


@pytest.mark.parametrize("W", [2056, 322])
def test_gray_output_is_the_luma_of_the_bgr_output(native, oracle, W):
    sbs, _, _ = _want(("random", W, 9))
    gray, bgr = _split(native, sbs, True), _split(native, sbs, False)
    for eye in (0, 1):
        assert np.array_equal(gray[eye], oracle.bgr_to_gray(np.ascontiguousarray(bgr[eye])))
