"""v3d_fuse_eye_source_batch on the GPU, bit-exact against tests/fuse_ref.py: small and ragged eyes under maps whose clamps engage
on both sides of both axes, both eyes, the eye as it lies in a full-SBS and in a full top-bottom output, padded pitches and
strides at odd bases, saturating inputs, and the shapes at which the two kernels take another route:

  k_fuse_means   one group of 64 samples a row (the small sizes); 15 and 17 groups (3840 and 4100 columns); a footprint wider than
                 the workgroup under a clamp (530 columns on one sample: the strided column loop) and taller than a row chunk (34
                 rows on one sample row); more rows than a 32-bit column sum takes (2^20 + 5 rows on one sample row: the flush);
  k_fuse_apply   whole runs of four targets and cut ones (W = 1, 5, 67, 530), one and more workgroups across a row;
  both           as many workgroups as items (the small sizes); the stride over items at 2048 workgroups (3840 x 2160: 16 200 and
                 8 640 items); 2048 / n of them and the floor of 8 a frame (64 and 260 frames); more frames than the grid has rows
                 (65 538 frames of 5 x 3)."""
import numpy as np
import pytest

import fuse_ref as F

pytestmark = pytest.mark.gpu

MAPS = [(14500, -70000, 25000, 3000), (65536, 0, 65536, 0), (4096, 1 << 20, 4096, -(1 << 18)), (60000, 123456, 30000, -99999)]
FOUR_BY_TWO = (16384, -24576, 32768, -16384)                   # the 2x release of the pipeline tests
# (W, H, Ws, Hs)
SIZES = [(1, 1, 2, 1), (5, 3, 4, 2), (64, 24, 32, 12), (67, 29, 46, 15)]
_known = {}


def _scene(seed, n, W, H, Ws, Hs):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8), rng.integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)


def _strided(flat, base, shape, pitch, stride):
    """a [n,rows,cols,3] view of a flat byte array (NumPy or torch alike) at byte `base`"""
    n, rows, cols, _ = shape
    if isinstance(flat, np.ndarray):
        return np.lib.stride_tricks.as_strided(flat[base:], shape, (stride, pitch, 3, 1))
    import torch
    return torch.as_strided(flat, shape, (stride, pitch, 3, 1), base)


def _run(native, E, sbs, eye, m, layout="alone", eye_phase=0, sbs_phase=0, rowpad=0, eye_rowpad=0, eye_framepad=0, ws_fill=0xC3):
    """E u8 [n,H,W,3] laid out as `layout` says at byte eye_phase of a 16-byte block, rows eye_rowpad and frames eye_framepad bytes
    apart from dense -> the fused eyes; the other eye, every padding byte and the SBS frames must have stayed"""
    import torch
    n, H, W = E.shape[:3]
    other = np.random.default_rng(7).integers(0, 256, E.shape, dtype=np.uint8)
    full = {"alone": E, "sbs": np.concatenate([other, E], axis=2), "tb": np.concatenate([other, E], axis=1)}[layout]
    oh, ow = full.shape[1:3]
    pitch = 3 * ow + eye_rowpad
    stride = oh * pitch + eye_framepad
    host = np.full(n * stride + 32, 0x77, np.uint8)
    _strided(host, 16 + eye_phase, full.shape, pitch, stride)[...] = full
    flat = torch.from_numpy(host).cuda()
    skew = (-flat.data_ptr()) % 16
    assert skew == 0                                            # the caching allocator's blocks are 512-byte aligned
    buf = _strided(flat, 16 + eye_phase, full.shape, pitch, stride)
    view = {"alone": buf, "sbs": buf[:, :, W:], "tb": buf[:, H:]}[layout]
    Hs, Ws = sbs.shape[1:3]
    sp = 3 * Ws + rowpad
    sflat = torch.full((n * Hs * sp + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    sd = _strided(sflat, sbs_phase, sbs.shape, sp, Hs * sp)
    sd.copy_(torch.from_numpy(sbs))
    ws = torch.full((native.fuse_eye_source_ws_bytes(n, Ws, Hs),), ws_fill, dtype=torch.uint8, device="cuda")
    assert native.fuse_eye_source_batch(view, sd, eye, *m, ws=ws) is view
    after = flat.cpu().numpy()
    got = _strided(after, 16 + eye_phase, full.shape, pitch, stride)
    out = np.array({"alone": got, "sbs": got[:, :, W:], "tb": got[:, H:]}[layout])
    {"alone": got, "sbs": got[:, :, W:], "tb": got[:, H:]}[layout][...] = E
    assert np.array_equal(after, host), "a byte outside the eye's payload changed"
    assert np.array_equal(sd.cpu().numpy(), sbs)
    return out


def _check(native, E, sbs, eye, m, want=None, **kw):
    want = F.fuse_batch(E, sbs, eye, *m) if want is None else want
    got = _run(native, E, sbs, eye, m, **kw)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[0].tolist()}"
    return want


@pytest.mark.parametrize("m", MAPS)
@pytest.mark.parametrize("W,H,Ws,Hs", SIZES)
def test_sizes_and_maps(native, W, H, Ws, Hs, m):
    E, sbs = _scene(W * H, 1, W, H, Ws, Hs)
    for eye in (0, 1):
        want = _check(native, E, sbs, eye, m)
        assert W * H == 1 or (want != E).any()


def test_the_clamps_engage_on_both_sides_of_both_axes():
    """what the maps are there for, at 67 x 29 over a 23 x 15 eye: targets below 0 and above the last sample, in x and in y"""
    lo = {"x": False, "y": False}
    hi = dict(lo)
    for ax, bx, ay, by in MAPS:
        for k, a, b, Nd, Ns in (("x", ax, bx, 67, 23), ("y", ay, by, 29, 15)):
            lo[k] |= b < 0
            hi[k] |= a * (Nd - 1) + b > (Ns - 1) << 16
    assert all(lo.values()) and all(hi.values())


@pytest.mark.parametrize("layout,eye_phase,sbs_phase,rowpad", [("sbs", 0, 0, 0), ("tb", 0, 0, 0), ("sbs", 1, 3, 5), ("tb", 15, 7, 1),
                                                               ("alone", 15, 1, 0), ("alone", 1, 15, 7)])
def test_the_eye_as_it_lies_in_a_packed_output(native, layout, eye_phase, sbs_phase, rowpad):
    for (W, H, Ws, Hs), m in (((67, 29, 46, 15), MAPS[0]), ((64, 24, 32, 12), FOUR_BY_TWO)):
        E, sbs = _scene(W + H, 1, W, H, Ws, Hs)
        _check(native, E, sbs, 1, m, layout=layout, eye_phase=eye_phase, sbs_phase=sbs_phase, rowpad=rowpad)


@pytest.mark.parametrize("layout", ["alone", "sbs", "tb"])
def test_a_padded_batch_at_an_odd_base_equals_single_calls(native, layout):
    W, H, Ws, Hs = 67, 29, 46, 15
    E, sbs = _scene(3, 3, W, H, Ws, Hs)
    want = _check(native, E, sbs, 1, MAPS[3], layout=layout, eye_phase=5, sbs_phase=3, rowpad=5, eye_rowpad=7, eye_framepad=11)
    assert len({w.tobytes() for w in want}) == 3
    for i in range(3):
        assert np.array_equal(_run(native, E[i:i + 1], sbs[i:i + 1], 1, MAPS[3], layout=layout)[0], want[i])


def test_saturating_inputs(native):
    for m in MAPS:
        for e, s in ((255, 0), (0, 255)):
            E, sbs = np.full((1, 9, 14, 3), e, np.uint8), np.full((1, 5, 12, 3), s, np.uint8)
            assert (_check(native, E, sbs, 0, m) == s).all()
    # 255 - 64 + 255 and 0 - 191 + 0: both clamps cut (tests/test_fuse_ref.py)
    import stereo_source_ref as X
    E = np.zeros((1, 8, 16, 3), np.uint8)
    E[:, :, ::4] = 255
    m = X.identity_map(4, 16) + X.identity_map(4, 8)
    want = _check(native, E, np.full((1, 4, 8, 3), 255, np.uint8), 1, m)
    assert (want[:, :, ::4] == 255).all() and (want[:, :, 1::4] == 191).all()
    want = _check(native, 255 - E, np.zeros((1, 4, 8, 3), np.uint8), 1, m)
    assert (want[:, :, ::4] == 0).all() and (want[:, :, 1::4] == 64).all()


def test_wide_and_clamped_footprints(native):
    """4100 columns over 1025 samples (17 groups of samples, 5 workgroups across a row); one sample that owns all 530 columns and one
    sample row that owns all 34 rows (the smallest scales, offsets beyond the eye)"""
    E, sbs = _scene(1, 1, 4100, 6, 2 * 1025, 4)
    _check(native, E, sbs, 1, (16384, -24576, 32768, -16384), layout="sbs", eye_phase=3)
    E, sbs = _scene(2, 1, 530, 34, 32, 12)
    assert F.footprint_counts(4096, 1 << 20, 530, 16)[1].tolist() == [530] and F.footprint_counts(4096, -(1 << 18), 34, 12)[1].tolist() == [34]
    _check(native, E, sbs, 0, MAPS[2])
    _check(native, E, sbs, 1, MAPS[0], eye_phase=1)


def test_more_rows_than_a_column_sum_takes(native):
    """one column of 2^20 + 5 rows that all lie nearest to sample row 0: the 32-bit sums are flushed once on the way"""
    H = (1 << 20) + 5
    E, sbs = _scene(4, 1, 1, H, 4, 3)
    m = (65536, 0, 4096, -(1 << 40))
    assert F.footprint_counts(m[2], m[3], H, 3)[1].tolist() == [H]
    want = _check(native, E, sbs, 1, m)
    assert (want != E).any()


def _full_frame():
    if "4k" not in _known:
        E, sbs = _scene(5, 1, 3840, 2160, 1920, 1080)
        _known["4k"] = E, sbs, F.fuse_batch(E, sbs, 1, *FOUR_BY_TWO)
    return _known["4k"]


def test_a_full_frame_strides_over_the_items(native):
    """3840 x 2160 over a 960 x 1080 eye inside a full-SBS output: 16 200 groups of samples and 8 640 row pieces for 2048 workgroups"""
    E, sbs, want = _full_frame()
    _check(native, E, sbs, 1, FOUR_BY_TWO, want=want, layout="sbs")


@pytest.mark.parametrize("n,W,H,Ws,Hs,distinct", [(64, 70, 140, 36, 72, 5), (260, 70, 140, 36, 72, 5), (65538, 5, 3, 4, 2, 7)])
def test_long_batches(native, n, W, H, Ws, Hs, distinct):
    """2048 / n = 32 workgroups a frame for 140 and 72 items, the floor of 8, and more frames than the grid has rows: `distinct`
    frames repeated in order, so that frame f and frame f + 65535 differ"""
    E, sbs = _scene(n, distinct, W, H, Ws, Hs)
    want = F.fuse_batch(E, sbs, 1, *FOUR_BY_TWO)
    assert (n <= 65535 or 65535 % distinct) and len({w.tobytes() for w in want}) == distinct
    idx = np.arange(n) % distinct
    _check(native, E[idx], sbs[idx], 1, FOUR_BY_TWO, want=want[idx])


def test_twice_on_copies_gives_the_same_bytes_whatever_the_workspace_held(native):
    E, sbs = _scene(6, 2, 530, 34, 2 * 133, 17)
    a = _run(native, E, sbs, 1, FOUR_BY_TWO, layout="sbs", ws_fill=0x00)
    b = _run(native, E, sbs, 1, FOUR_BY_TWO, layout="sbs", ws_fill=0xFF)
    assert np.array_equal(a, b) and np.array_equal(a, F.fuse_batch(E, sbs, 1, *FOUR_BY_TWO))


def test_after_the_source_render_and_the_verification(native):
    """the convert step's sequence on the device: source render, verification, fusion of the same right eye under the same map"""
    import stereo_source_ref as X
    import stereo_sub_ref as S
    import verify_ref as V
    W, H, n = 530, 34, 2
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(k, H, W, 3 + i) for i, k in enumerate(("planar", "steep"))])
    sbs = rng.integers(0, 256, (n, 17, 2 * 133, 3), dtype=np.uint8)
    m, gains = FOUR_BY_TWO, (0, -(40 << 8), 0)
    for packing, view in ((native.STEREO_PACK_FULL_SBS, lambda o: o[:, :, W:]), (native.STEREO_PACK_FULL_TB, lambda o: o[:, H:])):
        out = native.render_stereo_source_batch(native.to_device(frames), native.to_device(depth.view(np.int16)), *gains, packing,
                                                native.to_device(sbs), 2, *m)
        native.verify_eye_source_batch(view(out), native.to_device(sbs), 1, *m, 48)
        native.fuse_eye_source_batch(view(out), native.to_device(sbs), 1, *m)
        want = np.stack([X.render(frames[i], depth[i], *gains, packing, False, sbs[i], 2, *m) for i in range(n)])
        eye = V.verify_batch(np.ascontiguousarray(view(want)), sbs, 1, *m, 48)[0]
        view(want)[...] = F.fuse_batch(eye, sbs, 1, *m)
        assert np.array_equal(out.cpu().numpy(), want)


def test_python_surface_refusals(native):
    import torch
    E, sbs = _scene(9, 1, 5, 3, 4, 2)
    e, s = native.to_device(E), native.to_device(sbs)
    for eye in (2, -1):
        with pytest.raises(ValueError):
            native.fuse_eye_source_batch(e, s, eye, *FOUR_BY_TWO)
    with pytest.raises(native.NativeError):
        native.fuse_eye_source_batch(e, torch.cat([s, s]), 1, *FOUR_BY_TWO)
    with pytest.raises(native.NativeError):
        native.fuse_eye_source_batch(e, s, 1, 65537, 0, 65536, 0)
    with pytest.raises(native.NativeError):
        native.fuse_eye_source_batch(e, s, 1, *FOUR_BY_TWO, ws=torch.empty(16, dtype=torch.uint8, device="cuda")[:8])
    with pytest.raises(native.NativeError):
        native.fuse_eye_source_ws_bytes(1, 5, 2)
    assert np.array_equal(e.cpu().numpy(), E)
    assert native.fuse_eye_source_ws_bytes(1, 4, 2) == 16 and native.fuse_eye_source_ws_bytes(3, 1920, 1080) == 3 * 1080 * 960 * 3
