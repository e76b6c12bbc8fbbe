"""v3d_eye_fidelity_batch on the GPU, bit-exact against tests/fidelity_ref.py: every cell size class (1 x 1, 2 x 2, 3 x 2, 11 x 5 =
55 of a wave's 64 lanes, 16 x 16, a map that does not enlarge), sizes that are no multiple of the cell, rows of cells that cross a
wave's columns and an item's rows, ncx / ncy at the edges of a window's fit and beyond one tile of the window stage, both eyes, the
eye as it lies in a full-SBS and in a full top-bottom output, batches with padded pitches and strides, the contents that reach the
ends of the arithmetic, workspace and records that hold garbage, and the refusals.

Which shape reaches which route of csrc/v3d_fidelity.hip (tests/launch_plan.py restates the entry's plan, tests/test_launch_plan_host.py
holds every line below against it):
  k_fid_cells  one item per wave: SIZES and everything built on them; a second item for 128 of the 1024 waves: 8192 x 130 at
               16 x 16 cells (test_wide_rows, 1152 items); the item stride proper (t[] carried over a second and a third item, fresh
               taps per item): LP.STRIDE_SHAPES, 70 columns (two waves across, the second with 6, 7 or 15 live lanes) by as many
               rows as give 2402 items, for every cell class and in both eyes for 4 x 2; a wave's next item in ANOTHER column of
               waves under SBS rows that every target row shares: LP.EMU_TAPS, 130 x 2730 against a one-row SBS frame;
  k_fid_ssim   one tile per workgroup: everything up to 200 x 120 (at most 36 tiles); the tile stride (q carried, the three LDS
               planes refilled behind the barrier): LP.TILE_SHAPES, 136 x 8408 (33 x 2101 windows: two tiles across, 526 tiles =
               two passes of the 256 workgroups and 14 tiles more), 9 x 8204 (one window across, 257 tiles: workgroup 0 alone walks
               on) and both at twice the size under 2 x 2 cells; at the first two the identical eye (n_win << 20 exactly) and at
               9 x 8204 the inverted one (a negative sum);
  the floor of 8 workgroups a frame, both stages: LP.TILE_FLOOR_CASE, 260 frames of 200 x 152 (76 items, 10 tiles);
  the frame stride of all three kernels (f += gridDim.y; scratch reused for a workgroup's second frame): LP.FRAMES_CASE, 65 538
               frames of 5 x 3 (no window: k_fid_ssim is not launched) and LP.FRAMES_WINDOW_CASE, 65 538 frames of 8 x 8 (one window
               each), 7 distinct frames repeated so that frame f and frame f + 65535 differ."""
import numpy as np
import pytest

import fidelity_ref as F
import launch_plan as LP
import stereo_source_ref as X

pytestmark = pytest.mark.gpu

MAPS = {"1x1": (65536, 0, 70000, 333), "2x2": (32768, -16384, 32768, -16384), "3x2": (21846, 0, 32768, 0), "11x5": (5958, 0, 13108, 0),
        "16x16": (4096, -5000, 4096, 77), "1x1-up": (1 << 20, -9000, 200000, 5 << 16), "4x2": (16384, -24576, 32768, -16384)}
# 200 x 120: at 1 x 1 cells 49 x 29 windows (more than one 32 x 8 tile either way), four waves across; 67 x 41: cut cells
SIZES = [(1, 1), (5, 3), (67, 41), (200, 120)]
_cache = {}


def _sbs(seed, n, Ws, Hs):
    return np.random.default_rng(seed).integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)


def _scene(W, H, name, n=1, eye=1):
    key = (W, H, name, n, eye)
    if key not in _cache:
        sbs = _sbs(W + H, n, 2 * max(2, W // 3), max(2, H // 2 + 1))
        E = F.V.disturbed(np.stack([X.eye_plane(s, eye, W, H, *MAPS[name]) for s in sbs]), W * H)
        _cache[key] = sbs, E, F.fidelity_batch(E, sbs, eye, *MAPS[name], 48)
    return _cache[key]


def _run(native, E, sbs, eye, m, thr, layout="alone", eye_phase=0, sbs_phase=0, rowpad=0, poison=0xA5):
    """E u8 [n,H,W,3] laid out as `layout` says at byte eye_phase of a 16-byte block; records and workspace pre-filled with
    `poison` -> the records int64 [n,6]; both images must stay as they are"""
    import torch
    n, H, W = E.shape[:3]
    other = np.random.default_rng(7).integers(0, 256, E.shape, dtype=np.uint8)
    full = {"alone": E, "sbs": np.concatenate([other, E], axis=2), "tb": np.concatenate([other, E], axis=1)}[layout]
    flat = torch.zeros(full.size + 32, dtype=torch.uint8, device="cuda")
    base = (-flat.data_ptr()) % 16 + eye_phase
    buf = flat[base:base + full.size].view(full.shape)
    buf.copy_(torch.from_numpy(full))
    view = {"alone": buf, "sbs": buf[:, :, W:], "tb": buf[:, H:]}[layout]
    Hs, Ws = sbs.shape[1:3]
    pitch = 3 * Ws + rowpad
    sflat = torch.full((n * Hs * pitch + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    sbase = (-sflat.data_ptr()) % 16 + sbs_phase
    sd = torch.as_strided(sflat, (n, Hs, Ws, 3), (Hs * pitch, pitch, 3, 1), sbase)
    sd.copy_(torch.from_numpy(sbs))
    need = native.lib().v3d_eye_fidelity_ws_bytes(n, W, H, m[0], m[2])
    assert need == LP.fidelity_plan(n, W, H, m[0], m[2]).ws_bytes > 0
    ws = torch.full((need,), poison, dtype=torch.uint8, device="cuda")
    out = torch.full((n, F.FIELDS), poison * 0x0101010101010101 - (1 << 64 if poison > 127 else 0), dtype=torch.int64, device="cuda")
    got = native.eye_fidelity_batch(view, sd, eye, *m, thr, out=out, ws=ws)
    assert got is out
    assert np.array_equal(buf.cpu().numpy(), full) and np.array_equal(sd.cpu().numpy(), sbs), "an image changed"
    return out.cpu().numpy()


def _check(native, E, sbs, eye, m, thr, want=None, **kw):
    want = F.fidelity_batch(E, sbs, eye, *m, thr) if want is None else want
    got = _run(native, E, sbs, eye, m, thr, **kw)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return want


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_and_cells(native, W, H, name):
    assert {k: F.V.cell(m[0], m[2]) for k, m in MAPS.items()} == {"1x1": (1, 1), "2x2": (2, 2), "3x2": (3, 2), "11x5": (11, 5),
                                                                   "16x16": (16, 16), "1x1-up": (1, 1), "4x2": (4, 2)}
    for eye in (0, 1):
        sbs, E, want = _scene(W, H, name, eye=eye)
        _check(native, E, sbs, eye, MAPS[name], 48, want)
        assert tuple(want[0, [0, 4]]) == (lambda g: (g[0] * g[1], g[2]))(native.fidelity_grid(W, H, MAPS[name][0], MAPS[name][2]))
        if (W, H) == (200, 120) and name in ("1x1", "2x2", "3x2"):
            assert want[0, 4] > 0 and 0 < want[0, 3] < want[0, 0]          # windows exist, the threshold decides both ways
    for thr in (0, 765):
        rec = _check(native, E, sbs, 1, MAPS[name], thr)
        assert thr != 765 or rec[0, 3] == 0


@pytest.mark.parametrize("name,c", [("1x1", 1), ("2x2", 2)])
def test_window_fits(native, name, c):
    """ncx and ncy at 7, 8, 11 and 12: 0, 1, 1 and 2 windows along that axis, the last cell cut"""
    for nc, nw in ((7, 0), (8, 1), (11, 1), (12, 2)):
        W, H = nc * c - (c - 1), 12 * c
        for w, h in ((W, H), (H, W)):
            sbs, E, want = _scene(w, h, name)
            assert want[0, 4] == 2 * nw
            _check(native, E, sbs, 1, MAPS[name], 48, want)


@pytest.mark.parametrize("layout,eye_phase,sbs_phase,rowpad", [("sbs", 0, 0, 0), ("tb", 0, 0, 0), ("sbs", 1, 3, 5), ("tb", 15, 7, 1),
                                                               ("alone", 15, 1, 0), ("alone", 1, 15, 7)])
def test_the_eye_as_it_lies_in_a_packed_output(native, layout, eye_phase, sbs_phase, rowpad):
    for (W, H), eye in (((67, 41), 1), ((200, 120), 0)):
        sbs, E, want = _scene(W, H, "4x2", eye=eye)
        _check(native, E, sbs, eye, MAPS["4x2"], 48, want, layout=layout, eye_phase=eye_phase, sbs_phase=sbs_phase, rowpad=rowpad)


def test_content(native):
    """identical (every window scores 2^20), noise, constants, 0 against 255 (the sums' headroom), inverted (negative Q)"""
    m = MAPS["2x2"]
    sbs = _sbs(4, 1, 2 * 60, 40)
    P = X.eye_plane(sbs[0], 1, 120, 80, *m)[None]
    assert _check(native, P, sbs, 1, m, 0)[0].tolist() == [2400, 0, 0, 0, 14 * 9, (14 * 9) << 20]
    assert _check(native, 255 - P, sbs, 1, m, 100)[0, 5] < 0
    _check(native, np.random.default_rng(5).integers(0, 256, P.shape, dtype=np.uint8), sbs, 1, m, 100)
    white = np.full((1, 40, 120, 3), 255, np.uint8)
    rec = _check(native, np.zeros((1, 80, 120, 3), np.uint8), white, 0, m, 764)
    assert rec[0].tolist()[:5] == [2400, 2400 * 765, 2400 * 3 * 255 * 255, 2400, 126]
    rec = _check(native, np.full((1, 80, 120, 3), 77, np.uint8), np.full((1, 40, 120, 3), 70, np.uint8), 1, m, 20)
    assert rec[0].tolist()[:4] == [2400, 2400 * 21, 2400 * 147, 2400]


def test_wide_rows(native):
    """one 3840-wide strip (60 waves across), an 8192-wide row of 1 x 1 cells, 8192 targets of 16 x 16 cells"""
    sbs = _sbs(1, 1, 3840, 9)
    _check(native, F.V.disturbed(X.eye_plane(sbs[0], 1, 3840, 18, *MAPS["4x2"])[None], 2), sbs, 1, MAPS["4x2"], 48, layout="sbs")
    sbs = _sbs(3, 1, 2 * 8192, 2)
    _check(native, F.V.disturbed(X.eye_plane(sbs[0], 1, 8192, 1, 65536, 0, 65536, 0)[None], 4), sbs, 1, (65536, 0, 65536, 0), 48, eye_phase=15)
    sbs = _sbs(5, 1, 2 * 512, 9)
    _check(native, F.V.disturbed(X.eye_plane(sbs[0], 0, 8192, 130, *MAPS["16x16"])[None], 6), sbs, 0, MAPS["16x16"], 24)


def _tall(W, H, name, n=1, eye=1):
    """as _scene, the SBS frames as tall as the map reaches, so that the rows a target blends keep moving down to the last item"""
    key = ("tall", W, H, name, n, eye)
    if key not in _cache:
        m = MAPS[name]
        sbs = _sbs(W + H + n, n, 2 * min((W * m[0] >> 16) + 2, 36), (H * m[2] >> 16) + 2)
        E = F.V.disturbed(np.stack([X.eye_plane(s, eye, W, H, *m) for s in sbs]), W * H + n)
        _cache[key] = sbs, E, F.fidelity_batch(E, sbs, eye, *m, 48)
    return _cache[key]


@pytest.mark.parametrize("name", list(MAPS))
def test_item_stride(native, name):
    """stage 1 at 2402 items for 1024 wave slots: every wave walks a second item, 354 of them a third"""
    assert set(MAPS) == set(LP.FIDELITY_CLASSES) and all(MAPS[k] == LP.MAPS[k] for k in MAPS)
    W, H = LP.STRIDE_SHAPES[name]
    for eye in ((0, 1) if name == "4x2" else (1,)):
        sbs, E, want = _tall(W, H, name, eye=eye)
        assert 0 < want[0, 3] < want[0, 0] and want[0, 1] > 0
        _check(native, E, sbs, eye, MAPS[name], 48, want)


def test_item_stride_into_another_column_of_waves(native):
    """LP.EMU_TAPS, the emulated twin's shape: three waves across and 1026 items, so a wave's second item lies one column of waves
    further, and a one-row SBS frame, so both items blend the same rows: taps kept from the first item would be another column's"""
    _, W, H = LP.EMU_TAPS
    sbs = _sbs(9, 1, 2 * W, 1)
    rec = _check(native, F.V.disturbed(X.eye_plane(sbs[0], 0, W, H, *LP.EMU_MAP)[None], 10), sbs, 0, LP.EMU_MAP, 48)
    assert 0 < rec[0, 3] < W * H and rec[0, 4] > 256


@pytest.mark.parametrize("W,H,name", LP.TILE_SHAPES)
def test_tile_stride(native, W, H, name):
    """stage 2 at more tiles than workgroups: 526 (two across: three passes, the last of 14) and 257 (workgroup 0 alone walks on)"""
    sbs, E, want = _tall(W, H, name)
    p = LP.fidelity_plan(1, W, H, MAPS[name][0], MAPS[name][2])
    assert want[0, 4] == p.nwx * p.nwy and p.tile_passes >= 2 and 0 < abs(want[0, 5]) < want[0, 4] << 20
    _check(native, E, sbs, 1, MAPS[name], 48, want, eye_phase=3, sbs_phase=1, rowpad=2)


@pytest.mark.parametrize("W,H,name", LP.TILE_SHAPES[:2])
def test_tile_stride_content(native, W, H, name):
    """the identical eye: every window scores 2^20, so a dropped or a doubled tile shows as a wrong multiple; the inverted eye:
    negative Q carried from tile to tile"""
    m = MAPS[name]
    sbs = _tall(W, H, name)[0]
    P = X.eye_plane(sbs[0], 1, W, H, *m)[None]
    ncx, ncy, n_win = native.fidelity_grid(W, H, m[0], m[2])
    assert _check(native, P, sbs, 1, m, 0)[0].tolist() == [ncx * ncy, 0, 0, 0, n_win, n_win << 20]
    if W < 100:
        assert _check(native, 255 - P, sbs, 1, m, 100)[0, 5] < -(n_win << 16)


@pytest.mark.parametrize("case,distinct", [(LP.TILE_FLOOR_CASE, 5), (LP.FRAMES_CASE, 7), (LP.FRAMES_WINDOW_CASE, 7)])
def test_long_batches(native, case, distinct):
    """the floor of 8 workgroups a frame in both stages, and more frames than the grid has rows (without windows: two launches;
    with one window a frame: all three): `distinct` frames repeated in order, every record checked"""
    n, W, H, name = case
    sbs, E, want = _scene(W, H, name, n=distinct) if n > 65535 else _tall(W, H, name, n=distinct)
    assert len({tuple(r) for r in want.tolist()}) == distinct and (n <= 65535 or 65535 % distinct)
    idx = np.arange(n) % distinct
    _check(native, E[idx], sbs[idx], 1, MAPS[name], 48, want[idx])


def test_a_batch_equals_single_calls_whatever_the_buffers_held(native):
    W, H = 67, 41
    sbs, E, want = _scene(W, H, "2x2", n=3)
    assert len({tuple(r) for r in want.tolist()}) == 3
    for layout in ("sbs", "tb"):
        _check(native, E, sbs, 1, MAPS["2x2"], 48, want, layout=layout, rowpad=5, eye_phase=3)
    for i in range(3):
        for poison in (0xA5, 0xFF, 0x00):
            got = _run(native, E[i:i + 1], sbs[i:i + 1], 1, MAPS["2x2"], 48, layout="sbs", rowpad=5, poison=poison)
            assert np.array_equal(got[0], want[i])
    assert np.array_equal(_run(native, E, sbs, 1, MAPS["2x2"], 48, poison=0xFF), want)


def test_after_the_source_render(native):
    """the convert step's sequence: the source render with fill_eyes 0 and 2 into a full-SBS and a full-TB output, the right eye
    measured with the render's own map and the left eye against the stored left eye; no byte of the output changes"""
    import stereo_sub_ref as S
    W, H, n = 200, 64, 2
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(k, H, W, 3 + i) for i, k in enumerate(("planar", "steep"))])
    sbs = _sbs(12, n, 2 * 100, 32)
    m, gains = MAPS["2x2"], (0, -(40 << 8), 0)
    for packing, view in ((native.STEREO_PACK_FULL_SBS, lambda o, e: o[:, :, e * W:(e + 1) * W]),
                          (native.STEREO_PACK_FULL_TB, lambda o, e: o[:, e * H:(e + 1) * H])):
        for fill in (0, 2):
            out = native.render_stereo_source_batch(native.to_device(frames), native.to_device(depth.view(np.int16)), *gains, packing,
                                                    native.to_device(sbs), fill, *m)
            before = out.cpu().numpy()
            for eye in (1, 0):
                got = native.eye_fidelity_batch(view(out, eye), native.to_device(sbs), eye, *m, 48).cpu().numpy()
                assert np.array_equal(got, F.fidelity_batch(np.ascontiguousarray(view(before, eye)), sbs, eye, *m, 48))
            assert np.array_equal(out.cpu().numpy(), before)


def test_python_surface_refusals(native):
    import torch
    sbs, E, _ = _scene(5, 3, "4x2")
    e, s = native.to_device(E), native.to_device(sbs)
    for bad in (dict(eye=2), dict(eye=True), dict(thr=-1), dict(thr=766), dict(thr=1.5)):
        kw = dict(eye=1, thr=48)
        kw.update(bad)
        with pytest.raises(ValueError):
            native.eye_fidelity_batch(e, s, kw["eye"], *MAPS["4x2"], kw["thr"])
    out = torch.full((1, F.FIELDS), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(native.NativeError):
        native.eye_fidelity_batch(e, torch.cat([s, s]), 1, *MAPS["4x2"], 48, out=out)
    with pytest.raises(native.NativeError):
        native.eye_fidelity_batch(e, s, 1, 4095, 0, 65536, 0, 48, out=out)
    with pytest.raises(native.NativeError):
        native.eye_fidelity_batch(e, s, 1, *MAPS["4x2"], 48, out=out, ws=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    # the raw entry: every refusal leaves the records as they were (tests/test_fidelity_guard_gpu.py holds the whole arena)
    import ctypes as C
    ws = torch.zeros(native.lib().v3d_eye_fidelity_ws_bytes(1, 5, 3, 16384, 32768), dtype=torch.uint8, device="cuda")
    for change in (dict(thr=766), dict(eye=2), dict(ax=4095), dict(ws=ws.data_ptr() + 8), dict(out=out.data_ptr() + 4)):
        a = dict(thr=48, eye=1, ax=16384, ws=ws.data_ptr(), out=out.data_ptr())
        a.update(change)
        rc = native.lib().v3d_eye_fidelity_batch(C.c_void_p(e.data_ptr()), 45, 15, 1, 5, 3, C.c_void_p(s.data_ptr()), s[0].numel(),
                                                 s.shape[2], s.shape[1], 3 * s.shape[2], a["eye"], a["ax"], -24576, 32768, -16384, a["thr"],
                                                 C.c_void_p(a["out"]), C.c_void_p(a["ws"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == -1, (change, rc)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all() and np.array_equal(e.cpu().numpy(), E)
    assert native.fidelity_grid(3840, 2160, 32768, 32768) == (1920, 1080, 479 * 269)
