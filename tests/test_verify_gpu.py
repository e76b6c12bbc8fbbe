"""v3d_verify_eye_source_batch on the GPU, bit-exact against tests/verify_ref.py: every size at which a cell is cut by the right or
the bottom edge or a wave holds a part of a row, every cell size class, both eyes, the eye as it lies in a full-SBS and in a full
top-bottom output, unaligned bases, pitched SBS rows, the threshold's edge, batches and the counters' overwrite.

Which shape reaches which route of k_verify_eye (tests/launch_plan.py restates the entry's plan, tests/test_launch_plan_host.py holds
every line below against it):
  one item per wave, the grid as wide as the frame has items for: SIZES, the packed layouts, the wide rows and the pipeline test
               (at most 128 items for 1024 wave slots; the pipeline's 1020 stay four short of them);
  the item stride, n = 1 (a wave's second and third item, `count` carried from item to item, fresh VfTaps and bad_bands per
               item): LP.STRIDE_SHAPES, 70 columns (two waves across, the second with 6, 7 or 15 live lanes) by as many rows as give
               2402 items: two passes of the 256 workgroups and a third of 354 items, for every cell class, in both eyes for 4 x 2
               and once inside a full-SBS buffer at an odd base with pitched SBS rows; in those shapes a wave's items lie in one
               column of waves (1024 is even), so a wave's next item in ANOTHER column, under SBS rows that every target row shares:
               LP.EMU_TAPS, 130 x 2730 (three waves across, 1026 items) against a one-row SBS frame;
  2048 / n workgroups a frame: LP.PER32_CASE, 64 frames of 134 items for 32 workgroups, the second pass 6 items long;
  the floor of 8 workgroups a frame: LP.FLOOR_CASE, 260 frames of 36 items = 9 workgroups wanted: workgroup 0 alone walks on;
  the frame stride (f += gridDim.y, wave_count reused for a workgroup's second frame): LP.FRAMES_CASE, 65 538 frames of 5 x 3 for
               a grid of 65 535 rows, 7 distinct frames repeated so that frame f and frame f + 65535 differ."""
import numpy as np
import pytest

import launch_plan as LP
import stereo_source_ref as X
import verify_ref as V

pytestmark = pytest.mark.gpu

# cells 4 x 2 (the 2x release of the pipeline tests), 1 x 1 (scale 1 and above), 16 x 16, cx = 4 from a non-integer ratio with
# cy = 1, and cells of 3 x 5: 21 cells = 63 lanes of a wave
MAPS = {"4x2": (16384, -24576, 32768, -16384), "1x1": (65536, 0, 70000, 333), "1x1-up": (1 << 20, -9000, 200000, 5 << 16),
        "16x16": (4096, -5000, 4096, 77), "4x1": (17000, 1 << 18, 65536, -(1 << 17)), "3x5": (21846, 0, 13108, 0)}
SIZES = [(1, 1), (5, 3), (67, 9), (530, 34)]
_cache = {}


def _noisy(seed, sbs, eye, W, H, m, share=0.15, amp=40):
    """eyes that agree with the stored eye up to noise, except for `share` of their pixels: cells fall on both sides of tau"""
    return V.disturbed(np.stack([X.eye_plane(s, eye, W, H, *m) for s in sbs]), seed, amp, share)


def _sbs(seed, n, Ws, Hs):
    return np.random.default_rng(seed).integers(0, 256, (n, Hs, Ws, 3), dtype=np.uint8)


def _scene(W, H, name, n=1, eye=1):
    key = (W, H, name, n, eye)
    if key not in _cache:
        sbs = _sbs(W + H, n, 2 * max(2, W // 3), max(2, H // 2 + 1))
        _cache[key] = sbs, _noisy(W * H, sbs, eye, W, H, MAPS[name])
    return _cache[key]


def _run(native, E, sbs, eye, m, tau, layout="alone", eye_phase=0, sbs_phase=0, rowpad=0, counts_before=0x5A5A5A5A):
    """E u8 [n,H,W,3] laid out as `layout` says at byte eye_phase of a 16-byte block -> (verified eyes, counters, the whole buffer
    before and after: what lies around the eye must stay)"""
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
    counts = torch.full((n,), counts_before, dtype=torch.int32, device="cuda")
    got = native.verify_eye_source_batch(view, sd, eye, *m, tau, out=counts)
    assert got is counts
    after = buf.cpu().numpy()
    out = {"alone": after, "sbs": after[:, :, W:], "tb": after[:, H:]}[layout]
    keep = {"alone": None, "sbs": after[:, :, :W], "tb": after[:, :H]}[layout]
    assert keep is None or np.array_equal(keep, other), "the other eye changed"
    assert np.array_equal(sd.cpu().numpy(), sbs)
    return out, counts.cpu().numpy().view(np.uint32)


def _check(native, E, sbs, eye, m, tau, **kw):
    want, counts = V.verify_batch(E, sbs, eye, *m, tau)
    got, c = _run(native, E, sbs, eye, m, tau, **kw)
    assert np.array_equal(c, counts), (c, counts)
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    return counts


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("W,H", SIZES)
def test_sizes_and_cells(native, W, H, name):
    assert {k: V.cell(m[0], m[2]) for k, m in MAPS.items()} == {"4x2": (4, 2), "1x1": (1, 1), "1x1-up": (1, 1), "16x16": (16, 16),
                                                                "4x1": (4, 1), "3x5": (3, 5)}
    for eye in (0, 1):
        sbs, E = _scene(W, H, name, eye=eye)
        for tau in (0, 48, 765):
            counts = _check(native, E, sbs, eye, MAPS[name], tau)
            assert tau != 765 or counts[0] == 0
        if W > 500:
            cx, cy = V.cell(MAPS[name][0], MAPS[name][2])
            assert 0 < V.verify(E[0], sbs[0], eye, *MAPS[name], 48)[1] < -(-W // cx) * -(-H // cy)   # tau 48 decides both ways


@pytest.mark.parametrize("layout,eye_phase,sbs_phase,rowpad", [("sbs", 0, 0, 0), ("tb", 0, 0, 0), ("sbs", 1, 3, 5), ("tb", 15, 7, 1),
                                                               ("alone", 15, 1, 0), ("alone", 1, 15, 7)])
def test_the_eye_as_it_lies_in_a_packed_output(native, layout, eye_phase, sbs_phase, rowpad):
    for W, H in ((67, 9), (530, 34)):
        sbs, E = _scene(W, H, "4x2")
        _check(native, E, sbs, 1, MAPS["4x2"], 48, layout=layout, eye_phase=eye_phase, sbs_phase=sbs_phase, rowpad=rowpad)


def test_wide_rows(native):
    """one 3840-wide band of 4 rows (60 waves across), one 8192-wide row of 1 x 1 cells against an eye of 8192"""
    sbs = _sbs(1, 1, 3840, 3)
    _check(native, _noisy(2, sbs, 1, 3840, 4, MAPS["4x2"]), sbs, 1, MAPS["4x2"], 48, layout="sbs")
    sbs = _sbs(3, 1, 2 * 8192, 2)
    _check(native, _noisy(4, sbs, 1, 8192, 1, (65536, 0, 65536, 0)), sbs, 1, (65536, 0, 65536, 0), 48, eye_phase=15)
    sbs = _sbs(5, 1, 2 * 512, 2)
    _check(native, _noisy(6, sbs, 0, 8192, 1, MAPS["16x16"]), sbs, 0, MAPS["16x16"], 24)


def _tall(W, H, name, n=1, eye=1):
    """as _scene, the SBS frames as tall as the map reaches, so that the rows a target blends keep moving down to the last item"""
    key = ("tall", W, H, name, n, eye)
    if key not in _cache:
        m = MAPS[name]
        sbs = _sbs(W + H + n, n, 2 * min((W * m[0] >> 16) + 2, 36), (H * m[2] >> 16) + 2)
        E = _noisy(W * H + n, sbs, eye, W, H, m)
        _cache[key] = sbs, E, V.verify_batch(E, sbs, eye, *m, 48)
    return _cache[key]


def _check_known(native, E, sbs, eye, m, tau, known, **kw):
    """_check against a reference computed before"""
    got, c = _run(native, E, sbs, eye, m, tau, **kw)
    assert np.array_equal(c, known[1]), (c, known[1])
    assert np.array_equal(got, known[0]), f"{int((got != known[0]).sum())} bytes differ"


@pytest.mark.parametrize("name", list(MAPS))
def test_item_stride(native, name):
    """2402 items for 1024 wave slots: every wave walks a second item, 354 of them a third; both verdicts occur in every pass"""
    assert set(MAPS) == set(LP.VERIFY_CLASSES) and all(MAPS[k] == LP.MAPS[k] for k in MAPS)
    W, H = LP.STRIDE_SHAPES[name]
    cx, cy = V.cell(MAPS[name][0], MAPS[name][2])
    for eye in ((0, 1) if name == "4x2" else (1,)):
        sbs, E, known = _tall(W, H, name, eye=eye)
        _check_known(native, E, sbs, eye, MAPS[name], 48, known)
        changed = (known[0] != E).any(axis=3)[0]                # the pixels that a replaced cell changed
        thirds = [changed[k * H // 3:(k + 1) * H // 3] for k in range(3)]
        assert 0 < known[1][0] < -(-W // cx) * -(-H // cy) and all(t.any() and not t.all() for t in thirds)


def test_item_stride_in_a_packed_output(native):
    W, H = LP.STRIDE_SHAPES["3x5"]
    sbs, E, known = _tall(W, H, "3x5")
    _check_known(native, E, sbs, 1, MAPS["3x5"], 48, known, layout="sbs", eye_phase=1, sbs_phase=3, rowpad=5)


def test_item_stride_into_another_column_of_waves(native):
    """LP.EMU_TAPS, the emulated twin's shape: three waves across and 1026 items, so a wave's second item lies one column of waves
    further, and a one-row SBS frame, so both items blend the same rows: taps kept from the first item would be another column's"""
    _, W, H = LP.EMU_TAPS
    sbs = _sbs(9, 1, 2 * W, 1)
    counts = _check(native, _noisy(10, sbs, 0, W, H, LP.EMU_MAP), sbs, 0, LP.EMU_MAP, 48)
    assert 0 < counts[0] < W * H


@pytest.mark.parametrize("case,distinct", [(LP.FLOOR_CASE, 5), (LP.PER32_CASE, 5), (LP.FRAMES_CASE, 7)])
def test_long_batches(native, case, distinct):
    """the floor of 8 workgroups a frame, 2048 / n = 32 of them, and more frames than the grid has rows: `distinct` frames
    repeated in order (frames are independent: test_a_batch_equals_single_calls...), every counter and every byte checked"""
    n, W, H, name = case
    if n > 65535:
        sbs = _sbs(3, distinct, 2, 2)                           # the smallest SBS frame there is
        E = _noisy(5, sbs, 1, W, H, MAPS[name], share=0.3)
        known = V.verify_batch(E, sbs, 1, *MAPS[name], 48)
        assert 65535 % distinct and len(set(known[1].tolist())) > 1            # frame f and frame f + 65535 differ
    else:
        sbs, E, known = _tall(W, H, name, n=distinct)
    assert len({e.tobytes() for e in known[0]}) == distinct
    idx = np.arange(n) % distinct
    _check_known(native, E[idx], sbs[idx], 1, MAPS[name], 48, (known[0][idx], known[1][idx]))


def test_threshold_edge(native):
    """tests/test_verify_ref.py's hand-computed cells: m == tau npix kept, one more replaced, a partial cell on its own npix"""
    m, tau = (16384, 0, 32768, 0), 48
    sbs = np.full((1, 4, 8, 3), 100, np.uint8)
    E = np.full((1, 4, 10, 3), 100, np.uint8)
    E[0, 0, 0], E[0, 0, 4] = (255, 0, 229), (255, 0, 230)
    E[0, 2, 8], E[0, 3, 9] = (196, 100, 100), (100, 4, 100)
    E[0, 2, 0], E[0, 2, 1] = (200, 100, 100), (0, 100, 100)
    got, c = _run(native, E, sbs, 1, m, tau)
    want = E.copy()
    want[0, 0, 4] = 100
    assert c.tolist() == [1] and np.array_equal(got, want)
    E[0, 3, 8] = (100, 100, 101)
    got, c = _run(native, E, sbs, 1, m, tau)
    want[0, 2:4, 8:10] = 100
    assert c.tolist() == [2] and np.array_equal(got, want)
    black, white = np.zeros((1, 12, 12, 3), np.uint8), np.full((1, 6, 24, 3), 255, np.uint8)
    assert _run(native, black, white, 0, (32768, 0, 32768, 0), 765)[1].tolist() == [0]
    got, c = _run(native, black, white, 0, (32768, 0, 32768, 0), 764)
    assert c.tolist() == [36] and (got == 255).all()


def test_a_batch_equals_single_calls_and_the_counters_are_overwritten(native):
    W, H = 67, 9
    sbs, E = _scene(W, H, "4x2", n=3)
    got, c = _run(native, E, sbs, 1, MAPS["4x2"], 48, layout="sbs", rowpad=5)
    assert len(set(c.tolist())) > 1
    for i in range(3):
        for before in (0, -1):
            g1, c1 = _run(native, E[i:i + 1], sbs[i:i + 1], 1, MAPS["4x2"], 48, layout="sbs", rowpad=5, counts_before=before)
            assert np.array_equal(g1[0], got[i]) and c1[0] == c[i]
    _check(native, E, sbs, 1, MAPS["4x2"], 48, layout="tb")


@pytest.mark.parametrize("subpixel", [False, True])
def test_after_the_source_render(native, subpixel):
    """the convert step's sequence: the source render into a full-SBS and a full-TB output, then the right eye verified in place
    with the render's own map; the left eye and the SBS frames stay"""
    import torch
    import stereo_sub_ref as S
    W, H, n = 530, 34, 2
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.stack([S.scene_depth(k, H, W, 3 + i) for i, k in enumerate(("planar", "steep"))])
    sbs = _sbs(12, n, 2 * 133, 17)
    m, gains = MAPS["4x2"], (0, -(40 << 8), 0)
    for packing, view in ((native.STEREO_PACK_FULL_SBS, lambda o: o[:, :, W:]), (native.STEREO_PACK_FULL_TB, lambda o: o[:, H:])):
        out = native.render_stereo_source_batch(native.to_device(frames), native.to_device(depth.view(np.int16)), *gains, packing,
                                                native.to_device(sbs), 2, *m, subpixel=subpixel)
        before = out.cpu().numpy()
        assert np.array_equal(before, np.stack([X.render(frames[i], depth[i], *gains, packing, subpixel, sbs[i], 2, *m) for i in range(n)]))
        counts = native.verify_eye_source_batch(view(out), native.to_device(sbs), 1, *m, 48)
        want, wc = V.verify_batch(np.ascontiguousarray(view(before)), sbs, 1, *m, 48)
        after = out.cpu().numpy()
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), wc) and wc.min() > 0
        assert np.array_equal(view(after), want)
        view(after)[...] = view(before)
        assert np.array_equal(after, before)                   # nothing but the right eye changed


def test_python_surface_refusals(native):
    import torch
    sbs, E = _scene(5, 3, "4x2")
    e, s = native.to_device(E), native.to_device(sbs)
    for bad in (dict(eye=2), dict(eye=True), dict(tau=-1), dict(tau=766), dict(tau=1.5)):
        kw = dict(eye=1, tau=48)
        kw.update(bad)
        with pytest.raises(ValueError):
            native.verify_eye_source_batch(e, s, kw["eye"], *MAPS["4x2"], kw["tau"])
    with pytest.raises(native.NativeError):
        native.verify_eye_source_batch(e, torch.cat([s, s]), 1, *MAPS["4x2"], 48)
    with pytest.raises(native.NativeError):
        native.verify_eye_source_batch(e, s, 1, 4095, 0, 65536, 0, 48)
    assert np.array_equal(e.cpu().numpy(), E) and native.verify_cell(16384, 32768) == (4, 2)
