"""The three colour-matching entries on the device, bit for bit against tests/colour_ref.py, through the binding (strided views of
one flat buffer give the odd bases, pitches and strides) and, for the refusals, through the raw library.

Which shape reaches which route of csrc/v3d_colour.hip:
  k_bgr_hist   a chunk inside the segment (one atomic per byte, no test): every width from 17 pixels on;
               a chunk at a segment's end (every byte tested): every case, and the only route of the widths 1 and 5;
               a lane's second item and items that wrap over a row end: 2731 x 37 (171 chunks a row, two rows to a band);
               one row longer than the workgroup's lanes: 4200 x 3 (263 chunks); a lane whose second item lies past the band: every
               band whose item count is no multiple of 512; several workgroups flushing into one histogram: 2731 x 37 (19 bands),
               300 x 200 constant (60 000 counts in one bin of each channel) and n = 3.
  k_colour_lut the cases of tests/test_colour_ref.py, among them the one a 64-bit compare gets wrong.
  k_bgr_lut<true>  (aligned 16-byte loads): in place at every phase, and out of place with both images at the same byte of a block;
  k_bgr_lut<false> (byte loads): out of place at different phases; both with whole blocks (one 16-byte store) and row ends (byte
               stores), one shared table and one per frame.
  col_band     rows per workgroup from the lanes' fill: every case above; from the frame count (8 workgroups a frame, the floor):
               130 frames of 171 x 210, both kernels (tests/test_launch_plan_host.py holds it against tests/launch_plan.py)."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as CR
from test_colour_ref import lut_cases

pytestmark = pytest.mark.gpu
_cache = {}


def _big():
    """one random 2760 x 40 image; every histogram case is a rectangle of it at some base"""
    if "big" not in _cache:
        _cache["big"] = np.random.default_rng(7).integers(0, 256, (1, 40, 2760, 3), dtype=np.uint8)
    return _cache["big"]


def _place(torch, F, base, rowpad, framepad, poison=0xA5):
    """frames [n,H,W,3] -> (flat poisoned device buffer, strided view of it that starts `base` bytes in)"""
    n, H, W, _ = F.shape
    pitch = 3 * W + rowpad
    stride = H * pitch + framepad
    flat = torch.full((base + n * stride + 64,), poison, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(flat, (n, H, W, 3), (stride, pitch, 3, 1), base)
    view.copy_(torch.from_numpy(np.ascontiguousarray(F)).cuda())
    return flat, view


def _hist(native, F, rect, base=1, rowpad=0, framepad=0):
    import torch
    _, view = _place(torch, F, base, rowpad, framepad)
    out = torch.full((F.shape[0], 3, 256), -1, dtype=torch.int32, device="cuda")       # any content: the entry zeroes it
    got = native.bgr_hist_batch(view, rect, out=out).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, CR.hist(F, rect)), f"rect {rect} base {base} rowpad {rowpad}"


@pytest.mark.parametrize("h", [1, 37])
@pytest.mark.parametrize("w", [1, 5, 16, 17, 341, 2731])
def test_histogram_widths_and_heights(native, w, h):
    F = _big()
    for k, x0 in enumerate((0, 1, 2, 7, 29)):
        if x0 + w <= F.shape[2]:
            _hist(native, F, (x0, k % 3, x0 + w, k % 3 + h), base=2 * k + 1, rowpad=k)


def test_histogram_every_phase_of_a_block(native):
    """x0 = 0 .. 15 with the image base at an odd byte: the segment starts at all 16 bytes of a block (3 x0 + 1 mod 16 is a
    permutation), and the odd pitch moves it on from row to row"""
    F = _big()[:, :9, :120]
    assert sorted((3 * x0 + 1) % 16 for x0 in range(16)) == list(range(16))
    for x0 in range(16):
        for w in (5, 17, 100):
            _hist(native, F, (x0, 0, x0 + w, 9), base=1, rowpad=x0 % 2)


def test_histogram_contended_whole_single_and_batch(native):
    _hist(native, np.full((1, 200, 300, 3), 131, np.uint8), (0, 0, 300, 200), base=0)
    F = _big()
    _hist(native, F, (0, 0, 2760, 40), base=3)
    _hist(native, F, (2759, 39, 2760, 40), base=3)
    _hist(native, F, (0, 0, 1, 1), base=0)
    _hist(native, np.random.default_rng(8).integers(0, 256, (1, 3, 4200, 3), dtype=np.uint8), (0, 0, 4200, 3), base=5, rowpad=3)
    F3 = np.random.default_rng(9).integers(0, 256, (3, 50, 333, 3), dtype=np.uint8)
    F3[1] = F3[1] // 64 * 64                                   # four levels: a frame of its own must not leak into its neighbours
    _hist(native, F3, (0, 0, 333, 50), base=7, rowpad=5, framepad=11)
    _hist(native, F3, (10, 3, 300, 47), base=8, rowpad=16, framepad=48)


def test_histogram_refusals(native):
    import torch
    L = native.lib()
    img = torch.zeros(2 * 4 * 18, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3, 256), 7, dtype=torch.int32, device="cuda")
    P, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(bgr=P(img.data_ptr()), fs=72, n=2, W=6, H=4, pitch=18, x0=0, y0=0, x1=6, y1=4, hist=P(out.data_ptr()))
    bad = [dict(bgr=None), dict(hist=None), dict(n=0), dict(n=65536), dict(W=0), dict(H=0), dict(W=65536, pitch=3 * 65536), dict(H=65536),
           dict(pitch=17), dict(fs=71), dict(x0=-1), dict(y0=-1), dict(x1=7), dict(y1=5), dict(x0=6), dict(x0=3, x1=3), dict(y0=2, y1=2),
           dict(y0=3, y1=2)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.v3d_bgr_hist_batch(a["bgr"], a["fs"], a["n"], a["W"], a["H"], a["pitch"], a["x0"], a["y0"], a["x1"], a["y1"], a["hist"], st)
        assert rc == -1 and L.v3d_last_error(), change
    assert L.v3d_bgr_hist_batch(ok["bgr"], 0, 1, 6, 4, 18, 0, 0, 6, 4, ok["hist"], st) == 0        # one frame: the stride is ignored
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[1] == 7).all() and got[0, :, 0].tolist() == [24, 24, 24] and got[0].sum() == 72


@pytest.mark.parametrize("case", lut_cases(), ids=lambda c: c[0])
def test_tables(native, case):
    import torch
    name, s, d, group, _ = case
    dev = lambda h: torch.from_numpy(h.astype(np.uint32).view(np.int32)).cuda()
    got = native.colour_lut_batch(dev(s), dev(d), group).cpu().numpy()
    want = CR.lut(s, d, group)
    assert got.shape == want.shape and np.array_equal(got, want), name
    assert (np.diff(got.astype(int), axis=2) >= 0).all()


def test_table_refusals(native):
    import torch
    L = native.lib()
    h = torch.zeros((2, 3, 256), dtype=torch.int32, device="cuda")
    out = torch.full((2, 3, 256), 9, dtype=torch.uint8, device="cuda")
    P, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((None, P(h.data_ptr()), 2, 1, P(out.data_ptr())), (P(h.data_ptr()), None, 2, 1, P(out.data_ptr())),
                 (P(h.data_ptr()), P(h.data_ptr()), 2, 1, None), (P(h.data_ptr()), P(h.data_ptr()), 0, 1, P(out.data_ptr())),
                 (P(h.data_ptr()), P(h.data_ptr()), 2, 0, P(out.data_ptr())), (P(h.data_ptr()), P(h.data_ptr()), 2, 3, P(out.data_ptr()))):
        assert L.v3d_colour_lut_batch(*args, st) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 9).all()
    with pytest.raises(ValueError):
        native.colour_lut_batch(h, h, 3)


def _apply(native, F, T, rect, in_place, sbase=0, dbase=0, srowpad=0, drowpad=0, sframepad=0, dframepad=0):
    import torch
    n, H, W, _ = F.shape
    x0, y0, x1, y1 = rect
    sflat, sview = _place(torch, F, sbase, srowpad, sframepad)
    before = sflat.cpu().numpy().copy()
    lut = torch.from_numpy(T).cuda()
    want = CR.apply(F, T, rect)
    inside = np.zeros(F.shape, bool)
    inside[:, y0:y1, x0:x1] = True
    if in_place:
        assert native.bgr_lut_batch(sview, lut, rect, out=sview) is sview
        assert np.array_equal(sview.cpu().numpy(), want)
        after = sflat.cpu().numpy()
        idx = torch.as_strided(torch.arange(sflat.numel()), sview.shape, sview.stride(), sbase).numpy()
        keep = np.ones(after.size, bool)
        keep[idx[inside]] = False
        assert np.array_equal(after[keep], before[keep]), "a byte outside the rectangle changed"
        return
    dflat, dview = _place(torch, np.full(F.shape, 0x5A, np.uint8), dbase, drowpad, dframepad, poison=0x5A)
    native.bgr_lut_batch(sview, lut, rect, out=dview)
    got = dview.cpu().numpy()
    assert np.array_equal(got[inside], want[inside])
    assert (got[~inside] == 0x5A).all() and (dflat.cpu().numpy() == 0x5A).sum() == dflat.numel() - int((got[inside] != 0x5A).sum())
    assert np.array_equal(sflat.cpu().numpy(), before)


def test_apply_in_place_at_every_phase(native):
    rng = np.random.default_rng(1)
    F = rng.integers(0, 256, (2, 6, 210, 3), dtype=np.uint8)
    shared, per = rng.integers(0, 256, (3, 256), dtype=np.uint8), rng.integers(0, 256, (2, 3, 256), dtype=np.uint8)
    for ph in range(16):
        _apply(native, F, per if ph % 2 else shared, (105 - ph % 5, ph % 2, 210 - ph % 3, 6), True, sbase=ph, srowpad=ph % 4, sframepad=ph % 7)
    _apply(native, F, shared, (0, 0, 210, 6), True)
    _apply(native, F, per, (209, 5, 210, 6), True, sbase=3)


def test_apply_out_of_place_both_routes(native):
    rng = np.random.default_rng(2)
    T = rng.integers(0, 256, (3, 3, 256), dtype=np.uint8)
    F = rng.integers(0, 256, (3, 40, 333, 3), dtype=np.uint8)
    _apply(native, F, T, (0, 0, 333, 40), False, sbase=6, dbase=6, srowpad=2, drowpad=18, sframepad=3, dframepad=35)       # same phase
    _apply(native, F, T, (7, 1, 300, 39), False, sbase=6, dbase=22, srowpad=2, drowpad=18, sframepad=3, dframepad=35)
    for dbase in (0, 7, 15):                                                                                          # different phases
        _apply(native, F, T[0], (7, 1, 300, 39), False, sbase=3, dbase=dbase, srowpad=1, drowpad=4, dframepad=9)
    F = rng.integers(0, 256, (1, 2, 1500, 3), dtype=np.uint8)                   # 282 blocks a row: more than the workgroup's lanes
    _apply(native, F, T[1], (1, 0, 1500, 2), False, sbase=1, dbase=1)
    _apply(native, F, T[1], (1499, 1, 1500, 2), False, sbase=1, dbase=2)
    import torch                                                               # the binding's own outputs
    src = torch.from_numpy(F).cuda()
    assert np.array_equal(native.bgr_lut_batch(src, torch.from_numpy(T[2]).cuda()).cpu().numpy(), CR.apply(F, T[2]))
    assert np.array_equal(native.bgr_lut_batch(src, torch.from_numpy(T[2]).cuda(), (5, 0, 900, 1)).cpu().numpy(), CR.apply(F, T[2], (5, 0, 900, 1)))
    assert np.array_equal(src.cpu().numpy(), F)


def test_bands_decided_by_the_frame_count(native):
    """col_band gives a workgroup as many rows as fill its 256 lanes once, or ceil(rows / max(1024 / n, 8)) where that is more
    (tests/launch_plan.py).  Every case above has the former; LP.COLOUR_BAND_CASE, 130 frames of 171 x 210, has the latter in
    k_bgr_hist (27 rows for 24) and k_bgr_lut (27 for 8): 8 workgroups a frame, the last with 21 rows.  Five distinct frames
    repeated in order"""
    import launch_plan as LP
    n, W, H = LP.COLOUR_BAND_CASE
    rng = np.random.default_rng(130)
    base = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    base[1] = base[1] // 64 * 64
    F = base[np.arange(n) % 5]
    _hist(native, F, (0, 0, W, H), base=1, rowpad=2, framepad=5)
    _hist(native, F, (3, 0, W - 2, H), base=0)
    T = rng.integers(0, 256, (n, 3, 256), dtype=np.uint8)
    _apply(native, F, T, (0, 0, W, H), False, sbase=6, dbase=6, srowpad=2, drowpad=18, sframepad=3, dframepad=35)
    _apply(native, F, T[0], (3, 0, W - 2, H), False, sbase=3, dbase=7, srowpad=1)
    _apply(native, F, T, (0, 0, W, H), True, sbase=5, srowpad=3)


def test_apply_refusals(native):
    import torch
    L = native.lib()
    img = torch.full((2 * 4 * 18 + 18,), 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * 4 * 18,), 4, dtype=torch.uint8, device="cuda")
    lut = torch.zeros(768, dtype=torch.uint8, device="cuda")
    P, st = C.c_void_p, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(src=P(img.data_ptr()), ss=72, n=2, W=6, H=4, pitch=18, x0=0, y0=0, x1=6, y1=4, lut=P(lut.data_ptr()), ls=0, dst=P(dst.data_ptr()),
              ds=72, dp=18)
    bad = [dict(src=None), dict(lut=None), dict(dst=None), dict(n=0), dict(W=0), dict(H=65536), dict(pitch=17), dict(dp=17), dict(ss=71),
           dict(ds=71), dict(x1=7), dict(y1=5), dict(x0=2, x1=2), dict(y0=-1), dict(ls=1), dict(ls=767), dict(ls=-768),
           dict(dst=P(img.data_ptr() + 18)), dict(dst=P(img.data_ptr()), dp=19, ds=80), dict(dst=P(img.data_ptr()), ds=73)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.v3d_bgr_lut_batch(a["src"], a["ss"], a["n"], a["W"], a["H"], a["pitch"], a["x0"], a["y0"], a["x1"], a["y1"], a["lut"], a["ls"],
                                 a["dst"], a["ds"], a["dp"], st)
        assert rc == -1 and L.v3d_last_error(), change
    torch.cuda.synchronize()
    assert (img.cpu().numpy() == 3).all() and (dst.cpu().numpy() == 4).all()
