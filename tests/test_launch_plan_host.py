"""tests/launch_plan.py held against the library (the workspace size it reports, the binding's grid helpers) and, shape by shape,
against the regime each GPU and emulated case is there to reach.  A cap retuned in csrc/ moves v3d_eye_fidelity_ws_bytes away
from the restatement; a shape that stops striding after a retune of both fails its own line below.  No GPU."""
import pytest

import launch_plan as LP

ALL = {"verify": LP.VERIFY_CLASSES, "fidelity": LP.FIDELITY_CLASSES}


def _sized_cases():
    """(n, W, H, class) of every new case of the two entries"""
    out = [(1,) + LP.STRIDE_SHAPES[k] + (k,) for k in LP.STRIDE_SHAPES]
    out += [LP.FLOOR_CASE, LP.PER32_CASE, LP.FRAMES_CASE, LP.TILE_FLOOR_CASE, LP.FRAMES_WINDOW_CASE]
    out += [(1, W, H, k) for W, H, k in LP.TILE_SHAPES]
    return out


def test_the_restated_workspace_is_the_librarys():
    """ws = n planes + n g1 slots of 24 bytes + n g2 slots of 8: g1 and g2 are the grids, so every cap and floor shows in it"""
    from video_3d_pipeline import _native as N
    lib = N.lib()
    cases = [(n, W, H, LP.MAPS[k]) for n, W, H, k in _sized_cases()]
    cases += [(n, W, H, LP.EMU_MAP) for n, W, H in (LP.EMU_STRIDE, LP.EMU_TAPS, LP.EMU_TILES, LP.EMU_FLOOR_VERIFY, LP.EMU_FLOOR_FIDELITY)]
    for n in (1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 260, 2048, 2049, 65535, 65536):
        for W, H in ((1, 1), (5, 3), (67, 41), (200, 120), (200, 152), (8192, 130), (3840, 2160), (136, 8408), (9, 8204)):
            if n * W * H <= 1 << 31:
                cases += [(n, W, H, m) for m in LP.MAPS.values()]
    assert len(cases) > 500
    for n, W, H, m in cases:
        p = LP.fidelity_plan(n, W, H, m[0], m[2])
        assert lib.v3d_eye_fidelity_ws_bytes(n, W, H, m[0], m[2]) == p.ws_bytes == n * p.plane_bytes + n * p.grid_x * 24 + n * p.g2 * 8, (n, W, H, m)
        assert N.fidelity_grid(W, H, m[0], m[2]) == (p.ncx, p.ncy, p.nwx * p.nwy) and N.verify_cell(m[0], m[2]) == p.cell
        v = LP.verify_plan(n, W, H, m[0], m[2])
        assert (v.cell, v.items, v.grid_x, v.grid_y, v.passes) == p[:5]           # VF_BLOCKS == FF_BLOCKS: one stage-1 plan for both
    p = LP.fidelity_plan(1, 3840, 2160, *LP.MAPS["4x2"][::2])
    assert (p.items, p.grid_x, p.passes, p.tiles, p.tile_passes) == (16200, 256, 16, 8 * 34, 2)     # what the convert CLI runs at 4K


def test_what_the_cases_from_before_reach():
    """the largest shapes of the suites as they were: no item stride in the verify entry, one partial second pass in stage 1 of the
    fidelity entry, no tile stride, no n above 3"""
    m = LP.MAPS
    for W, H, k in ((530, 34, "4x2"), (3840, 4, "4x2"), (8192, 1, "16x16"), (67, 9, "4x2")):
        assert LP.verify_plan(3, W, H, m[k][0], m[k][2]).passes == 1
    p = LP.verify_plan(2, 960, 540, m["4x2"][0], m["4x2"][2])
    assert (p.items, p.passes) == (1020, 1)
    p = LP.fidelity_plan(1, 8192, 130, m["16x16"][0], m["16x16"][2])
    assert (p.items, p.grid_x, p.passes) == (1152, 256, 2)
    for k in LP.FIDELITY_CLASSES:
        p = LP.fidelity_plan(1, 200, 120, m[k][0], m[k][2])
        assert p.passes == 1 and p.tile_passes <= 1 and p.tiles <= 8


@pytest.mark.parametrize("entry", ["verify", "fidelity"])
def test_item_stride_shapes(entry):
    """n = 1: the cap of 256 workgroups, two full passes and a partial third, two waves across with a few live lanes in the second"""
    plan = LP.verify_plan if entry == "verify" else LP.fidelity_plan
    for k in ALL[entry]:
        (W, H), m = LP.STRIDE_SHAPES[k], LP.MAPS[k]
        p = plan(1, W, H, m[0], m[2])
        assert p.grid_x == 256 and 2048 < p.items < 3072 and p.items % 1024 and p.passes == 3, (k, p)
        cw = 64 // p.cell[0] * p.cell[0]
        assert cw < W <= 2 * cw and W - cw < 16, k                          # so a wave's items, 1024 apart, lie in one column of waves
        assert H % p.cell[1] or p.cell[1] == 1, k                           # the last row of cells is cut wherever a cell has rows
    assert LP.fidelity_plan(1, 70, 6003, LP.MAPS["11x5"][0], LP.MAPS["11x5"][2]).cell == (11, 5)


def test_batch_regimes():
    for plan in (LP.verify_plan, LP.fidelity_plan):
        n, W, H, k = LP.FLOOR_CASE
        p = plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
        assert 2048 // n < 8 and (p.items, p.grid_x, p.passes, p.grid_y) == (36, 8, 2, n)       # 9 workgroups wanted
        n, W, H, k = LP.PER32_CASE
        p = plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
        assert p.grid_x == 32 == 2048 // n and p.passes >= 2 and p.items % 128
        n, W, H, k = LP.FRAMES_CASE
        p = plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
        assert p.grid_y == 65535 < n and p.grid_x == 1
    n, W, H, k = LP.FRAMES_CASE
    assert LP.fidelity_plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2]).g2 == 0               # no window: two launches
    n, W, H, k = LP.FRAMES_WINDOW_CASE
    p = LP.fidelity_plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
    assert p.grid_y == 65535 < n and (p.grid_x, p.g2, p.nwx * p.nwy) == (1, 1, 1)
    n, W, H, k = LP.TILE_FLOOR_CASE
    p = LP.fidelity_plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
    assert (p.tiles, p.g2, p.tile_passes) == (10, 8, 2) and (p.grid_x, p.passes) == (8, 3) and p.items % 32


def test_tile_stride_shapes():
    want = {(136, 8408, "1x1"): (33, 2101, 526, 3), (9, 8204, "1x1"): (1, 2050, 257, 2),
            (272, 16816, "2x2"): (33, 2101, 526, 3), (18, 16408, "2x2"): (1, 2050, 257, 2)}
    assert set(want) == set(LP.TILE_SHAPES)
    for (W, H, k), v in want.items():
        p = LP.fidelity_plan(1, W, H, LP.MAPS[k][0], LP.MAPS[k][2])
        assert (p.nwx, p.nwy, p.tiles, p.tile_passes) == v and p.g2 == 256 and p.tiles % 256
    p = LP.fidelity_plan(1, 136, 8408, LP.MAPS["1x1"][0], LP.MAPS["1x1"][2])
    assert p.tile_passes >= 3 and p.passes >= 3                             # a carried q and carried t[] over two full passes


def test_emulated_shapes():
    a = LP.EMU_MAP
    for plan in (LP.verify_plan, LP.fidelity_plan):
        p = plan(*LP.EMU_STRIDE, a[0], a[2])
        assert (p.items, p.grid_x, p.passes) == (1025, 256, 2) and LP.EMU_STRIDE[1] <= 64
        p = plan(*LP.EMU_TAPS, a[0], a[2])
        # a wave's items are 4 grid_x apart: with three waves across, its second item lies one column of waves further
        assert (p.items, p.grid_x, p.passes) == (1026, 256, 2) and LP.cdiv(LP.EMU_TAPS[1], 64) == 3 and 4 * p.grid_x % 3 == 1
    p = LP.verify_plan(*LP.EMU_FLOOR_VERIFY, a[0], a[2])
    assert (p.items, p.grid_x, p.passes) == (33, 8, 2)
    p = LP.fidelity_plan(*LP.EMU_FLOOR_FIDELITY, a[0], a[2])
    assert (p.items, p.grid_x, p.passes, p.tiles, p.g2, p.tile_passes) == (33, 8, 2, 9, 8, 2)
    p = LP.fidelity_plan(*LP.EMU_TILES, a[0], a[2])
    assert (p.tiles, p.g2, p.tile_passes) == (257, 256, 2)
    # as small as the plan allows: one item or one tile fewer and 8 workgroups are all that is wanted
    assert LP.verify_plan(260, 3, 256, a[0], a[2]).passes == 1 and LP.fidelity_plan(260, 9, 260, a[0], a[2]).tile_passes == 1


def test_every_regime_is_reached_by_some_case():
    """per kernel: a second full pass, a partial last pass, the floor of the grid and grid_y < n"""
    v = [(1,) + LP.STRIDE_SHAPES[k] + (k,) for k in LP.VERIFY_CLASSES] + [LP.FLOOR_CASE, LP.PER32_CASE, LP.FRAMES_CASE]
    f = [(1,) + LP.STRIDE_SHAPES[k] + (k,) for k in LP.FIDELITY_CLASSES] + [(1, W, H, k) for W, H, k in LP.TILE_SHAPES]
    f += [LP.TILE_FLOOR_CASE, LP.FRAMES_CASE, LP.FRAMES_WINDOW_CASE]
    v = [LP.verify_plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2]) for n, W, H, k in v]
    f = [LP.fidelity_plan(n, W, H, LP.MAPS[k][0], LP.MAPS[k][2]) for n, W, H, k in f]
    for plans in (v, f):
        assert any(p.passes >= 3 for p in plans) and any(p.passes >= 2 and p.items % (4 * p.grid_x) for p in plans)
        assert any(p.grid_x == 8 and p.passes >= 2 for p in plans) and any(p.grid_y == 65535 for p in plans)
    assert any(p.tile_passes >= 3 for p in f) and any(p.tile_passes >= 2 and p.tiles % p.g2 for p in f)
    assert any(p.g2 == 8 and p.tile_passes >= 2 for p in f) and any(p.grid_y == 65535 and p.g2 for p in f)       # k_fid_ssim, k_fid_reduce


# ---- the older entries whose plan depends on n x size ----
def test_temporal_cuts_case_strides_in_both_loops():
    """k_tp_sad: the sized cases of test_cuts stop at 9 x 270 x 480 (32 workgroups wanted, 256 allowed, one 16-byte step a lane)"""
    assert LP.temporal_sad_plan(9, 480, 270, True)[:3] == (32, 1, 0) and LP.temporal_sad_plan(4, 256, 128, True)[:2] == (8, 1)
    T, W, H = LP.CUTS_CASE
    assert LP.temporal_sad_plan(T, W, H, True) == (32, 2, 1, 13)               # 8207 steps for 8192 lanes, 13 pixels in the byte loop
    assert LP.temporal_sad_plan(T, W, H, False) == (32, 0, 17, W * H)          # 16 full passes of the byte loop and 253 pixels
    assert LP.cdiv(W * H, 4096) == 33 and 2048 // (T - 1) < 32 and (W * H) % 16 and (W * H + 3) % 16 == 0


def test_mono_blend_cases_pass_the_cap():
    assert [LP.mono_blend_plan(W, H) for W, H in LP.BLEND_CASES] == [(1024, 8), (1024, 2)]
    assert LP.mono_blend_plan(320, 180) == (225, 1) and all(W * H % (256 * 1024) for W, H in LP.BLEND_CASES)    # partial last passes


def test_fill_band_cases():
    assert [LP.fill_band(n, H) for n, W, H in LP.FILL_BAND_CASES] == [5, 64]
    assert all(H % LP.fill_band(n, H) for n, W, H in LP.FILL_BAND_CASES)
    assert LP.fill_band(4, 1080) == LP.fill_band(3, 700) == LP.fill_band(1, 1) == 4        # what the cases from before reach
    assert LP.fill_band(185, 701) == LP.fill_band(65535, 4320) == 64 and LP.cdiv(185 * 701, 2048) == 64    # reached, not only clamped to


def test_flat_kernels_pass_their_caps():
    for entry, (H, W) in LP.PRE_CASES.items():
        blocks, passes = LP.pre_plan(entry, H * W)
        assert blocks == LP.PRE_CAPS[entry] and passes == 3 and (H * W) % (256 * blocks), entry     # two full passes and a partial one
    assert LP.pre_plan("v3d_disp_to_depth", 200 * 333)[1] == LP.pre_plan("v3d_round_to_u16", 50306)[1] == LP.pre_plan("v3d_bgr_to_gray", 33 * 71)[1] == 1


def test_range_and_colour_regimes():
    """k_minmax / k_norm_u16: tests/test_temporal_gpu.py's test_range_normalisation reaches the cap of 1024 / n blocks at
    3 x 1080 x 1920 and, with LP.RANGE_FLOOR_CASE, the floor of 64; test_minmax_and_range has the floor for k_minmax at the same
    shape.  col_band: of the sized cases of tests/test_colour_gpu.py only LP.COLOUR_BAND_CASE lets the frame count decide"""
    assert LP.frame_blocks(1080 * 1920, 3, 64) == (341, 24) and (1080 * 1920) % (256 * 341)
    n, H, W = LP.RANGE_FLOOR_CASE
    assert LP.frame_blocks(H * W, n, 64) == (64, 2) and 1024 // n < 64 and (H * W) % (256 * 64)
    assert LP.frame_blocks(131 * 257, 5, 64)[1] == 1
    n, W, H = LP.COLOUR_BAND_CASE
    assert LP.col_band(H, n, 3 * W, LP.COL_CHUNK) == (27, 8, True) and LP.col_band(H, n, 3 * W, 16) == (27, 8, True) and H % 27
    assert LP.col_band(H, n, 3 * (W - 5), LP.COL_CHUNK)[2]                      # the narrower rectangle of the same test
    for rows, k, nb in ((37, 1, 3 * 2731), (200, 1, 900), (40, 1, 3 * 2760), (50, 3, 999), (6, 2, 630), (40, 3, 999)):
        assert not LP.col_band(rows, k, nb, LP.COL_CHUNK)[2] and not LP.col_band(rows, k, nb, 16)[2]
    assert LP.col_band(37, 1, 3 * 2731, LP.COL_CHUNK)[:2] == (2, 19)            # tests/test_colour_gpu.py: "19 bands", two rows each
