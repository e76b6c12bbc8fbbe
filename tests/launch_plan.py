"""The launch plans of the entries whose grid depends on n x size, restated in plain Python from the host code of csrc/ (no GPU, no
library): how many workgroups a call launches and how often each of them walks on with the grid's stride.  The GPU and emulated
tests take their shapes from the tables below, and tests/test_launch_plan_host.py asserts for every one of them the regime it is
there to reach, and pins this restatement to what the library shows of itself (v3d_eye_fidelity_ws_bytes, native.fidelity_grid,
native.verify_cell).  A cap retuned in csrc/ without this file fails there; retuned in both, a shape that no longer reaches its
regime fails there as well.

Terms: `items` the units of work of one frame, `grid_x` the workgroups per frame, `passes` = ceil(items / (units a grid_x-wide
row of workgroups takes at once)): passes >= 2 means that the stride is taken, passes >= 3 with items no multiple of a pass that
a workgroup carries its state over a full second pass into a partial third."""
from collections import namedtuple

# ---- v3d_verify.hip / v3d_fidelity.hip ----
VF_ROWS, VF_BLOCKS, FF_BLOCKS, FF_TW, FF_TH, GRID_Y_MAX = 8, 256, 256, 32, 8, 65535
LAUNCH_BLOCKS, FLOOR_BLOCKS = 2048, 8              # workgroups per launch aimed at; per frame at least

VerifyPlan = namedtuple("VerifyPlan", "cell items grid_x grid_y passes cw waves")       # waves: across a row
FidelityPlan = namedtuple("FidelityPlan", "cell items grid_x grid_y passes tiles g2 tile_passes ncx ncy nwx nwy plane_bytes ws_bytes")


def cdiv(a, b):
    return -(-a // b)


def cell(ax, ay):
    return (65536 + ax - 1) // ax, (65536 + ay - 1) // ay


def per_frame(n, cap):
    """workgroups per frame at most: about 2048 per launch, at most `cap`, at least 8"""
    per = LAUNCH_BLOCKS // n
    return cap if per > cap else FLOOR_BLOCKS if per < FLOOR_BLOCKS else per


def _stage1(n, W, H, ax, ay, cap):
    cx, cy = cell(ax, ay)
    ncy = cdiv(H, cy)
    bands = 1 if cy >= VF_ROWS else VF_ROWS // cy
    cw = 64 // cx * cx
    nwx = cdiv(W, cw)
    items = nwx * cdiv(ncy, bands)
    grid_x = min(cdiv(items, 4), per_frame(n, cap))
    return (cx, cy), items, grid_x, min(n, GRID_Y_MAX), cdiv(items, 4 * grid_x), cw, nwx


def verify_plan(n, W, H, ax, ay):
    """v3d_verify_eye_source_batch: a wave owns an item, a workgroup four"""
    return VerifyPlan(*_stage1(n, W, H, ax, ay, VF_BLOCKS))


def fidelity_plan(n, W, H, ax, ay):
    """v3d_eye_fidelity_batch: stage 1 as verify_plan, stage 2 a workgroup per tile of 32 x 8 windows; ws_bytes as ff_plan lays the
    workspace out"""
    (cx, cy), items, g1, gy, passes, _, _ = _stage1(n, W, H, ax, ay, FF_BLOCKS)
    ncx, ncy = cdiv(W, cx), cdiv(H, cy)
    nwx, nwy = ((ncx - 8) // 4 + 1 if ncx >= 8 else 0), ((ncy - 8) // 4 + 1 if ncy >= 8 else 0)
    if not nwx or not nwy:
        nwx = nwy = 0
    tiles = cdiv(nwx, FF_TW) * cdiv(nwy, FF_TH)
    g2 = min(tiles, per_frame(n, FF_BLOCKS))
    plane = cdiv(ncy * cdiv(ncx, 4) * 4 * 2, 16) * 16
    return FidelityPlan((cx, cy), items, g1, gy, passes, tiles, g2, cdiv(tiles, g2) if g2 else 0, ncx, ncy, nwx, nwy, plane,
                        n * plane + n * g1 * 24 + n * g2 * 8)


# the maps of tests/test_verify_gpu.py and tests/test_fidelity_gpu.py (ax, bx, ay, by) by cell class
MAPS = {"4x2": (16384, -24576, 32768, -16384), "1x1": (65536, 0, 70000, 333), "1x1-up": (1 << 20, -9000, 200000, 5 << 16),
        "16x16": (4096, -5000, 4096, 77), "4x1": (17000, 1 << 18, 65536, -(1 << 17)), "3x5": (21846, 0, 13108, 0),
        "2x2": (32768, -16384, 32768, -16384), "3x2": (21846, 0, 32768, 0), "11x5": (5958, 0, 13108, 0)}

# item stride, n = 1: thin tall eyes, two waves across (the second with W - cw live lanes), 2402 items = two passes of 1024 and 354
STRIDE_SHAPES = {"1x1": (70, 9604), "1x1-up": (70, 9604), "4x2": (70, 9607), "4x1": (70, 9604), "3x5": (70, 6003), "16x16": (70, 19205),
                 "2x2": (70, 9607), "3x2": (70, 9607), "11x5": (70, 6003)}
VERIFY_CLASSES = ("4x2", "1x1", "1x1-up", "16x16", "4x1", "3x5")
FIDELITY_CLASSES = ("1x1", "2x2", "3x2", "11x5", "16x16", "1x1-up", "4x2")
# (n, W, H, class): the floor of 8 workgroups a frame; 2048 / n = 32 a frame; more frames than the grid's y holds
FLOOR_CASE = (260, 70, 140, "4x2")
PER32_CASE = (64, 70, 530, "4x2")
FRAMES_CASE = (65538, 5, 3, "4x2")
# fidelity's stage 2: (W, H, class), tiles past the 256 workgroups; its floor of 8; one window a frame, all three launches
TILE_SHAPES = [(136, 8408, "1x1"), (9, 8204, "1x1"), (272, 16816, "2x2"), (18, 16408, "2x2")]
TILE_FLOOR_CASE = (260, 200, 152, "1x1")
FRAMES_WINDOW_CASE = (65538, 8, 8, "1x1")
# the emulated twins (tests/test_verify_emulated.py, tests/test_fidelity_emulated.py): (n, W, H), 1 x 1 cells of (65536, 0, 65536, 0)
EMU_MAP = (65536, 0, 65536, 0)
EMU_STRIDE = (1, 5, 8200)              # 1025 items, one wave across: workgroup 0's wave 0 alone walks a second item
EMU_TAPS = (1, 130, 2730)              # three waves across, 1026 items: a wave's second item lies in ANOTHER column of waves, and
                                       # under a one-row SBS frame every row blends the same rows: taps kept across items are stale
EMU_TILES = (1, 9, 8204)               # 257 tiles: workgroup 0 alone walks a second tile
EMU_FLOOR_VERIFY = (260, 3, 257)       # 33 items = 9 workgroups wanted, 8 launched
EMU_FLOOR_FIDELITY = (260, 9, 264)     # the same 33 items, and 9 tiles for 8 workgroups


# ---- the older entries ----
CUTS_CASE = (66, 515, 255)             # T, W, H (tests/test_temporal_gpu.py): 32 workgroups a pair for 33 wanted
RANGE_FLOOR_CASE = (20, 135, 240)      # n, H, W (tests/test_temporal_gpu.py): the floor of 64 blocks a frame
BLEND_CASES = [(1920, 1080), (515, 510)]                      # W, H (tests/test_blend_gpu.py)
FILL_BAND_CASES = [(13, 5, 701), (185, 5, 701)]               # n, W, H (tests/test_fill_gpu.py): 5 and 64 rows a workgroup
PRE_CASES = {"v3d_bgr_to_gray": (1449, 1451), "v3d_disp_to_depth": (1025, 1031), "v3d_round_to_u16": (1449, 1451)}  # H, W
COLOUR_BAND_CASE = (130, 171, 210)     # n, W, H (tests/test_colour_gpu.py)
COL_CHUNK = 48                         # bytes a lane of k_bgr_hist owns; k_bgr_lut's lanes own 16


def temporal_sad_plan(T, W, H, aligned):
    """v3d_temporal_cuts, k_tp_sad: -> (bx, vec_passes, tail_passes, tail): steps of a lane in the 16-byte loop and in the byte
    loop behind it, and the pixels the byte loop has"""
    npx = W * H
    bx = min(max(cdiv(npx, 4096), 1), max(LAUNCH_BLOCKS // (T - 1), 32))
    nvec = npx // 16 if aligned else 0
    tail = npx - 16 * nvec
    return bx, cdiv(nvec, 256 * bx), cdiv(tail, 256 * bx), tail


def mono_blend_plan(W, H):
    """v3d_mono_blend_batch, k_mono_blend -> (blocks per frame, passes)"""
    blocks = min(cdiv(W * H, 256), 1024)
    return blocks, cdiv(W * H, 256 * blocks)


def fill_band(n, H):
    """v3d_fill_holes_disp16_batch: rows per workgroup of k_fill_rows"""
    return min(max(cdiv(n * H, 2048), 4), 64)


PRE_CAPS = {"v3d_disp_to_depth": 2048, "v3d_round_to_u16": 4096, "v3d_bgr_to_gray": 4096}


def pre_plan(entry, elems):
    """the flat kernels of v3d_pre.hip -> (blocks, passes)"""
    blocks = min(cdiv(elems, 256), PRE_CAPS[entry])
    return blocks, cdiv(elems, 256 * blocks)


def frame_blocks(elems, n, floor, px=256):
    """v3d_range.hip: blocks per frame of k_minmax / k_norm_u16 (floor 64) -> (blocks, passes)"""
    blocks = min(cdiv(elems, px), max(1024 // n, floor))
    return blocks, cdiv(elems, px * blocks)


def col_band(rows, n, nb, bytes_per_lane):
    """v3d_colour.hip: rows per workgroup of k_bgr_hist (16-byte chunks) and k_bgr_lut -> (band, bands per frame, True where the
    1024 / n cap and not the 256-lane fill decides the band)"""
    per = max(1024 // n, 8)
    fill, band = cdiv(256 * bytes_per_lane, nb), cdiv(rows, per)
    return max(band, fill), cdiv(rows, max(band, fill)), band > fill
