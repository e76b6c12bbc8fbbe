"""Planes for the speckle filter's lock-free union-find (test helper): figures in which many roots merge at once, shared by the
emulated test (tests/test_speckle_emulated.py) and the GPU test (tests/test_sgbm_gpu.py::test_speckle_merge_shapes);
tests/test_speckle_shapes_host.py shows against scipy.ndimage.label and the oracle that they are what their names say.

shapes(W, H, max_size, max_diff, new_val) -> {name: int16 [H][W]}, the figures that fit into W x H:
  comb-bottom, comb-top   vertical teeth two columns apart, joined by one full row at the bottom / at the top
  spiral                  a one-pixel 4-connected spiral
  serpentine              full rows two apart, joined alternately at their right and left ends: it crosses every row boundary, so
                          every 16-row merge band's, left to right and back
  staircase               three-pixel runs, each two columns right of the one above: neighbours overlap in ONE pixel
  exact                   (H >= 34, max_size >= 84) two components of exactly max_size and max_size + 1 pixels, each a brickwork of
                          three runs per row over rows 14..17 and 30..33 joined by a one-pixel column, plus a tail in row 33
  plateaus                two pairs of adjacent plateaus of max_size pixels each: the values of the first pair differ by max_diff
                          (one component of 2 max_size), those of the second by max_diff + 1 (two of max_size)
  forks                   (rows 0..1 and, from 17 rows on, rows 15..16: both merge levels) a run of max_size - 1 pixels above a row
                          of one-pixel runs whose values alternate max_diff below and above it: each joins the run above, none
                          its neighbour.  2 (max_size - 1) pixels, kept -- unless a vertical union is skipped because the pixel
                          to its left "already joined the same two runs", which here are not the same two
  full-lists              every pixel a run of its own (every row's run list is full, without an end marker) above one row that
                          is a single run
The first five hold the figure at full size in the left part and, where the plane is wide enough, the same figure in a box small
enough to have at most max_size pixels in the right part: the large one survives only if every merge was made, the small one is
erased only if no size was counted twice."""
import numpy as np

V = 160                                                             # the value figures are drawn in


def comb(w, h, top=False):
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    m[0 if top else h - 1] = True
    return m


def spiral(w, h):
    """a walker that turns right whenever the cell ahead would touch the path anywhere but at the walker (or the border is reached):
    rings one cell apart"""
    m = np.zeros((h, w), bool)
    x = y = d = 0
    m[0, 0] = True
    step = [(1, 0), (0, 1), (-1, 0), (0, -1)]
    inside = lambda a, b: 0 <= a < w and 0 <= b < h
    while True:
        for _ in range(2):
            dx, dy = step[d]
            nx, ny = x + dx, y + dy
            if inside(nx, ny) and not m[ny, nx] and not any(inside(nx + a, ny + b) and m[ny + b, nx + a] for a, b in step if (nx + a, ny + b) != (x, y)):
                x, y = nx, ny
                m[y, x] = True
                break
            d = (d + 1) % 4
        else:
            return m


def serpentine(w, h):
    m = np.zeros((h, w), bool)
    m[::2] = True
    m[1::4, w - 1] = True
    m[3::4, 0] = True
    if h % 2 == 0:
        m[h - 1] = False                                        # a joint below the last full row would dangle
    return m


def staircase(w, h):
    m = np.zeros((h, w), bool)
    for y in range(min(h, (w - 3) // 2 + 1)):
        m[y, 2 * y:2 * y + 3] = True
    return m


FIGURES = {"comb-bottom": comb, "comb-top": lambda w, h: comb(w, h, True), "spiral": spiral, "serpentine": serpentine, "staircase": staircase}
EXACT_MIN = 84                                                      # the brickwork without a tail
EXACT_ROWS = (14, 15, 16, 17, 30, 31, 32, 33)


def exact(size):
    """one component of `size` >= EXACT_MIN pixels as rows [0, 34) of a mask: see the module's text"""
    w = 13 + size - EXACT_MIN
    m = np.zeros((34, w), bool)
    for y in EXACT_ROWS:
        for x0 in (0, 4, 8):
            m[y, x0 + 2 * (y & 1):x0 + 2 * (y & 1) + 3] = True
    m[18:30, 4] = True                                          # row 17 holds columns 2..4, row 30 columns 4..6
    m[33, 13:] = True                                           # the tail lengthens row 33's last run (columns 10..12)
    assert m.sum() == size
    return m


def _small(fig, W, H, max_size):
    """the figure in the largest box of at most 20 x 12 that keeps it at max_size pixels or fewer, None if there is none"""
    boxes = sorted(((w * h, w, h) for w in range(5, min(W, 12) + 1) for h in range(3, min(H, 20) + 1)), reverse=True)
    for _, w, h in boxes:
        m = fig(w, h)
        if 5 <= m.sum() <= max_size:
            return m
    return None


def shapes(W, H, max_size=100, max_diff=512, new_val=-16):
    out = {}
    blank = lambda: np.full((H, W), new_val, np.int16)
    for name, fig in FIGURES.items():
        if W < 8 or H < 3:
            continue
        small = _small(fig, W - 9, H, max_size) if W >= 32 else None
        wm = W if small is None else W - small.shape[1] - 1
        img = blank()
        img[:, :wm][fig(wm, H)] = V
        if small is not None:
            img[:small.shape[0], wm + 1:][small] = V
        out[name] = img
    if H >= 34 and max_size >= EXACT_MIN and 2 * (13 + max_size - EXACT_MIN) + 2 <= W:
        a, b = exact(max_size), exact(max_size + 1)
        img = blank()
        img[:34, :a.shape[1]][a] = V
        img[:34, a.shape[1] + 1:a.shape[1] + 1 + b.shape[1]][b] = V + 16
        out["exact"] = img
    pw = min(max_size, 8)
    ph = -(-max_size // pw)
    if 4 * pw + 1 <= W and ph <= H:
        plate = (np.arange(ph * pw) < max_size).reshape(ph, pw)
        img = blank()
        for x0, v in ((0, V), (pw, V + max_diff), (2 * pw + 1, V), (3 * pw + 1, V + max_diff + 1)):
            img[:ph, x0:x0 + pw][plate] = v
        out["plateaus"] = img
    if H >= 2 and 2 <= max_size - 1 <= W and V - max_diff != new_val:
        img = blank()
        for y in (0, 15) if H >= 17 else (0,):
            img[y, :max_size - 1] = V
            img[y + 1, :max_size - 1] = V + max_diff * (2 * (np.arange(max_size - 1) & 1) - 1)
        out["forks"] = img
    if H >= 2:
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.where((xx + yy) & 1, V, V + max_diff + 1).astype(np.int16)
        img[H - 1] = V + 2 * (max_diff + 1)
        out["full-lists"] = img
    return out


def extremes(W, H):
    """the planes of tests/test_sgbm_gpu.py::test_speckle_run_lists_extremes, restated: every pixel its own run, one run per row, W
    runs per row joined vertically, and random mixtures"""
    rng = np.random.default_rng(W * 31 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    return {
        "checkerboard": np.where((yy + xx) % 2 == 0, 0, 8000).astype(np.int16),
        "rows": (yy * 16).astype(np.int16) * np.ones((1, W), np.int16),
        "columns": np.where(xx % 2 == 0, 160, 9000).astype(np.int16),
        "random": (rng.integers(0, 6, (H, W)) * 700).astype(np.int16),
        "sparse": np.where(rng.random((H, W)) < 0.6, -16, (rng.integers(0, 4, (H, W)) * 300)).astype(np.int16),
    }
