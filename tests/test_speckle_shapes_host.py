"""tests/speckle_shapes.py is not vacuous (CPU): against scipy.ndimage.label and the C oracle, the figures' components have the
sizes their names say, `exact` flips between kept and erased at the threshold, and every shape changes under at least one of the
thresholds the emulated test and the GPU test run it with."""
import numpy as np
import pytest
from scipy.ndimage import label

import speckle_shapes as SS

THRESHOLDS = lambda H: [(100, 512), (H, 100), (3, 1)]
SIZES = [(640, 48), (516, 35), (1920, 33), (300, 40), (72, 48), (64, 17), (64, 9)]


def _sizes(mask):
    lab, n = label(mask)
    return sorted(np.bincount(lab.ravel())[1:].tolist(), reverse=True)


@pytest.mark.parametrize("w,h", [(8, 3), (31, 16), (64, 33), (201, 48)])
def test_each_figure_is_one_component_of_the_stated_kind(w, h):
    for name, fig in SS.FIGURES.items():
        m = fig(w, h)
        assert len(_sizes(m)) == 1, name
    assert SS.comb(w, h).sum() == (w + 1) // 2 * (h - 1) + w and SS.comb(w, h, True)[0].all() and not SS.comb(w, h)[0, 1]
    sp = SS.spiral(w, h)
    nb = sum(np.roll(np.pad(sp, 1), s, a)[1:-1, 1:-1] for s, a in ((1, 0), (-1, 0), (1, 1), (-1, 1)))
    assert nb[sp].max() <= 2 and (nb[sp] == 1).sum() == 2 and sp.sum() > w + h           # a path: two ends, no branch, more than one side
    se = SS.serpentine(w, h)
    assert all(se[y].any() and se[y + 1].any() for y in range(h - 2))                  # every row boundary is crossed ...
    assert all(_sizes(se[y:y + 2])[0] == se[y:y + 2].sum() for y in range(h - 2))      # ... by one joint
    assert [int(np.flatnonzero(se[y])[0]) for y in range(1, h - 1, 2)][:2] == ([w - 1, 0][:len(range(1, h - 1, 2))])
    st = SS.staircase(w, h)
    rows = min(h, (w - 3) // 2 + 1)
    assert st.sum() == 3 * rows and all((st[y] & st[y + 1]).sum() == 1 for y in range(rows - 1))


@pytest.mark.parametrize("size", [84, 100, 101, 517])
def test_exact_has_its_size_and_three_runs_per_row(size):
    m = SS.exact(size)
    assert _sizes(m) == [size]
    for y in SS.EXACT_ROWS:
        assert np.diff(np.r_[0, m[y].astype(int)]).clip(0).sum() >= 3          # run starts
    assert set(range(14, 33)) == {y for y in range(33) if (m[y] & m[y + 1]).any()}      # 15|16 and 31|32 are the 16-row merge bands' edges


@pytest.mark.parametrize("W,H", SIZES)
def test_shapes_change_under_a_threshold_and_exact_flips(oracle, W, H):
    changed = {}
    for max_size, max_diff in THRESHOLDS(H):
        for name, img in SS.shapes(W, H, max_size, max_diff).items():
            assert img.shape == (H, W) and img.dtype == np.int16
            out = oracle.filter_speckles(img, -16, max_size, max_diff)
            changed[name] = changed.get(name, False) or not np.array_equal(out, img)
            if name in SS.FIGURES:
                sizes = _sizes(img != -16)
                assert len(sizes) <= 2 and (out != -16).sum() == sum(s for s in sizes if s > max_size)
                if len(sizes) == 2:
                    assert max_size >= sizes[1] >= 5                    # the small one is erased
                if max_size == 3:
                    assert sizes[0] > H and (out == img).all() == (len(sizes) == 1)     # the large one is kept (a staircase's 3 H pixels too)
            if name == "exact":
                assert _sizes(img != -16) == [max_size + 1, max_size]
                assert (out == SS.V).sum() == 0 and (out == SS.V + 16).sum() == max_size + 1
                assert (oracle.filter_speckles(img, -16, max_size - 1, max_diff) != -16).sum() == 2 * max_size + 1
            if name == "plateaus":
                assert (out != -16).sum() == 2 * max_size and (img != -16).sum() == 4 * max_size
                assert np.array_equal(np.unique(out[out != -16]), [SS.V, SS.V + max_diff])
            if name == "forks":
                n = 2 if H >= 17 else 1
                assert _sizes(img != -16) == [2 * (max_size - 1)] * n and np.array_equal(out, img)
                assert (np.abs(np.diff(img[1, :max_size - 1].astype(int))) == 2 * max_diff).all()       # the lower row: one-pixel runs
                assert (np.abs(img[1, :max_size - 1].astype(int) - img[0, :max_size - 1]) == max_diff).all()
                changed[name] = True                            # kept as it is when every union is made: that is its point
            if name == "full-lists":
                assert (img != -16).all() and (out[:-1] == -16).all() and (out[-1] != -16).all() == (W > max_size)
    assert changed and all(changed.values()), changed
    assert ("exact" in changed) == (H >= 34)
    assert set(SS.FIGURES) | {"plateaus", "full-lists", "forks"} <= set(changed)
