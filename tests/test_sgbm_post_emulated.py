"""The L-R check + 3x3 median of csrc/v3d_sgbm_post.hip itself, without a GPU: sgbm_lrcheck_median (what run_sgbm calls) runs in the
stand-alone emulator driver (tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, on WTA records fed
in directly (tests/sgbm_post_ref.py states their domain) and must equal that reference bit for bit, with the median and without
it (the debug_raw export).  Every route: the row march with 4 and with 8 pixel pairs per thread, and the 128 x 16 tiles for odd
widths, widths above 4096, the lrm_tiles switch, a record plane 4 bytes off an 8-byte boundary and an output plane 2 bytes off a
4-byte boundary (the sanitized build reports a misaligned 8- or 4-byte access if the row march were taken there).  Both planes end
on their heap block's last byte; the never-written record columns [0, 64) carry the run's poison."""
import numpy as np
import pytest

import emu_case as E
import sgbm_post_emu as X
import sgbm_post_ref as P

driver = X.fixture()
MS = [0, -1, -2, -31, -32, -63, -64]
ROWS, TILES = 0, 1
# (W, H, m, frames, lrm_tiles, skew of the records, skew of the output) -> route.  Every W, H and m of each route appears; the
# smallest W with the smallest H, the largest with a band edge (the march's bands are 15 rows, the tiles 16)
MARCH4 = ([(70, 1, 0, 1), (70, 2, -31, 1), (130, 15, 0, 1), (130, 16, -1, 2), (512, 31, -31, 1), (514, 16, 0, 1), (514, 2, -31, 1),
           (2048, 31, 0, 1), (2048, 15, -31, 1)] + [(130, 16, m, 1) for m in MS if m != -1])
MARCH8 = [(2050, 1, 0, 1), (2050, 16, -31, 2), (4096, 16, 0, 1), (4096, 1, -31, 1)]
TILED = ([(69, 1, 0, 1), (127, 15, -31, 1), (129, 17, -1, 2), (257, 33, 0, 1), (257, 16, -31, 1), (4098, 16, 0, 1), (4098, 33, -31, 1)] +
         [(129, 17, m, 1) for m in MS if m != -1])
CASES = ([c + (0, 0, 0, ROWS) for c in MARCH4 + MARCH8] + [c + (0, 0, 0, TILES) for c in TILED] +
         [(130, 16, 0, 1, 1, 0, 0, TILES), (512, 17, -31, 1, 1, 0, 0, TILES), (2048, 16, -31, 1, 1, 0, 0, TILES),   # the switch, even widths
          (130, 16, -31, 1, 0, 4, 0, TILES), (514, 15, 0, 2, 0, 4, 0, TILES),                                      # records off an 8-byte boundary
          (130, 16, -2, 1, 0, 0, 2, TILES), (70, 1, -63, 1, 0, 0, 2, TILES)])                                      # output off a 4-byte boundary
RAW = [(70, 1, 0, 1, 0, 0, 0, ROWS), (130, 16, 0, 1, 0, 0, 0, ROWS), (130, 16, -1, 2, 0, 0, 0, ROWS), (130, 16, -64, 1, 0, 0, 0, ROWS),
       (2048, 16, -31, 1, 0, 0, 0, ROWS), (4096, 1, -32, 1, 0, 0, 0, ROWS), (69, 1, 0, 1, 0, 0, 0, TILES), (129, 17, -1, 2, 0, 0, 0, TILES),
       (129, 17, -63, 1, 0, 0, 0, TILES), (4098, 17, 0, 1, 0, 0, 0, TILES), (130, 16, -31, 1, 0, 4, 2, TILES)]
FLAVOURS = [{}, {"few_costs": True}, {"best63_at_64": True}, {"subpix_extremes": True, "few_costs": True}, {"empty_rows": (0,)},
            {"best63_at_64": True, "reject": 0.5}]


def _route(W, tiles, skew_rec, skew_out):
    """the dispatch of sgbm_lrcheck_median, restated: which cases take which route is part of what is tested"""
    return TILES if (tiles or W > 4096 or W & 1 or skew_rec & 7 or skew_out & 3) else ROWS


def _ids(cases):
    return [f"{W}x{H}m{m}n{n}" + ("-tiles" if t else "") + (f"-rec{sr}" if sr else "") + (f"-out{so}" if so else "") for W, H, m, n, t, sr, so, _ in cases]


def _case(driver, tmp_path, case, med):
    W, H, m, n, tiles, skew_rec, skew_out, route = case
    assert _route(W, tiles, skew_rec, skew_out) == route
    rng = np.random.default_rng(W * 1000 + H * 10 - m)
    flavour = FLAVOURS[(W + H - m) % len(FLAVOURS)]
    d12 = (1, 1, 0, 2)[(W + H) % 4]
    rec = np.stack([P.random_records(rng, W, H, **flavour) for _ in range(n)])
    if H > 4 and "empty_rows" not in flavour:
        rec[-1, H // 2] = 0                                     # a row without any record inside the plane
    want = np.stack([(P.lrcheck_median if med else P.lrcheck)(r, d12, m) for r in rec])
    assert n * H * (W - 64) < 200 or len(np.unique(want)) > 3

    def make(gp):
        dirty = rec.copy()
        dirty[:, :, :64] = gp * 0x01010101                      # never written: the allocation's garbage
        return [E.exact("wta", dirty.view(np.uint8), skew_rec), n, W, H, d12, m, tiles, int(med),
                E.exact("out", np.full(2 * want.size, gp, np.uint8), skew_out, expect=want.view(np.uint8).reshape(-1)), 0]
    E.run_configs(driver, tmp_path, X.LRCHECK, make)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_lrcheck_and_median(driver, tmp_path, case):
    _case(driver, tmp_path, case, True)


@pytest.mark.parametrize("case", RAW, ids=_ids(RAW))
def test_lrcheck_without_the_median(driver, tmp_path, case):
    _case(driver, tmp_path, case, False)


def test_the_cases_cover_what_they_claim():
    for route, Ws, Hs in ((ROWS, {70, 130, 512, 514, 2048, 2050, 4096}, {1, 2, 15, 16, 31}), (TILES, {69, 127, 129, 257, 4098}, {1, 15, 16, 17, 33})):
        mine = [c for c in CASES if c[7] == route]
        assert Ws <= {c[0] for c in mine} and Hs <= {c[1] for c in mine} and {0, -31} <= {c[2] for c in mine}
        assert any(c[3] == 2 for c in mine)
    for W, H in ((130, 16), (129, 17)):
        assert set(MS) <= {c[2] for c in CASES if c[:2] == (W, H) and not c[4] and not c[5] and not c[6]}
    assert {(2050, 1), (2050, 16), (4096, 1), (4096, 16)} <= {c[:2] for c in CASES}
