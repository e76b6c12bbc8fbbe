"""The one emulator driver of csrc/v3d_sgbm_post.hip, shared by tests/test_sgbm_post_emulated.py and tests/test_speckle_emulated.py
(one build per pytest process): the source's two public entries and the test-only entries of tests/emu/sgbm_post_entries.cpp"""
import os

import emu_case as E

LRCHECK, SPECKLES, FILTER, MEDIAN = "emu_sgbm_lrcheck_median", "emu_sgbm_speckles", "v3d_filter_speckles", "v3d_median3x3_i16"


def fixture():
    return E.driver_fixture("sgbm_post", ["v3d_sgbm_post.hip"], [LRCHECK, SPECKLES, FILTER, MEDIAN], header="sgbm_post_entries.h",
                            extra=[os.path.join(E.EMU, "sgbm_post_entries.cpp")])
