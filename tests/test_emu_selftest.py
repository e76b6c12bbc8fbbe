"""The emulator's own test (tests/emu/, tests/emu_case.py), without a GPU and without the product's kernels: six toy kernels,
each with one defect that leaves a device's output bits alone, must be rejected by the sanitized driver or by the comparison under
two poisons and two orders, and the correct twin of each must pass.  Also: a launch outside a workgroup's limits is an error, and
each cross-lane shim of the stand-in (DPP row shifts and broadcasts, ballot, readlane, readfirstlane) gives its known answer."""
import os

import numpy as np
import pytest

import emu_case as E

TOYS = ["toy_lds_overrun", "toy_global_overread", "toy_misaligned_load", "toy_lds_unwritten", "toy_missing_barrier", "toy_workgroup_order", "toy_launch"]
LANE_TOYS = ["toy_row_shr", "toy_row_bcast", "toy_wave_scan", "toy_ballot", "toy_readlane", "toy_wave_exit"]
driver = E.driver_fixture("toys", [], TOYS + LANE_TOYS, header="toys.h", extra=[os.path.join(E.EMU, "toys.cpp")])

IN32 = (np.arange(256, dtype=np.uint32) * 2654435761 + 12345).astype(np.uint32)
IN8 = (np.arange(4096 + 16) * 37 % 251).astype(np.uint8)


def _words(a):
    return np.ascontiguousarray(a, np.uint32).view(np.uint8)


def _args(toy, bad, gp):
    """the toy's arguments and what its correct twin writes"""
    out = lambda want: E.exact("out", np.full(4 * want.size, gp, np.uint8), 0, expect=_words(want))
    if toy == "toy_global_overread":
        return [E.exact("in", IN8[:256], 0), out(IN8[:256].astype(np.uint32)), bad, 0]
    if toy == "toy_misaligned_load":
        w = IN8[:4096].view(np.uint32).reshape(256, 4)
        return [E.exact("in", IN8, 0), out(w[:, 0] ^ w[:, 1] ^ w[:, 2] ^ w[:, 3]), bad, 0]
    if toy == "toy_workgroup_order":
        return [E.exact("counter", np.zeros(4, np.uint8), 0, expect=_words(np.array([4]))), out(np.arange(4, dtype=np.uint32)), bad, 0]
    want = {"toy_lds_overrun": IN32, "toy_lds_unwritten": IN32, "toy_missing_barrier": np.roll(IN32, -64)}[toy]
    return [E.exact("in", _words(IN32), 0), out(want), bad, 0]


@pytest.mark.parametrize("toy", TOYS[:6])
def test_the_correct_twin_passes(driver, tmp_path, toy):
    E.run_configs(driver, tmp_path, toy, lambda gp: _args(toy, 0, gp))


# defect -> what rejects it in the plain and in the sanitized build: a counter, the comparison, a sanitizer's report.  None: the
# output is right and nothing but a sanitizer can see the defect, which is why the sanitized build exists
DEFECTS = [("toy_lds_overrun", 1, None, "heap-buffer-overflow"), ("toy_global_overread", 1, None, "heap-buffer-overflow"),
           ("toy_misaligned_load", 1, "off their alignment", "off their alignment"),
           ("toy_misaligned_load", 2, "bytes differ", "misaligned address"),
           ("toy_lds_unwritten", 1, "bytes differ", "bytes differ"), ("toy_missing_barrier", 1, "bytes differ", "bytes differ"),
           ("toy_workgroup_order", 1, "bytes differ", "bytes differ")]


@pytest.mark.parametrize("toy,bad,plain,sanitized", DEFECTS, ids=[f"{d[0]}-{d[1]}" for d in DEFECTS])
def test_the_defect_is_rejected(driver, tmp_path, toy, bad, plain, sanitized):
    report = sanitized if os.path.dirname(driver).endswith("_san") else plain
    if report is None:
        E.run_configs(driver, tmp_path, toy, lambda gp: _args(toy, bad, gp))
        return
    with pytest.raises(AssertionError, match=report):
        E.run_configs(driver, tmp_path, toy, lambda gp: _args(toy, bad, gp))


@pytest.mark.parametrize("lds,threads,ok", [(160 * 1024, 256, True), (160 * 1024 + 16, 64, False), (0, 1024, True), (0, 1025, False), (0, 100, True)])
def test_a_launch_outside_a_workgroups_limits_is_an_error(driver, tmp_path, lds, threads, ok):
    make = lambda gp: [E.exact("out", np.zeros(4, np.uint8), 0, expect=_words(np.array([threads]))), lds, threads, 0]
    if ok:
        E.run_configs(driver, tmp_path, "toy_launch", make)
    else:
        with pytest.raises(AssertionError, match="launch outside a workgroup's range"):
            E.run_configs(driver, tmp_path, "toy_launch", make)


# ---- the cross-lane shims: lane l of wave w is thread 64 w + l; rows are 16 lanes ----
LANE = np.arange(256) % 64
WAVE0 = np.arange(256) // 64 * 64


def _lane_case(toy, arg, want, threads=256):
    def make(gp):
        out = np.full(4 * want.size, gp, np.uint8)
        return [E.exact("in", _words(IN32), 0), E.exact("out", out, 0, expect=_words(want)), arg, 0]
    return make


@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_row_shr_keeps_old_at_row_starts(driver, tmp_path, n):
    want = np.where(LANE % 16 >= n, np.roll(IN32, n), ~IN32)
    assert np.all(want[::16] == ~IN32[::16])
    E.run_configs(driver, tmp_path, "toy_row_shr", _lane_case("toy_row_shr", n, want))


@pytest.mark.parametrize("which,rows,lane", [(15, (1, 3), None), (31, (2, 3), 31), (150, (1, 2, 3), None), (310, (2, 3), 31)])
def test_row_bcast_under_a_row_mask(driver, tmp_path, which, rows, lane):
    """row_bcast:15 gives lane 15 of a row to the next row, row_bcast:31 lane 31 to rows 2 and 3; rows masked off or without a
    source keep `old`"""
    src = WAVE0 + (LANE // 16 * 16 - 1 if lane is None else lane)
    want = np.where(np.isin(LANE // 16, rows), IN32[src % 256], ~IN32)
    E.run_configs(driver, tmp_path, "toy_row_bcast", _lane_case("toy_row_bcast", which, want))


def test_another_dpp_control_is_an_emulator_error(driver, tmp_path):
    with pytest.raises(AssertionError, match="DPP control 0x140 is not emulated"):
        E.run_configs(driver, tmp_path, "toy_row_bcast", _lane_case("toy_row_bcast", 0x140, IN32))


def test_the_wave_max_scan_equals_a_plain_loop_and_its_defective_twin_does_not(driver, tmp_path):
    want = np.empty_like(IN32)
    for t in range(256):
        want[t] = IN32[t // 64 * 64:t + 1].max()
    E.run_configs(driver, tmp_path, "toy_wave_scan", _lane_case("toy_wave_scan", 0, want))
    with pytest.raises(AssertionError, match="bytes differ"):
        E.run_configs(driver, tmp_path, "toy_wave_scan", _lane_case("toy_wave_scan", 1, want))


@pytest.mark.parametrize("threads", [256, 100, 1])
def test_ballot_with_a_partial_last_wave(driver, tmp_path, threads):
    bits = (IN32[:threads] & 1).astype(np.uint64)
    want = np.zeros(2 * threads, np.uint32)
    for w in range((threads + 63) // 64):
        b = bits[64 * w:64 * w + 64]
        m = int((b << np.arange(b.size, dtype=np.uint64)).sum())
        want[2 * 64 * w:2 * (64 * w + b.size):2] = m & 0xFFFFFFFF
        want[2 * 64 * w + 1:2 * (64 * w + b.size):2] = m >> 32
    assert threads != 100 or (want[2 * 64 + 1] >> 4 == 0 and want[1] != 0)      # lanes 36 .. 63 of the last wave do not vote
    E.run_configs(driver, tmp_path, "toy_ballot", _lane_case("toy_ballot", threads, want))


def test_readlane_63_and_readfirstlane(driver, tmp_path):
    want = np.stack([IN32[WAVE0 + 63], IN32[WAVE0]], axis=1).reshape(-1)
    E.run_configs(driver, tmp_path, "toy_readlane", _lane_case("toy_readlane", 63, want))
    with pytest.raises(AssertionError, match="readlane of lane 64"):
        E.run_configs(driver, tmp_path, "toy_readlane", _lane_case("toy_readlane", 64, want))


@pytest.mark.parametrize("live", [4, 2, 1])
def test_a_wave_that_returns_before_any_rendezvous(driver, tmp_path, live):
    up = np.where(LANE > 0, np.roll(IN32, 1), IN32)
    pop = np.array([int((IN32[w:w + 64] & 1).sum()) for w in WAVE0], np.uint32)
    shr = np.where(LANE % 16 >= 1, np.roll(IN32, 1), 0)
    want = (up ^ IN32[WAVE0 + 63] ^ pop ^ shr).astype(np.uint32)

    def make(gp):
        w = _words(want).copy()
        w[4 * 64 * live:] = gp                                  # the waves that returned wrote nothing
        return [E.exact("in", _words(IN32), 0), E.exact("out", np.full(1024, gp, np.uint8), 0, expect=w), live, 0]
    E.run_configs(driver, tmp_path, "toy_wave_exit", make)
