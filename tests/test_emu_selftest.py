"""The emulator's own test (tests/emu/, tests/emu_case.py), without a GPU and without the product's kernels: six toy kernels,
each with one defect that leaves a device's output bits alone, must be rejected by the sanitized driver or by the comparison under
two poisons and two orders, and the correct twin of each must pass.  Also: a launch outside a workgroup's limits is an error."""
import os

import numpy as np
import pytest

import emu_case as E

TOYS = ["toy_lds_overrun", "toy_global_overread", "toy_misaligned_load", "toy_lds_unwritten", "toy_missing_barrier", "toy_workgroup_order", "toy_launch"]
driver = E.driver_fixture("toys", [], TOYS, header="toys.h", extra=[os.path.join(E.EMU, "toys.cpp")])

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
