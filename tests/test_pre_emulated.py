"""k_split_sbs of csrc/v3d_pre.hip (gray and BGR, single and batch), without a GPU: the kernel source runs in the stand-alone
emulator driver (tests/emu_case.py), plain and under AddressSanitizer / UndefinedBehaviorSanitizer, and must equal the oracle
byte for byte.  The frame starts 0 .. 3 bytes into its 4-byte word and ends on its heap block's last byte: the last row has no
pitch padding behind it, so the dword staging plan's over-read has to stay inside the image row as its comment promises.
Widths: 1024 plain and 1032 unsqueezed end a staging block exactly on the half row (`eye == 0 && s0 + ns <= hw`); 1076 has rows
of a multiple of 4 bytes, so the dword plan runs from an unaligned base; pitches dense, + 4 and + 5 (the byte plan)."""
import numpy as np
import pytest

import emu_case as E

ENTRIES = ["v3d_sbs_to_gray", "v3d_split_sbs", "v3d_sbs_to_gray_batch"]
driver = E.driver_fixture("pre", ["v3d_pre.hip"], ENTRIES)
WIDTHS = [64, 322, 1024, 1030, 1032, 1076, 2050]


def _frame_bytes(frames, pitch, stride, gp):
    """[n,H,W,3] -> the bytes from the first frame's first to the last frame's last payload byte"""
    n, H, W, _ = frames.shape
    img = np.full((n - 1) * stride + (H - 1) * pitch + W * 3, gp, np.uint8)
    for f in range(n):
        for y in range(H):
            img[f * stride + y * pitch:f * stride + y * pitch + W * 3] = frames[f, y].reshape(-1)
    return img


def _content(n, H, W, seed):
    sbs = np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    sbs[:, :, W // 8:W // 6] = 255                                  # hard edges overshoot under Lanczos: the saturation
    sbs[:, :, W // 6:W // 5] = 0
    return sbs


@pytest.mark.parametrize("unsqueeze", [1, 0])
@pytest.mark.parametrize("H", [1, 9])
@pytest.mark.parametrize("W", WIDTHS)
def test_split_at_every_base_offset_and_pitch(driver, tmp_path, oracle, W, H, unsqueeze):
    sbs = _content(1, H, W, W * 3 + H)
    want = {True: oracle.sbs_to_gray(sbs[0], bool(unsqueeze)), False: oracle.split_sbs(sbs[0], bool(unsqueeze))}
    for i, (off, pad) in enumerate((o, p) for o in range(4) for p in (0, 4, 5)):
        gray = (i + H) % 2 == 0                                     # both entries meet every offset and both staging plans
        wl, wr = want[gray]
        pitch = W * 3 + pad

        def make(gp):
            out = lambda name, w, skew: E.exact(name, np.full(w.size, gp, np.uint8), skew, expect=w.reshape(-1))
            return [E.exact("sbs", _frame_bytes(sbs, pitch, 0, gp), off), W, H, pitch, unsqueeze, out("left", wl, 1), out("right", wr, 3), 0]
        E.run_configs(driver, tmp_path, ENTRIES[0] if gray else ENTRIES[1], make)


@pytest.mark.parametrize("unsqueeze", [1, 0])
@pytest.mark.parametrize("W,off,pad,spad", [(66, 0, 0, 0), (1076, 3, 4, 8), (1030, 2, 5, 7)])
def test_gray_batch(driver, tmp_path, oracle, W, off, pad, spad, unsqueeze):
    n, H = 3, 9
    sbs = _content(n, H, W, W + 1)
    both = [oracle.sbs_to_gray(sbs[f], bool(unsqueeze)) for f in range(n)]
    wl, wr = np.stack([b[0] for b in both]), np.stack([b[1] for b in both])
    pitch = W * 3 + pad
    stride = H * pitch + spad

    def make(gp):
        out = lambda name, w, skew: E.exact(name, np.full(w.size, gp, np.uint8), skew, expect=w.reshape(-1))
        return [E.exact("sbs", _frame_bytes(sbs, pitch, stride, gp), off), n, W, H, pitch, stride, unsqueeze, out("left", wl, 2), out("right", wr, 5), 0]
    E.run_configs(driver, tmp_path, ENTRIES[2], make)
