"""The benchmarked configuration itself, frame by frame: bench.HotPath at bench.py's default batch (what ONE co-resident
lock-step k_vdd launch holds at 1080p, `vdd_frames_per_launch_dpl8`), every frame of the step against the float64 oracle,
and the launch splits the product uses (batch 8, one frame more than a launch, two full launches).

The batch holds B + 1 DISTINCT frames (bench cycles 8), with content extremes at positions 0, B // 2 and B - 1, so a wrong
frame stride or tile order that hits every frame of one index mod 8 cannot hide behind a repeat."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bench
from conftest import mismatch_report
from test_guided_gpu import RTOL, _rel_err

pytestmark = pytest.mark.gpu

W, H, SCALE, GF_R, GF_EPS = bench.W, bench.H, bench.SCALE, bench.GF_R, bench.GF_EPS
SEED0 = 900                     # synthetic frame indices bench.py never draws (it takes rank * 8 + i, i < 8)
SHIFT = 48                      # right-eye shift of the "past numDisparities" frame, in SBS half-width columns (96 > 64 px)


def _bench_batch(native):
    """the batch bench.main() derives when --batch is 0"""
    probe = native.StereoSGBM(W, H, 1)
    try:
        return probe.get_option("vdd_frames_per_launch_dpl8")
    finally:
        probe.close()


def _frame(kind, seed):
    """(sbs [H, W, 3] u8, guide [SCALE H, SCALE W] u8) of one batch position"""
    from video_3d_pipeline import synthetic as syn
    if kind == "black":              # no texture: disparity 0 or -16 everywhere (both invalid to depth.py:374), 4K depth exactly 0
        return np.zeros((H, W, 3), np.uint8), np.zeros((SCALE * H, SCALE * W), np.uint8)
    sbs, guide = syn.sbs_frame(W, H, seed).copy(), syn.guide_frame(W, H, seed, SCALE)
    left = sbs[:, :W // 2]
    if kind == "same":               # both eyes identical: disparity 0 wherever the match is unique
        sbs[:, W // 2:] = left
    elif kind == "far":              # right eye = left eye shifted by 2 * SHIFT px: no match inside numDisparities
        sbs[:, W // 2:] = np.roll(left, -SHIFT, axis=1)
    return np.ascontiguousarray(sbs), guide


class Frames:
    """B + 1 distinct frames, their oracle gray pair, disparity and float64 4K depth"""

    def __init__(self, native, oracle):
        self.B = B = _bench_batch(native)
        assert B >= 2, f"bench batch B = {B}: the lock-step bound of this device is too small to test"
        self.kinds = ["tex"] * (B + 1)
        for pos, kind in ((0, "black"), (B // 2, "same"), (B - 1, "far")):
            self.kinds[pos] = kind
        nthr = max(1, min(16, len(os.sched_getaffinity(0))))
        gate = threading.Semaphore(8)            # one guided oracle call holds ~530 MB

        def one(i):
            sbs, guide = _frame(self.kinds[i], SEED0 + i)
            lg, rg = oracle.sbs_to_gray(sbs, True)
            disp = oracle.sgbm_compute(lg, rg)    # ctypes releases the GIL inside liboracle.so
            with gate:
                q = oracle.guided_upscale(oracle.disp_to_depth(disp), guide, GF_R, GF_EPS)
            return sbs, guide, lg, rg, disp, q

        with ThreadPoolExecutor(nthr) as ex:
            rows = list(ex.map(one, range(B + 1)))
        self.sbs, self.guide, self.lg, self.rg, self.disp, self.q = (list(c) for c in zip(*rows))


@pytest.fixture(scope="module")
def frames(native, oracle):
    return Frames(native, oracle)


def test_content_extremes_are_what_they_claim(frames):
    """the oracle's view of the three extremes: the black frame has no positive disparity and a 4K depth of exactly 0 (so the
    1e-3 bound below demands an exact 0 of the GPU), the identical eyes match at disparity 0, the far-shifted eyes leave a large
    part invalid; the textured frames are mostly valid"""
    B, k = frames.B, frames.kinds
    black, same, far = k.index("black"), k.index("same"), k.index("far")
    assert (black, same, far) == (0, B // 2, B - 1)
    assert (frames.disp[black] <= 0).all() and not frames.q[black].any()
    assert (frames.disp[same][:, 64:] == 0).mean() > 0.9
    assert (frames.disp[far] < 0).mean() > 0.3
    assert all((frames.disp[i] > 0).mean() > 0.5 for i in range(B + 1) if k[i] == "tex")


def _check_q(got, frames, i, stage):
    err = _rel_err(got.astype(np.float64), frames.q[i])
    assert err.max() <= RTOL, (f"B = {frames.B}, frame {i} ({frames.kinds[i]}), {stage}: max rel err {err.max():.3e} "
                               f"at {np.unravel_index(err.argmax(), err.shape)}")


def test_hot_path_at_the_bench_batch(native, frames):
    """one hp.step() of bench.py's timed region on frames 0 .. B-1: gray pair and disparity bit-exact, 4K depth within 1e-3 of
    the f64 oracle for EVERY frame, and the same bits as the float32-depth route and the int16 route with the f64 first stage"""
    import torch
    B = frames.B
    dev = torch.device("cuda", torch.cuda.current_device())
    sbs = torch.from_numpy(np.stack(frames.sbs[:B])).to(dev)
    guides = torch.from_numpy(np.stack(frames.guide[:B])).to(dev)
    hp = bench.HotPath(native, dev, B, 0)
    try:
        hp.step(sbs, guides)
        assert hp.matcher.sync_errors() == 0, f"B = {B}: lock-step time-outs"
        for i in range(B):
            for name, got, want in (("left gray", hp.lg[i], frames.lg[i]), ("right gray", hp.rg[i], frames.rg[i]),
                                    ("disparity", hp.disp[i], frames.disp[i])):
                g = got.cpu().numpy()
                assert np.array_equal(g, want), f"B = {B}, frame {i} ({frames.kinds[i]}), {name}: " + mismatch_report(g, want, name)
            _check_q(hp.out4k[i].cpu().numpy(), frames, i, "4K depth")
        via_f32 = native.guided_upscale_batch(native.disp_to_depth(hp.disp[:B]), guides, GF_R, GF_EPS)
        for i in range(B):
            assert torch.equal(hp.out4k[i], via_f32[i]), (f"B = {B}, frame {i}: the int16 route differs from the float32-depth route "
                                                          f"in {int((hp.out4k[i] != via_f32[i]).sum())} px")
        del via_f32
        try:
            native.set_option("gf_int1", 0)
            via_f64 = native.guided_upscale_batch(hp.disp[:B], guides, GF_R, GF_EPS)
        finally:
            native.set_option("gf_int1", 1)
        for i in range(B):
            assert torch.equal(hp.out4k[i], via_f64[i]), (f"B = {B}, frame {i}: the integer first stage differs from the f64 one "
                                                          f"in {int((hp.out4k[i] != via_f64[i]).sum())} px")
        del via_f64
        assert hp.matcher.sync_errors() == 0
    finally:
        hp.matcher.close()
        del hp
        torch.cuda.empty_cache()


@pytest.mark.parametrize("split", ["batch8", "one_more_than_a_launch", "two_full_launches"])
def test_sgbm_launch_splits(native, frames, split):
    """the batch splits of the product: 8 frames (one launch, 4 disparities per lane when 8 fit one such launch), B + 1 (two
    launches of unequal size, the second at a frame offset), 2B (two full launches; frames B .. 2B-1 repeat the contents
    B, B-1, .., 1, a period that matches neither launch).  Every frame equals the oracle's bits."""
    import torch
    B = frames.B
    n = {"batch8": 8, "one_more_than_a_launch": B + 1, "two_full_launches": 2 * B}[split]
    if n == 8:                       # the three extremes among ordinary frames
        order = [0, 1, 2, 3, B // 2, 5, 6, B - 1]
    elif n == B + 1:
        order = list(range(n))
    else:
        order = list(range(B)) + [B - k for k in range(B)]
    assert len(order) == n and max(order) <= B
    m = native.StereoSGBM(W, H, n)
    try:
        mf4, mf8 = m.get_option("vdd_frames_per_launch_dpl4"), m.get_option("vdd_frames_per_launch_dpl8")
        mf = mf4 if n <= mf4 else mf8
        mapping = f"{4 if n <= mf4 else 8} disparities per lane, {-(-n // mf)} launch(es) (dpl4 bound {mf4}, dpl8 bound {mf8})"
        assert mf8 == B, f"a {n}-frame handle sizes launches for {mf8} frames, the bench batch is {B}"
        if split != "batch8":
            assert n > mf4 and -(-n // mf8) == 2, f"B = {B}, n = {n}: {mapping}"
        lg = torch.from_numpy(np.stack([frames.lg[j] for j in order])).cuda()
        rg = torch.from_numpy(np.stack([frames.rg[j] for j in order])).cuda()
        got = m.compute(lg, rg)
        assert m.sync_errors() == 0, f"B = {B}, n = {n} ({mapping}): lock-step time-outs"
        for i, j in enumerate(order):
            g = got[i].cpu().numpy()
            assert np.array_equal(g, frames.disp[j]), (f"B = {B}, n = {n} ({mapping}), frame {i} (content {j}, {frames.kinds[j]}): "
                                                       + mismatch_report(g, frames.disp[j], "disp16"))
        del got, lg, rg
    finally:
        m.close()
        torch.cuda.empty_cache()
