"""GPU cases of the fused guided filter's four-row steps and runs of four outputs per lane (v3d_guided.hip, k_gff): runs that
straddle a strip's last output column or the image's right edge, bands that end partway through a four-row step, r = 4 and
r = 8, both strip widths.  Each case meets the float64 oracle at 1e-3 relative, and the int16 route (exact-integer stage 1)
equals the float32 route (f64 stage 1) bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-3


def _rel_err(got, want):
    scale = np.maximum(np.abs(want), 1e-6 * max(float(np.abs(want).max()), 1e-30))
    return np.abs(got - want) / scale


# widths: 224 / 240 outputs per 256-column strip (r = 8 / 4) and 480 / 496 per 512-column strip, so W = k * NOUT +- 1..3 ends a
# run partway; heights: band 37, 38, 39 and H = 4k + 1..3 end a band and the frame partway through a four-row step
@pytest.mark.parametrize("cols", [256, 512])
@pytest.mark.parametrize("Wg,Hg,r,band", [(226, 74, 8, 37), (450, 91, 8, 38), (482, 58, 8, 39), (242, 45, 4, 37), (478, 66, 4, 38),
                                          (498, 30, 4, 432), (962, 70, 8, 432), (18, 22, 8, 9), (10, 14, 4, 10)])
def test_runs_and_partial_steps_meet_the_oracle_and_routes_agree(native, oracle, Wg, Hg, r, band, cols):
    import torch
    Wg, Hg = Wg + (Wg & 1), Hg + (Hg & 1)                # exact 2x of an integer low-resolution frame
    Wlo, Hlo = Wg // 2, Hg // 2
    rng = np.random.default_rng(Wg * 7 + Hg + r + cols)
    disp = rng.integers(-16, 1024, (2, Hlo, Wlo)).astype(np.int16)
    disp[rng.random(disp.shape) < 0.1] = -16
    disp[:, :, :3] = 0
    guide = rng.integers(0, 256, (2, Hg, Wg), dtype=np.uint8)
    d16, g = native.to_device(disp), native.to_device(guide)
    try:
        native.set_option("gf_band", band)
        native.set_option("gf_cols", cols)
        via_int = native.guided_upscale_batch(d16, g, r, 1e-3)                             # int16 route: integer stage 1
        via_f32 = native.guided_upscale_batch(native.disp_to_depth(d16), g, r, 1e-3)       # float route: f64 stage 1
    finally:
        native.set_option("gf_band", 432)
        native.set_option("gf_cols", 256)
    assert torch.equal(via_int, via_f32)
    for i in range(2):
        want = oracle.guided_upscale(oracle.disp_to_depth(disp[i]), guide[i], r, 1e-3)
        assert _rel_err(via_int[i].cpu().numpy().astype(np.float64), want).max() <= RTOL


@pytest.mark.parametrize("Wg,Hg,r", [(227, 75, 8), (243, 43, 4)])
def test_odd_sizes_float_route_meets_the_oracle(native, oracle, Wg, Hg, r):
    """odd widths (scalar stores at the right edge) and a non-integer scale: the f64 stage 1 with its float bilinear weights"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(Wg + Hg)
    depth = gaussian_filter(rng.uniform(0, 63, (Hg // 3 + 1, Wg // 3 + 1)), 2.0).astype(np.float32)
    depth[rng.random(depth.shape) < 0.05] = 0.0
    guide = rng.integers(0, 256, (Hg, Wg), dtype=np.uint8)
    try:
        native.set_option("gf_band", 37)
        got = native.guided_upscale(native.to_device(depth), native.to_device(guide), r, 1e-3).cpu().numpy().astype(np.float64)
    finally:
        native.set_option("gf_band", 432)
    want = oracle.guided_upscale(depth, guide, r, 1e-3)
    assert _rel_err(got, want).max() <= RTOL
