"""Inputs and arithmetic for the tests at the edges of the SGBM matcher's accepted domain
(test_sgbm_domain_host.py pins them against the oracle on the CPU, test_sgbm_domain_gpu.py runs the kernels on them)."""
import numpy as np

D = 64                       # numDisparities of this build
FTZEROS = (15, 17, 21, 31)   # ftzero = max(preFilterCap, 15) | 1 of the preFilterCap values 0, 16, 20, 31
CAP_OF_FTZERO = {15: 0, 17: 16, 21: 20, 31: 31}
CAPS = [0, 16, 20, 31]
# frame sizes of the GPU headroom tests, per preFilterCap: 64 + 70 .. 64 + 260 columns (at least two 64-column k_vdd strips,
# two 128-column ones from 64 + 129 on), 40 .. 90 rows, none a multiple of a tile
HEADROOM_SIZES = {0: (64 + 136, 60), 16: (64 + 260, 41), 20: (64 + 70, 90), 31: (64 + 200, 47)}


def ftzero_of(pre_filter_cap):
    return max(pre_filter_cap, 15) | 1


def cost_ceiling(ftzero):
    """largest 5 x 5 box sum of pixel costs: the gradient plane gives at most 2 * ftzero, the raw plane 255 >> 2 = 63"""
    return 25 * (2 * ftzero + 63)


def accepted(P2, pre_filter_cap):
    """the headroom rule of the packed int16 recurrence, restated: delta = min L + P2 <= C_max = 2 * P2 + ceiling must stay
    below 32767, and the pre-filter bytes must add pairwise without carry"""
    ft = ftzero_of(pre_filter_cap)
    return ft <= 31 and 2 * P2 + cost_ceiling(ft) < 32767


def p2max(ftzero):
    """largest accepted P2, solved from the rule: 2 * P2 <= 32766 - ceiling"""
    return (32766 - cost_ceiling(ftzero)) // 2


def ceiling_pair(W, H, ftzero):
    """content that drives the box sum to its ceiling: saw-tooth ramps, constant over bands of 7 rows (so that rows 2..4 of a
    band see a uniform 5 x 5 window).  The left view rises to 255 and the right view falls to 0 at a slope that saturates
    the x-Sobel at +-ftzero (8 * slope >= ftzero), so the gradient planes sit at 2 * ftzero and 0 and the raw planes near
    255 and 0.  The period changes from band to band: the teeth of the two views then meet at other disparities."""
    slope = (ftzero + 7) // 8                                  # 2, 3, 3, 4 for ftzero 15, 17, 21, 31
    x = np.arange(W)[None, :]
    band = (np.arange(H) // 7)[:, None]
    period = 16 + 4 * (band % 5)                               # 16, 20, .. 32 columns
    t = period - 1 - (x + 3 * band + 8) % period               # period-1 .. 0 along a tooth; column 64 starts mid-tooth
    left = 255 - slope * t
    right = slope * t
    return np.ascontiguousarray(left.astype(np.uint8)), np.ascontiguousarray(right.astype(np.uint8))


def binary_inverse_pair(W, H, seed):
    """binary noise against its inverse: every gradient saturated, raw costs at their maximum wherever the views
    disagree; saturates S and has about half the pixels rejected"""
    rng = np.random.default_rng(seed)
    left = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
    return left, (255 - left).astype(np.uint8)


def noise_pair(W, H, seed):
    """unrelated uniform noise: components of every size survive the L-R check"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)


def same_view_noise(W, H, seed):
    """left == right: min S == 0 at d = 0 on every pixel, S > 0 at the far disparities"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    return left, left.copy()


def patchy_pair(W, H, seed, block=12, share=0.4):
    """a textured pair whose right view has `share` of its block x block patches replaced by noise: matched regions next to
    unmatched ones, so that the uniqueness test, the L-R check and the speckle filter all decide pixels"""
    from conftest import textured_pair
    left, right = textured_pair(W, H, seed)
    rng = np.random.default_rng(seed + 1000)
    m = rng.random((-(-H // block), -(-W // block))) < share
    m = np.repeat(np.repeat(m, block, axis=0), block, axis=1)[:H, :W]
    return left, np.where(m, rng.integers(0, 256, (H, W)), right).astype(np.uint8)


def speckle_pairs():
    """the pairs of the speckle-parameter tests: components of every size after the L-R check"""
    return noise_pair(64 + 200, 50, 9), patchy_pair(64 + 136, 60, 17)
