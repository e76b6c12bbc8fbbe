// Test-only entries of tests/test_sgbm_post_emulated.py and tests/test_speckle_emulated.py (sgbm_post_entries.cpp), next to the two
// public entries of csrc/v3d_sgbm_post.hip and, for tests/test_blend_emulated.py, those of csrc/v3d_blend.hip
#pragma once
#include <stdint.h>
#include "v3d_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
// sgbm_lrcheck_median on a handle with these fields: n frames of WTA records [H][W] -> int16 [H][W]
int emu_sgbm_lrcheck_median(const uint32_t* wta, int n, int W, int H, int d12, int min_disparity, int lrm_tiles, int med, int16_t* out, void* stream);
// sgbm_speckles on a handle with these fields: n frames in place; labels = 3 * W * H * n int32
int emu_sgbm_speckles(int16_t* out, int n, int W, int H, int min_disparity, int speckle_window, int speckle_range, int32_t* labels, void* stream);
#ifdef __cplusplus
}
#endif
