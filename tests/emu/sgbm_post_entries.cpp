// Test-only entries (sgbm_post_entries.h): a v3d_sgbm on the stack with the fields the post stage reads, handed to the two functions
// run_sgbm calls.  Nothing here is part of the product.
#include "v3d_sgbm_internal.h"
#include "sgbm_post_entries.h"

extern "C" int emu_sgbm_lrcheck_median(const uint32_t* wta, int n, int W, int H, int d12, int min_disparity, int lrm_tiles, int med, int16_t* out, void* stream)
{
    v3d_sgbm h{};
    h.wta = const_cast<uint32_t*>(wta); h.d12 = d12; h.prm.minDisparity = min_disparity; h.lrm_tiles = lrm_tiles;
    return sgbm_lrcheck_median(&h, n, W, H, out, med != 0, (hipStream_t)stream);
}

extern "C" int emu_sgbm_speckles(int16_t* out, int n, int W, int H, int min_disparity, int speckle_window, int speckle_range, int32_t* labels, void* stream)
{
    v3d_sgbm h{};
    h.prm.minDisparity = min_disparity; h.prm.speckleWindowSize = speckle_window; h.prm.speckleRange = speckle_range; h.labels = labels;
    return sgbm_speckles(&h, out, n, W, H, (hipStream_t)stream);
}
