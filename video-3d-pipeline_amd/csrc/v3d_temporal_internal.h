// v3d_temporal_internal.h -- what v3d_temporal_mc.hip takes from v3d_temporal.hip: the launches of the two kernels that turn
// per-pair 64-bit sums into cut flags.  v3d_temporal_cuts fills the sums with luma differences, v3d_temporal_motion with the
// compensated residual; zeroing them and comparing them are the same kernels for both.
#pragma once
#include "v3d_common.h"
#include "v3d_temporal_math.h"

void v3d_tp_launch_zero(unsigned long long* sums, int T, hipStream_t st);
// cut[u] = u >= 1 && v3d_tp_is_cut(sums[u], c, npx) for u in [0, T)
void v3d_tp_launch_cutflag(const unsigned long long* sums, int T, int c, size_t npx, uint8_t* cut, hipStream_t st);
