// v3d_temporal_math.h -- the integer arithmetic of the temporal depth stabilisation, written once (contract in include/v3d_hip.h).
// Plain C11 for host and device, no HIP header: tests/test_temporal_math_host.py compiles it with the oracle's gcc and holds it to
// tests/temporal_ref.py.  The plain and the motion-compensated window (v3d_temporal.hip, v3d_temporal_mc.hip) both compute with
// these lines and with no others.
#pragma once
#include "v3d_depth_math.h"

// a 0/1 flag as the language's own boolean (no <stdbool.h>: C and C++ spell it differently).  As an int, the filter kernel's four
// centre flags become a byte vector in VGPRs; as a boolean they stay four lane masks in SGPRs (2 to 10 VGPRs fewer on gfx950).
#ifdef __cplusplus
typedef bool v3d_flag;
#else
typedef _Bool v3d_flag;
#endif

// frames [lo, hi] that may contribute to target t: |u - t| <= R, inside [0, T), no cut in (min(t,u), max(t,u)]
V3D_HD static inline void v3d_tp_admissible(const uint8_t* cut, int T, int t, int R, int* lo, int* hi)
{
    const int a = t - R > 0 ? t - R : 0, b = t + R < T - 1 ? t + R : T - 1;
    int l = t, h = t;
    while (l - 1 >= a && !cut[l]) l--;
    while (h + 1 <= b && !cut[h + 1]) h++;
    *lo = l;
    *hi = h;
}

// cut[u] of a pair's 64-bit sum of absolute luma differences (or compensated residual): more than c levels per pixel on average
V3D_HD static inline int v3d_tp_is_cut(uint64_t sum, int c, uint64_t npx) { return sum > (uint64_t)c * npx; }

// floor(256 s / (9 tau)) = (256 s * mul) >> 32 with mul = ceil(2^32 / (9 tau)): exact for s <= 2295 because the excess
// 256 s e / (9 tau 2^32), e < 9 tau, stays below 2^20 / 2^32, far under the 1 / (9 tau) a quotient's fraction leaves.
// The high half of the 64-bit product is one instruction on the device, the one __umulhi gave (v_mad_u64_u32 on gfx950).
V3D_HD static inline uint32_t v3d_tp_rw_magic(int tau)
{
    const uint32_t d = 9u * (uint32_t)tau;
    return (uint32_t)((((uint64_t)1 << 32) + d - 1u) / d);
}
// rw = max(0, 256 - floor(256 s / (9 tau))), s the 3x3 sum of absolute luma differences (0..2295)
V3D_HD static inline uint32_t v3d_tp_range_weight(uint32_t s, uint32_t mul)
{
    const uint32_t q = (uint32_t)(((uint64_t)(s << 8) * mul) >> 32);
    return q >= 256u ? 0u : 256u - q;
}
// the weight of the tap k frames from the target: triangular in |k| <= R, times rw, 0 for an invalid depth (d16 < 1).  Written as a
// select on tw, not as `valid ? tw * rw : 0`: the compiler branches around rw in that form and the kernel then waits for its
// depth load before it starts on the weights
V3D_HD static inline uint32_t v3d_tp_weight(uint32_t s, uint32_t mul, int R, int k, int d16)
{
    const uint32_t tw = d16 >= 1 ? (uint32_t)(R + 1 - (k < 0 ? -k : k)) : 0u;
    return tw * v3d_tp_range_weight(s, mul);
}
// out16 = floor((2 Dsum + Wsum) / (2 Wsum)), Wsum = sum w, Dsum = sum w d16: the weighted mean rounded half up; 0 without weight,
// and 0 at an invalid centre unless holes are filled.  2 Dsum + Wsum < 2^31 for R <= 8 and d16 <= 32767.
V3D_HD static inline uint32_t v3d_tp_quotient(uint32_t Wsum, uint32_t Dsum, int fill, v3d_flag centre_valid)
{
    if (!Wsum || (!fill && !centre_valid)) return 0u;
    return (2u * Dsum + Wsum) / (2u * Wsum);
}
