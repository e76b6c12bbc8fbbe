// v3d_common.h -- shared helpers for libv3d_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/v3d_hip.h"
#include "v3d_depth_math.h"   // V3D_HD, the ordered float codec, d16 and the u16 normalisations

#define V3D_D 64              // numDisparities this build is specialised for (one wavefront of d)
#define V3D_MAX_COST 32767
#define V3D_INVALID16 (-16)   // invalid in RELATIVE values (d - minDisparity) x16, what the kernels work in; the output holds (minDisparity - 1) * 16

void v3d_set_error(const char* fmt, ...);

// library-wide tuning switches (v3d_set_option / v3d_get_option); the library reads no environment variables.
// X(key = field of g_v3d_opt, default, the values `value` may take, what is stored, what it does)
// gf_band: 432 rows = 5 bands of a 4K frame: 34 frames (one lock-step launch upstream) are 5.98 rounds of the 512 resident
// workgroups, where round 2's 270 rows were 9.56 (2.56 -> 2.43 ms).  A FIXED height, not the per-launch optimum (value 0):
// the second stage's sliding sums round differently for a different band origin, and a frame's bits must not depend on how
// many frames share its launch.
#define V3D_LIB_OPTIONS(X) \
    X(gf_band1, 90, value >= 8 && value <= 65536, value, "rows per workgroup of the first guided sweep (measured best on 30 x 4K frames)") \
    X(gf_band2, 270, value >= 8 && value <= 65536, value, "rows per workgroup of the second guided sweep") \
    X(gf_tiled, 0, true, value != 0, "1: force the LDS-tiled guided kernel for every radius") \
    X(gf_fused, 1, true, value != 0, "1: single-launch guided filter (a/b rows handed from stage-1 to stage-2 waves through LDS), 0: two sweeps through HBM") \
    X(gf_band, 432, value == 0 || (value >= 8 && value <= 65536), value, "rows per workgroup of the fused kernel; 0 = per launch: fewest rounds x (band + 4r)") \
    X(gf_cols, 256, value == 256 || value == 512, value, "strip width of the fused kernel: 256 (8 waves) or 512 (16 waves, one workgroup per CU; int16 exact-2x route only)") \
    X(gf_int1, 1, true, value != 0, "1: int16 disparity + exact 2x -> stage 1 of the fused kernel in exact integers (same bits)") \
    X(corr_gather, 0, true, value != 0, "1: register-only gather-GEMM correlation (bit-identical, blends every position twice, slower)") \
    X(corr_fused, 1, true, value != 0, "1: gather-GEMM through LDS for the 1x9 pattern (warped features never touch HBM), 0: warp kernel + GEMM kernel")
struct v3d_lib_options {
#define X(name, def, ok, store, doc) int name = def;
    V3D_LIB_OPTIONS(X)
#undef X
};
extern v3d_lib_options g_v3d_opt;

#define V3D_HIP_CHECK(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            v3d_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            (void)hipGetLastError();   /* clear the sticky error so the next call starts clean */ \
            return V3D_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

#define V3D_LAUNCH_CHECK()                                                               \
    do {                                                                                 \
        hipError_t _e = hipGetLastError();                                               \
        if (_e != hipSuccess) {                                                          \
            v3d_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
            return V3D_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

static inline int v3d_cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- division-free integer arithmetic of the winner-take-all tail (plain C: host and device; tests/test_wta_arith_host.py
// restates these lines in NumPy and checks them against exact division) ----
// T1 = ceil(minS * 100 / uq) = (100 minS + uq - 1) / uq for uq = 100 - uniquenessRatio in [1, 100] and minS in [0, 32767], as
// (n * mul) >> shift with mul = ceil(2^shift / uq), shift = 23 + ceil(log2 uq).  Exact: mul * uq = 2^shift + e with
// 0 <= e < uq <= 2^(shift - 23), so n * mul / 2^shift = n / uq + n e / (uq 2^shift) and the excess n e / 2^shift < n / 2^23 < 1
// (n < 2^22) is too small to carry n / uq's fraction (at most (uq - 1) / uq) over the next integer.  n < 2^22 and
// 2^23 <= mul < 2^24 are 24-bit operands (the masks say so to the compiler): the full-rate v_mul_u32_u24 /
// v_mul_hi_u32_u24 pair, not a 32-bit multiply-high.
V3D_HD static inline void v3d_t1_magic(int uq, uint32_t* mul, int* shift)
{
    int c = 0;
    while ((1 << c) < uq) c++;
    *shift = 23 + c;
    *mul = (uint32_t)((((uint64_t)1 << *shift) + (uint64_t)uq - 1) / (uint64_t)uq);
}
V3D_HD static inline int v3d_t1_ceil(int minS, int uq, uint32_t mul, int shift)
{
    const uint32_t n = ((uint32_t)minS * 100u + (uint32_t)(uq - 1)) & 0xFFFFFFu;
    return (int)(((uint64_t)n * (mul & 0xFFFFFFu)) >> shift);
}
// sub-pixel term ((sm - sp) * 16 + den) / (den * 2), den = max(sm + sp - 2 minS, 1), truncated toward zero like the C
// expression, from a = sm - minS and b = sp - minS (both >= 0).  |a - b| <= den, so |num| <= 17 den and the quotient's
// magnitude is at most 8: four restoring steps for the bits 8, 4, 2, 1.  R carries the remainder above bit 4 and the quotient
// bits found so far below it; subtracting ((32 den - 1) << bit) takes 2 den << bit off the remainder and sets quotient bit
// `bit` in one go, and wraps to a huge unsigned number exactly when the remainder is too small, so the unsigned minimum
// keeps the right one.  R < 2^25: nothing else overflows.
V3D_HD static inline int v3d_subpix_q(int a, int b)
{
    const int den = a + b > 1 ? a + b : 1, num = (a - b) * 16 + den;
    const uint32_t step = (uint32_t)(1 - 32 * den);
    uint32_t R = (uint32_t)(num < 0 ? -num : num) << 4, t;
    t = R + (step << 3); R = t < R ? t : R;
    t = R + (step << 2); R = t < R ? t : R;
    t = R + (step << 1); R = t < R ? t : R;
    t = R + step; R = t < R ? t : R;
    const int qm = (int)(R & 15u);
    return num < 0 ? -qm : qm;
}

#ifdef __HIPCC__
// ---- packed 2 x int16 arithmetic on one VGPR (v_pk_*_i16 / _u16 on gfx950) ----
typedef short v3d_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short v3d_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v3d_s16x2 as_s(uint32_t a) { return __builtin_bit_cast(v3d_s16x2, a); }
__device__ __forceinline__ v3d_u16x2 as_us(uint32_t a) { return __builtin_bit_cast(v3d_u16x2, a); }
__device__ __forceinline__ uint32_t as_u(v3d_s16x2 a) { return __builtin_bit_cast(uint32_t, a); }
__device__ __forceinline__ uint32_t as_u(v3d_u16x2 a) { return __builtin_bit_cast(uint32_t, a); }

__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_s(a), as_s(b))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_max(as_s(a), as_s(b))); }
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) { return as_u((v3d_s16x2)(as_s(a) + as_s(b))); }
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) { return as_u((v3d_s16x2)(as_s(a) - as_s(b))); }
__device__ __forceinline__ uint32_t pk_subu(uint32_t a, uint32_t b) { return as_u((v3d_u16x2)(as_us(a) - as_us(b))); }      // wraps
__device__ __forceinline__ uint32_t pk_add_sat(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_add_sat(as_s(a), as_s(b))); }
__device__ __forceinline__ uint32_t pk_subu_sat(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_sub_sat(as_us(a), as_us(b))); }
__device__ __forceinline__ uint32_t pk_minu(uint32_t a, uint32_t b) { return as_u(__builtin_elementwise_min(as_us(a), as_us(b))); }
__device__ __forceinline__ uint32_t pk_shr_u(uint32_t a, int n) { return as_u((v3d_u16x2)(as_us(a) >> (unsigned short)n)); }
__device__ __forceinline__ uint32_t pk_bcast(int v) { return ((uint32_t)v & 0xFFFFu) * 0x00010001u; }

// ---- per-frame float min / max in a {min, max} slot of two ordered uints (v3d_f2ord): exact, so schedule-independent ----
__device__ __forceinline__ void mm_reset(unsigned* slot) { slot[0] = 0xFFFFFFFFu; slot[1] = 0u; }
// a lane's (lo, hi) folded over its wave by butterfly, then ONE atomic pair per wave.  skip_empty: a wave none of whose lanes
// saw a value (lo > hi) issues nothing
__device__ __forceinline__ void mm_wave_fold(unsigned* slot, unsigned lo, unsigned hi, bool skip_empty = false)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, s)); hi = max(hi, (unsigned)__shfl_xor((int)hi, s)); }
    if ((threadIdx.x & 63) == 0 && !(skip_empty && lo > hi)) { atomicMin(slot, lo); atomicMax(slot + 1, hi); }
}

// ({hi,lo} >> sh) & 0xffffffff  (v_alignbit_b32)
__device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }

// ---- DPP lane movement (CDNA4 is a gfx9-family ISA: row_* controls act inside 16-lane rows) ----
#define V3D_DPP_QUAD(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
#define V3D_DPP_ROW_SHL(n) (0x100 + (n))   // lane i reads lane i+n
#define V3D_DPP_ROW_SHR(n) (0x110 + (n))   // lane i reads lane i-n
#define V3D_DPP_ROW_MIRROR 0x140
#define V3D_DPP_ROW_HALF_MIRROR 0x141

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t old, uint32_t src)
{
    // lanes whose source is outside the row keep `old` (bound_ctrl = 0)
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, 0xF, 0xF, false);
}
// butterfly exchange (every lane has a valid source): bound_ctrl form, which the DPP-combine pass can fold into
// the consuming VOP2 instruction (v_min_u32_dpp ...)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_xchg(uint32_t src)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)src, CTRL, 0xF, 0xF, true);
}
// streaming accesses: once-read / once-written volume data bypasses cache retention
typedef uint32_t v3d_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t v3d_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 ld_stream(const uint4* p)
{
    const v3d_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const v3d_u32x4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint2 ld_stream(const uint2* p)
{
    const v3d_u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const v3d_u32x2*>(p));
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ void st_stream(uint4* p, uint4 v)
{
    v3d_u32x4 t = { v.x, v.y, v.z, v.w };
    __builtin_nontemporal_store(t, reinterpret_cast<v3d_u32x4*>(p));
}
__device__ __forceinline__ void st_stream(uint2* p, uint2 v)
{
    v3d_u32x2 t = { v.x, v.y };
    __builtin_nontemporal_store(t, reinterpret_cast<v3d_u32x2*>(p));
}

// ---- raw buffer access (range-checked: an offset with bit 31 set is out of range for every buffer this library
// builds, so a lane is switched off by its OFFSET, not by a branch).  Why it matters on CDNA: vmcnt counts loads
// AND stores in issue order, and once a VMEM instruction sits behind a branch the compiler's s_waitcnt model
// must assume it was not issued -- every later wait then degenerates to vmcnt(0) and a prefetch pipeline ends up
// waiting for the store it has just issued.  Unconditional instructions keep the counts exact.
#define V3D_BUF_OOB 0x80000000u
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint32_t buf_load_u32(__amdgpu_buffer_rsrc_t r, uint32_t off) { return __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0); }
__device__ __forceinline__ void buf_store_stream(__amdgpu_buffer_rsrc_t r, uint32_t off, uint4 v)
{
    v3d_u32x4 t = { v.x, v.y, v.z, v.w };
    __builtin_amdgcn_raw_buffer_store_b128(t, r, off, 0, 2);      // aux bit 1: non-temporal
}
__device__ __forceinline__ void buf_store_stream(__amdgpu_buffer_rsrc_t r, uint32_t off, uint2 v)
{
    v3d_u32x2 t = { v.x, v.y };
    __builtin_amdgcn_raw_buffer_store_b64(t, r, off, 0, 2);
}

// XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own 4 MB L2).  Map the linear
// workgroup id so that every XCD walks a CONTIGUOUS range of logical tiles: neighbouring tiles, which re-read each
// other's halo, then share an L2.  Speed only -- nothing may depend on the placement.
__device__ __forceinline__ uint32_t xcd_linear(uint32_t lin, uint32_t nb)
{
    const uint32_t x = lin & 7u, q = nb >> 3, r = nb & 7u;       // XCD x owns q (+1 if x < r) consecutive logical tiles
    return x * q + min(x, r) + (lin >> 3);
}
__device__ __forceinline__ void xcd_tile(int& bx, int& by, int& bz)
{
    const uint32_t nb = gridDim.x * gridDim.y * gridDim.z;
    const uint32_t lg = xcd_linear(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), nb);
    bx = (int)(lg % gridDim.x); by = (int)((lg / gridDim.x) % gridDim.y); bz = (int)(lg / (gridDim.x * gridDim.y));
}

#endif
