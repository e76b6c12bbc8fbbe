// v3d_wave.h -- the cross-lane plumbing of the stages around the matcher, written once ("Wave primitives"):
// butterflies over a wavefront, workgroup sums and scans through LDS, the two-sided nearest-neighbour scan, the byte-wise row
// loaders.  All integer operations: no bit of a result depends on how they are scheduled.  Wavefronts have 64 lanes; every
// function is called by all threads of the workgroup (the butterflies, near2_incl and near2_excl: by all lanes of the wave), with
// lane = tid & 63 and wave = tid >> 6 passed in by the kernel, which has them already.  Arguments and results travel by value.
#pragma once
#include "v3d_common.h"

// ---- butterflies: every lane gets the result over the wave's 64 lanes ----
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)       // two 32-bit halves per step
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, s), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), s);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, s);
        v = o < v ? o : v;
    }
    return v;
}

// ---- workgroup sum of F fields.  t[k]: the wave's total of field k, valid in lane 0 at least (a butterfly's result, or a value
// the wave agrees on).  Returns field tid's sum over the WAVES waves in the threads tid < F, 0 in the others.  `scratch` (LDS, T
// = uint32_t or unsigned long long) is written before the one barrier inside and read after it: it is busy until the workgroup's
// next barrier after the call ----
template <int WAVES, int F, typename T>
__device__ __forceinline__ unsigned long long block_sum_u64(const T (&t)[F], int lane, int wave, int tid, T (&scratch)[WAVES][F])
{
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < F; k++) scratch[wave][k] = t[k];
    }
    __syncthreads();
    unsigned long long s = 0;
    if (tid < F) {
#pragma unroll
        for (int w = 0; w < WAVES; w++) s += scratch[w][tid];
    }
    return s;
}

// ---- workgroup exclusive add-scan: the sum of v over the threads before mine, and over all of them.  `tot` (WAVES words of LDS)
// is written before the one barrier inside and read after it: busy until the workgroup's next barrier after the call ----
struct excl_total { uint32_t excl, total; };
template <int WAVES>
__device__ __forceinline__ excl_total block_excl_add_u32(uint32_t v, int lane, int wave, uint32_t* tot)
{
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= o) inc += t; }
    if (lane == 63) tot[wave] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const uint32_t t = tot[w]; total += t; if (w < wave) base += t; }
    return { base + inc - v, total };
}

// ---- workgroup inclusive add-scan of 64-bit values: the sum of v over the threads up to and including mine, and over all of them
// (two 32-bit halves per shuffle step, as wave_sum_u64).  `tot` (WAVES double words of LDS) as above: busy until the workgroup's
// next barrier after the call ----
struct incl_total64 { unsigned long long incl, total; };
template <int WAVES>
__device__ __forceinline__ incl_total64 block_incl_add_u64(unsigned long long v, int lane, int wave, unsigned long long* tot)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)v, o), hi = __shfl_up((uint32_t)(v >> 32), o);
        if (lane >= o) v += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 63) tot[wave] = v;
    __syncthreads();
    unsigned long long base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) { const unsigned long long t = tot[w]; total += t; if (w < wave) base += t; }
    return { base + v, total };
}

// ---- two-sided nearest-neighbour scan.  Thread t holds p = a key of the last item of its run and s = a key of the first one, keys
// that grow towards the side they are looked at from; 0 means the run has none.  The result is the max of p over the threads
// before mine and the combination R of s over the threads after mine: the nearest item on either side.  R is the max (sentinel
// 0) unless the caller's right-hand keys are positions, nearest = smallest: then op_min_u32, `none_s` above every position.
// Four steps, in this order at every call site (the compiler's output is sensitive to it, and to LDS pointers as arguments):
//   n = near2_incl(p, s, lane)          inclusive shuffle scans inside the wave
//   the caller stores the wave's totals  tot_p[wave] = n.pre by lane 63, tot_s[wave] = n.suf by lane 0 (WAVES words of LDS each)
//   n = near2_excl(n, lane, none_s)     the values of the lanes before / after mine: lane 0 gets pre = 0, lane 63 suf = none_s
//   the caller's barrier, then near2_fold folds the earlier waves' tot_p and the later waves' tot_s in; .any != 0 iff any thread
//   of the workgroup has an item.  tot_p and tot_s are busy until the workgroup's next barrier after near2_fold ----
struct near2 { uint32_t pre, suf; };
struct near2_any { uint32_t pre, suf, any; };
struct op_max_u32 { static __device__ __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return max(a, b); } };
struct op_min_u32 { static __device__ __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return min(a, b); } };

template <class R = op_max_u32>
__device__ __forceinline__ near2 near2_incl(uint32_t p, uint32_t s, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t pv = __shfl_up(p, o), sv = __shfl_down(s, o);
        if (lane >= o) p = max(p, pv);
        if (lane + o < 64) s = R::f(s, sv);
    }
    return { p, s };
}
__device__ __forceinline__ near2 near2_excl(near2 n, int lane, uint32_t none_s = 0u)
{
    const uint32_t pe = __shfl_up(n.pre, 1), se = __shfl_down(n.suf, 1);
    return { lane > 0 ? pe : 0u, lane < 63 ? se : none_s };
}
template <int WAVES, class R = op_max_u32>
__device__ __forceinline__ near2_any near2_fold(near2 n, int wave, const uint32_t* tot_p, const uint32_t* tot_s)
{
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t tp = tot_p[w], ts = tot_s[w];
        any |= tp;
        if (w < wave) n.pre = max(n.pre, tp);
        if (w > wave) n.suf = R::f(n.suf, ts);
    }
    return { n.pre, n.suf, any };
}

// ---- row loaders: 16 / 8 payload bytes of a row from x0 on as little-endian words, zero beyond the row's W bytes.  VEC: base,
// pitch and strides allow one aligned load of a group that lies wholly inside the row; the partial last group, and every group
// of an unaligned plane, is read byte by byte: nothing past a row's payload is touched ----
template <bool VEC>
__device__ __forceinline__ uint4 row_load16(const uint8_t* __restrict__ row, int x0, int W)
{
    if (VEC && x0 + 16 <= W) return *reinterpret_cast<const uint4*>(row + x0);
    uint32_t v[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (x0 + i < W) v[i >> 2] |= (uint32_t)row[x0 + i] << (8 * (i & 3));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
template <bool VEC>
__device__ __forceinline__ uint2 row_load8(const uint8_t* __restrict__ row, int x0, int W)
{
    if (VEC && x0 + 8 <= W) return *reinterpret_cast<const uint2*>(row + x0);
    uint32_t v[2] = { 0u, 0u };
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (x0 + i < W) v[i >> 2] |= (uint32_t)row[x0 + i] << (8 * (i & 3));
    return make_uint2(v[0], v[1]);
}
