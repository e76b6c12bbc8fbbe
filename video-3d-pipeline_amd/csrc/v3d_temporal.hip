// v3d_temporal.hip -- temporal depth stabilisation between sbs_to_disparity and the u16 normalisation (DESIGN.md section 4,
// "Temporal stabilisation"; contract in include/v3d_hip.h, NumPy restatement in tests/temporal_ref.py).  Per target frame t
// and pixel p, over the frames u = t+k of the window that no scene cut separates from t:
//   d16_u = rint(16 D_u)  (valid iff >= 1)          s_k = 3x3 edge-replicated sum of |Y_u - Y_t|  (0..2295)
//   w_k = (R + 1 - |k|) * max(0, 256 - floor(256 s_k / (9 tau))) * valid      out16 = floor((2 sum w d16 + sum w) / (2 sum w))
// All integers, so the bits do not depend on any order of evaluation; 2 Dsum + Wsum < 2^31 for R <= 8 and d16 <= 32767.
// Cut flags and the clip-stable ranges are produced and consumed on the device: no entry synchronises.  This file holds the cuts,
// the window range and the filter; the per-frame min/max they take (v3d_depth_minmax_batch) and the u16 samples against the
// window range (v3d_depth_to_u16_range_batch) live in v3d_range.hip, d16 in v3d_depth_math.h.
#include "v3d_common.h"

#define TP_MAX_R 8

// frames [lo, hi] that may contribute to target t: |u - t| <= R, inside [0, T), no cut in (min(t,u), max(t,u)]
__device__ __forceinline__ void tp_admissible(const uint8_t* __restrict__ cut, int T, int t, int R, int& lo, int& hi)
{
    lo = hi = t;
    const int a = max(0, t - R), b = min(T - 1, t + R);
    while (lo - 1 >= a && !cut[lo]) lo--;
    while (hi + 1 <= b && !cut[hi + 1]) hi++;
}

// ---- scene cuts: per-pair sum of absolute luma differences (64-bit integer, one atomic per workgroup), then the compare ----
__global__ void k_tp_zero(unsigned long long* s, int n)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s[i] = 0ull;
}
__global__ __launch_bounds__(256) void k_tp_sad(const uint8_t* __restrict__ gray, size_t stride, size_t npx, int vec,
                                                unsigned long long* __restrict__ sums)
{
    const int u = blockIdx.y + 1;
    const uint8_t* a = gray + (size_t)u * stride;
    const uint8_t* b = a - stride;
    unsigned long long acc = 0;
    const size_t nvec = vec ? npx / 16 : 0;                       // 16 px per lane and step: four v_sad_u8 on one 16-byte load each
    const uint4* a4 = reinterpret_cast<const uint4*>(a);
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) {
        const uint4 p = a4[i], q = b4[i];
        unsigned s = __builtin_amdgcn_sad_u8(p.x, q.x, 0u);
        s = __builtin_amdgcn_sad_u8(p.y, q.y, s);
        s = __builtin_amdgcn_sad_u8(p.z, q.z, s);
        s = __builtin_amdgcn_sad_u8(p.w, q.w, s);
        acc += s;
    }
    for (size_t i = nvec * 16 + (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        const int d = (int)a[i] - (int)b[i];
        acc += (unsigned)(d < 0 ? -d : d);
    }
    unsigned lo = (unsigned)acc, hi = (unsigned)(acc >> 32);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = ((unsigned long long)(unsigned)__shfl_xor((int)hi, s) << 32) | (unsigned)__shfl_xor((int)lo, s);
        acc += o;
        lo = (unsigned)acc; hi = (unsigned)(acc >> 32);
    }
    __shared__ unsigned long long part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + u, part[0] + part[1] + part[2] + part[3]);
}
__global__ void k_tp_cutflag(const unsigned long long* __restrict__ sums, int T, unsigned long long thresh, uint8_t* __restrict__ cut)
{
    for (int u = blockIdx.x * 256 + threadIdx.x; u < T; u += gridDim.x * 256) cut[u] = (u >= 1 && sums[u] > thresh) ? 1 : 0;
}

extern "C" int v3d_temporal_cuts(const uint8_t* gray, size_t gray_stride, int T, int W, int H, int c, void* ws, uint8_t* cut_out,
                                 void* stream)
{
    if (!gray || !ws || !cut_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (T < 1 || T > 65535 || W < 1 || H < 1) { v3d_set_error("bad geometry T=%d %dx%d", T, W, H); return V3D_ERR_ARG; }
    if (c < 0 || c > 256) { v3d_set_error("cut threshold %d outside [0, 256]", c); return V3D_ERR_ARG; }
    const size_t npx = (size_t)W * H;
    if (T > 1 && gray_stride < npx) { v3d_set_error("gray stride %zu below the frame size %zu", gray_stride, npx); return V3D_ERR_ARG; }
    if (((uintptr_t)ws & 7) != 0) { v3d_set_error("workspace must be 8-byte aligned"); return V3D_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(ws);
    hipLaunchKernelGGL(k_tp_zero, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, sums, T);
    if (T > 1) {
        const int vec = (((uintptr_t)gray & 15) == 0 && (gray_stride & 15) == 0) ? 1 : 0;
        const size_t want = (npx + 4095) / 4096;                             // one 16-px step per lane fills a block with 4096 px
        const size_t per = (size_t)(2048 / (T - 1) > 32 ? 2048 / (T - 1) : 32);
        const int bx = (int)(want < per ? (want ? want : 1) : per);
        hipLaunchKernelGGL(k_tp_sad, dim3(bx, T - 1), dim3(256), 0, st, gray, gray_stride, npx, vec, sums);
    }
    hipLaunchKernelGGL(k_tp_cutflag, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, sums, T, (unsigned long long)c * npx, cut_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- clip-stable range: min of the minima and max of the maxima over the admissible window ----
__global__ void k_tp_range(const float* __restrict__ mm, const uint8_t* __restrict__ cut, int T, int t0, int n, int R,
                           float* __restrict__ lohi)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        int a, b;
        tp_admissible(cut, T, t0 + j, R, a, b);
        float lo = mm[2 * a], hi = mm[2 * a + 1];
        for (int u = a + 1; u <= b; u++) {
            const float l = mm[2 * u], h = mm[2 * u + 1];
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        lohi[2 * j] = lo; lohi[2 * j + 1] = hi;
    }
}

static int tp_check_window(int T, int t0, int n, int R)
{
    if (T < 1 || T > 65535 || t0 < 0 || n < 1 || n > T - t0) { v3d_set_error("bad targets: T=%d t0=%d n=%d", T, t0, n); return V3D_ERR_ARG; }
    if (R < 0 || R > TP_MAX_R) { v3d_set_error("radius %d outside [0, %d]", R, TP_MAX_R); return V3D_ERR_ARG; }
    return V3D_OK;
}

extern "C" int v3d_temporal_range(const float* minmax, const uint8_t* cut, int T, int t0, int n, int R, float* lohi_out, void* stream)
{
    if (!minmax || !cut || !lohi_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (tp_check_window(T, t0, n, R) != V3D_OK) return V3D_ERR_ARG;
    hipLaunchKernelGGL(k_tp_range, dim3(v3d_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, minmax, cut, T, t0, n, R, lohi_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- the filter (the hot kernel) ----
// One lane owns 4 horizontally adjacent pixels of one row of one target; a 64 x 4 workgroup covers 256 x 4 px.  A gray row
// segment is the dword of the 4 pixels plus its left and right neighbours (edge-replicated) packed into 48 bits {hi, lo};
// pixel i's three horizontal neighbours are the 24-bit window (hi:lo) >> 8i, and |Y_u - Y_t| over them is one v_sad_u8
// on the masked windows (the fourth byte is zero on both sides).  Three rows accumulate into the 3x3 sum.
// floor(256 s / (9 tau)) = (256 s * mul) >> 32 with mul = ceil(2^32 / (9 tau)): exact for s <= 2295 because the excess
// 256 s e / (9 tau 2^32), e < 9 tau, stays below 2^20 / 2^32, far under the 1 / (9 tau) a quotient's fraction leaves
// (tests/test_temporal_ref.py checks every s and tau).
// VEC: W, both frame strides and all base addresses allow dword gray loads and 16-byte depth loads / stores; the other
// instantiation loads and stores element by element (odd widths, unaligned views).
template <bool VEC>
__device__ __forceinline__ void tp_gray_row(const uint8_t* __restrict__ row, int x, int W, uint32_t& lo, uint32_t& hi)
{
    uint32_t c;
    if (VEC) c = *reinterpret_cast<const uint32_t*>(row + x);
    else c = (uint32_t)row[x] | ((uint32_t)row[min(x + 1, W - 1)] << 8) | ((uint32_t)row[min(x + 2, W - 1)] << 16)
             | ((uint32_t)row[min(x + 3, W - 1)] << 24);
    const uint32_t L = row[max(x - 1, 0)], Rb = row[min(x + 4, W - 1)];
    lo = L | (c << 8);
    hi = (c >> 24) | (Rb << 8);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_tp_filter(const float* __restrict__ depth, size_t dstride, const uint8_t* __restrict__ gray,
                                                   size_t gstride, int T, int W, int H, int t0, int R, uint32_t mul, int fill,
                                                   const uint8_t* __restrict__ cut, float* __restrict__ out)
{
    const int t = t0 + blockIdx.z;
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    int ulo, uhi;
    tp_admissible(cut, T, t, R, ulo, uhi);
    const size_t r0 = (size_t)max(y - 1, 0) * W, r1 = (size_t)y * W, r2 = (size_t)min(y + 1, H - 1) * W;
    const size_t rows[3] = { r0, r1, r2 };

    uint32_t ref[3][4];
    {
        const uint8_t* g = gray + (size_t)t * gstride;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            uint32_t lo, hi;
            tp_gray_row<VEC>(g + rows[r], x, W, lo, hi);
#pragma unroll
            for (int i = 0; i < 4; i++) ref[r][i] = alignbit(hi, lo, 8 * i) & 0xFFFFFFu;
        }
    }
    uint32_t Wsum[4] = { 0, 0, 0, 0 }, Dsum[4] = { 0, 0, 0, 0 };
    bool centre[4] = { false, false, false, false };
    for (int u = ulo; u <= uhi; u++) {
        uint32_t s[4] = { 0, 0, 0, 0 };
        if (u != t) {
            const uint8_t* g = gray + (size_t)u * gstride;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                uint32_t lo, hi;
                tp_gray_row<VEC>(g + rows[r], x, W, lo, hi);
#pragma unroll
                for (int i = 0; i < 4; i++) s[i] = __builtin_amdgcn_sad_u8(alignbit(hi, lo, 8 * i) & 0xFFFFFFu, ref[r][i], s[i]);
            }
        }
        const float* dp = depth + (size_t)u * dstride + r1 + x;
        float d[4];
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(dp);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) d[i] = x + i < W ? dp[i] : 0.f;
        }
        const int k = u - t;
        const uint32_t tw = (uint32_t)(R + 1 - (k < 0 ? -k : k));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int d16 = (int)v3d_d16(d[i]);
            const bool valid = d16 >= 1;
            if (u == t) centre[i] = valid;
            const uint32_t q = __umulhi(s[i] << 8, mul);
            const uint32_t w = valid ? tw * (q >= 256u ? 0u : 256u - q) : 0u;
            Wsum[i] += w;
            Dsum[i] += w * (uint32_t)(valid ? d16 : 0);
        }
    }
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t q = Wsum[i] ? (2u * Dsum[i] + Wsum[i]) / (2u * Wsum[i]) : 0u;
        if (!fill && !centre[i]) q = 0u;
        o[i] = __fmul_rn((float)q, 0.0625f);
    }
    float* op = out + (size_t)blockIdx.z * W * H + r1 + x;
    if (VEC) *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (x + i < W) op[i] = o[i];
    }
}

extern "C" int v3d_temporal_filter_batch(const float* depth, size_t depth_stride, const uint8_t* gray, size_t gray_stride, int T,
                                         int W, int H, int t0, int n, int R, int tau, int fill, const uint8_t* cut, float* out,
                                         void* stream)
{
    if (!depth || !gray || !cut || !out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (W < 1 || H < 1) { v3d_set_error("bad geometry %dx%d", W, H); return V3D_ERR_ARG; }
    if (tp_check_window(T, t0, n, R) != V3D_OK) return V3D_ERR_ARG;
    if (tau < 1 || tau > 255) { v3d_set_error("tau %d outside [1, 255]", tau); return V3D_ERR_ARG; }
    if (fill != 0 && fill != 1) { v3d_set_error("fill must be 0 or 1"); return V3D_ERR_ARG; }
    const size_t npx = (size_t)W * H;
    if (T > 1 && (depth_stride < npx || gray_stride < npx)) { v3d_set_error("frame stride below the frame size %zu", npx); return V3D_ERR_ARG; }
    if (v3d_cdiv(H, 4) > 65535) { v3d_set_error("height %d not supported", H); return V3D_ERR_UNSUPPORTED; }
    const uint32_t mul = (uint32_t)((((uint64_t)1 << 32) + 9u * (uint32_t)tau - 1u) / (9u * (uint32_t)tau));
    const bool vec = (W & 3) == 0 && (depth_stride & 3) == 0 && (gray_stride & 3) == 0 && ((uintptr_t)depth & 15) == 0
                     && ((uintptr_t)gray & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid(v3d_cdiv(W, 256), v3d_cdiv(H, 4), n), block(64, 4);
    if (vec) hipLaunchKernelGGL(k_tp_filter<true>, grid, block, 0, (hipStream_t)stream, depth, depth_stride, gray, gray_stride, T, W, H,
                                t0, R, mul, fill, cut, out);
    else hipLaunchKernelGGL(k_tp_filter<false>, grid, block, 0, (hipStream_t)stream, depth, depth_stride, gray, gray_stride, T, W, H,
                            t0, R, mul, fill, cut, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
