// v3d_quality.hip -- the stereo quality report's two ground-truth-free measures ("Quality report"; contract
// in include/v3d_hip.h, NumPy restatement in tests/quality_ref.py).  Reprojection error: how well the right view, pulled back
// through the int16 disparity, explains the left view, next to the same pixels at disparity 0.  Flicker: how far the fixed-point
// depth of pixels whose luma stood still moves from one frame to the next.  Both are integer sums over pixels, so no bit depends
// on a schedule.  Two launches per entry: workgroups over (row band, frame or pair) leave one partial record each in the
// workspace (plain stores, no atomics, no flags), then one workgroup per frame or pair adds its partial records up.
#include "v3d_common.h"
#include "v3d_wave.h"

#define Q_THREADS 256
#define Q_WAVES (Q_THREADS / 64)
#define Q_BAND_GROUPS 2048          // pixel groups per workgroup at most: 8 per lane
#define Q_RF V3D_QUALITY_REPROJ_FIELDS
#define Q_FF V3D_QUALITY_FLICKER_FIELDS
#define Q_RPX 16                    // pixels a lane owns per group, reprojection
#define Q_FPX 8                     // flicker

// rows per band: a band is at most Q_BAND_GROUPS groups, so a lane owns at most 8 groups = 128 (reprojection) or 64 (flicker)
// pixels.  That is the u32 headroom of a lane's partial sums: e^2 <= 4080^2 = 16 646 400 and 2^32 / 16 646 400 = 258 pixels.
static inline int q_band_rows(int W, int px) { const int g = v3d_cdiv(W, px); return Q_BAND_GROUPS / g > 1 ? Q_BAND_GROUPS / g : 1; }
static inline int q_bands(int W, int H, int px) { return v3d_cdiv(H, q_band_rows(W, px)); }

// a workgroup's lane partials -> its record: butterfly inside the wave, the waves' sums through LDS, one u64 store per field
template <int F, typename T>
__device__ __forceinline__ void q_block_store(const T (&acc)[F], unsigned long long* __restrict__ rec)
{
    __shared__ unsigned long long part[Q_WAVES][F];
    const int tid = threadIdx.x;
    unsigned long long t[F];
#pragma unroll
    for (int k = 0; k < F; k++) t[k] = wave_sum_u64(acc[k]);
    const unsigned long long s = block_sum_u64<Q_WAVES, F>(t, tid & 63, tid >> 6, tid, part);
    if (tid < F) rec[tid] = s;
}

__device__ __forceinline__ int q_byte(const uint32_t* w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu); }

// ---- reprojection: integers only.  R's gather reads the right row straight from global memory: it is row-local (two
// neighbouring bytes at most d / 16 columns to the left of bytes this workgroup has just loaded for e0), so it is served by the
// cache for any disparity the contract allows, without an LDS apron and its fall-back ----
template <bool VEC>
__global__ __launch_bounds__(Q_THREADS) void k_q_reproj(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right, int W, int H,
                                                        size_t pitch, size_t stride, const int16_t* __restrict__ disp, size_t dstride,
                                                        int band_rows, int bad16, unsigned long long* __restrict__ ws)
{
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int G = (W + Q_RPX - 1) / Q_RPX;
    const int r0 = band * band_rows, rows = min(band_rows, H - r0);
    const uint8_t* L = left + (size_t)f * stride;
    const uint8_t* R = right + (size_t)f * stride;
    const int16_t* D = disp + (size_t)f * dstride;
    uint32_t acc[Q_RF] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
    for (int it = tid; it < rows * G; it += Q_THREADS) {
        const int ry = it / G, x0 = (it - ry * G) * Q_RPX, y = r0 + ry;
        const uint8_t* Rr = R + (size_t)y * pitch;
        const int16_t* Dr = D + (size_t)y * W;
        const uint4 lv = row_load16<VEC>(L + (size_t)y * pitch, x0, W), rv = row_load16<VEC>(Rr, x0, W);
        const uint32_t lw[4] = { lv.x, lv.y, lv.z, lv.w }, rw[4] = { rv.x, rv.y, rv.z, rv.w };
        uint32_t dw[8];
        if (VEC && x0 + Q_RPX <= W) {
            const uint4 a = *reinterpret_cast<const uint4*>(Dr + x0), b = *reinterpret_cast<const uint4*>(Dr + x0 + 8);
            dw[0] = a.x; dw[1] = a.y; dw[2] = a.z; dw[3] = a.w; dw[4] = b.x; dw[5] = b.y; dw[6] = b.z; dw[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {                       // beyond the row: 0 = invalid
                const uint32_t lo = x0 + 2 * i < W ? (uint16_t)Dr[x0 + 2 * i] : 0u, hi = x0 + 2 * i + 1 < W ? (uint16_t)Dr[x0 + 2 * i + 1] : 0u;
                dw[i] = lo | (hi << 16);
            }
        }
#pragma unroll
        for (int i = 0; i < Q_RPX; i++) {
            const int d = (int)(int16_t)(dw[i >> 1] >> (16 * (i & 1)));
            const int u = 16 * (x0 + i) - d;
            acc[0] += d >= 1;
            if (d >= 1 && u >= 0) {                             // d >= 1: (u >> 4) + 1 <= x0 + i <= W - 1
                const int fr = u & 15, a = Rr[u >> 4], b = Rr[(u >> 4) + 1];
                const int lp = q_byte(lw, i), rp = q_byte(rw, i);
                const int e = abs(16 * lp - ((16 - fr) * a + fr * b)), e0 = 16 * abs(lp - rp);
                acc[1] += 1u;
                acc[2] += (uint32_t)e;
                acc[3] += (uint32_t)(e * e);
                acc[4] += e > bad16;
                acc[5] += (uint32_t)e0;
                acc[6] += (uint32_t)(e0 * e0);
                acc[7] += e0 > bad16;
            }
        }
    }
    q_block_store<Q_RF>(acc, ws + ((size_t)f * gridDim.x + band) * Q_RF);
}

// ---- flicker: the only float step is v3d_d16_tap (the temporal stage's own fixed point): NaN and -inf are invalid, +inf and
// every depth above the range count as 32767, nothing out of an int's range is ever converted ----
__device__ __forceinline__ int q_d16(float D) { return v3d_d16_tap(D); }

template <bool VEC>
__device__ __forceinline__ void q_load_depth(const float* __restrict__ row, int x0, int W, int (&d)[Q_FPX])
{
    if (VEC && x0 + Q_FPX <= W) {
        const float4 a = *reinterpret_cast<const float4*>(row + x0), b = *reinterpret_cast<const float4*>(row + x0 + 4);
        d[0] = q_d16(a.x); d[1] = q_d16(a.y); d[2] = q_d16(a.z); d[3] = q_d16(a.w);
        d[4] = q_d16(b.x); d[5] = q_d16(b.y); d[6] = q_d16(b.z); d[7] = q_d16(b.w);
    } else {
#pragma unroll
        for (int i = 0; i < Q_FPX; i++) d[i] = x0 + i < W ? q_d16(row[x0 + i]) : 0;
    }
}

template <bool VEC>
__global__ __launch_bounds__(Q_THREADS) void k_q_flicker(const float* __restrict__ depth, size_t dstride, const uint8_t* __restrict__ gray,
                                                         size_t gstride, int W, int H, int band_rows, int still, int jump16,
                                                         unsigned long long* __restrict__ ws)
{
    const int band = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
    const int G = (W + Q_FPX - 1) / Q_FPX;
    const int r0 = band * band_rows, rows = min(band_rows, H - r0);
    const float* D0 = depth + (size_t)u * dstride;
    const float* D1 = D0 + dstride;
    const uint8_t* Y0 = gray + (size_t)u * gstride;
    const uint8_t* Y1 = Y0 + gstride;
    uint32_t acc[Q_FF] = { 0u, 0u, 0u, 0u };
    for (int it = tid; it < rows * G; it += Q_THREADS) {
        const int ry = it / G, x0 = (it - ry * G) * Q_FPX;
        const size_t o = (size_t)(r0 + ry) * W;
        const uint2 ya = row_load8<VEC>(Y0 + o, x0, W), yb = row_load8<VEC>(Y1 + o, x0, W);
        const uint32_t aw[2] = { ya.x, ya.y }, bw[2] = { yb.x, yb.y };
        int da[Q_FPX], db[Q_FPX];
        q_load_depth<VEC>(D0 + o, x0, W, da);
        q_load_depth<VEC>(D1 + o, x0, W, db);
#pragma unroll
        for (int i = 0; i < Q_FPX; i++) {                       // beyond the row: both lumas 0, both d16 invalid
            const int dy = abs(q_byte(bw, i) - q_byte(aw, i)), dd = abs(db[i] - da[i]);
            const bool s = dy <= still && da[i] >= 1 && db[i] >= 1;
            acc[0] += (uint32_t)dy;
            acc[1] += s;
            acc[2] += s ? (uint32_t)dd : 0u;
            acc[3] += s && dd > jump16;
        }
    }
    q_block_store<Q_FF>(acc, ws + ((size_t)u * gridDim.x + band) * Q_FF);
}

// ---- launch 2: one workgroup per frame or pair adds its nb partial records ----
template <int F>
__global__ __launch_bounds__(Q_THREADS) void k_q_sum(const unsigned long long* __restrict__ ws, int nb, unsigned long long* __restrict__ out)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* rec = ws + (size_t)f * nb * F;
    unsigned long long s[F];
#pragma unroll
    for (int k = 0; k < F; k++) s[k] = 0;
    for (int b = tid; b < nb; b += Q_THREADS)
#pragma unroll
        for (int k = 0; k < F; k++) s[k] += rec[(size_t)b * F + k];
    q_block_store<F>(s, out + (size_t)f * F);
}

// what both entries refuse about the plane and the two pointers every call has; 0 = fine
static int q_check_common(int count, int lo, const char* what, int W, int H, const void* out, const void* ws)
{
    if (count < lo || count > 65535) { v3d_set_error("%s %d outside [%d, 65535]", what, count, lo); return V3D_ERR_ARG; }
    if (W < 1 || H < 1) { v3d_set_error("empty plane %dx%d", W, H); return V3D_ERR_ARG; }
    if (W > 8192 || H > 65535) { v3d_set_error("quality measures of a %dx%d plane not supported (W <= 8192, H <= 65535)", W, H); return V3D_ERR_UNSUPPORTED; }
    if (ws && ((uintptr_t)ws & 15)) { v3d_set_error("ws must be 16-byte aligned"); return V3D_ERR_ARG; }
    if (out && ((uintptr_t)out & 7)) { v3d_set_error("out must be 8-byte aligned"); return V3D_ERR_ARG; }
    return V3D_OK;
}

extern "C" size_t v3d_quality_reproj_ws_bytes(int n, int W, int H)
{
    if (q_check_common(n, 1, "frame count", W, H, nullptr, nullptr) != V3D_OK) return 0;
    return (size_t)n * (size_t)q_bands(W, H, Q_RPX) * Q_RF * sizeof(uint64_t);
}

extern "C" int v3d_quality_reproj_batch(const uint8_t* left_gray, const uint8_t* right_gray, int n, int W, int H, int pitch,
                                        size_t frame_stride, const int16_t* disp16, size_t disp_stride, int bad_thr, uint64_t* out,
                                        void* ws, void* stream)
{
    if (!left_gray || !right_gray || !disp16 || !out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    const int rc = q_check_common(n, 1, "frame count", W, H, out, ws);
    if (rc != V3D_OK) return rc;
    if (pitch < W) { v3d_set_error("pitch %d below the width %d", pitch, W); return V3D_ERR_ARG; }
    if (n > 1 && (frame_stride < (size_t)H * (size_t)pitch || disp_stride < (size_t)W * (size_t)H)) {
        v3d_set_error("frame stride %zu / disparity stride %zu below the frame sizes %zu / %zu", frame_stride, disp_stride,
                      (size_t)H * (size_t)pitch, (size_t)W * (size_t)H);
        return V3D_ERR_ARG;
    }
    if (bad_thr < 0 || bad_thr > 255) { v3d_set_error("bad_thr %d outside [0, 255]", bad_thr); return V3D_ERR_ARG; }
    const int band_rows = q_band_rows(W, Q_RPX), nb = q_bands(W, H, Q_RPX);
    const bool vec = (((uintptr_t)left_gray | (uintptr_t)right_gray | (uintptr_t)disp16) & 15) == 0 && (pitch & 15) == 0 && (W & 7) == 0 &&
                     (n == 1 || ((frame_stride & 15) == 0 && (disp_stride & 7) == 0));
    unsigned long long* part = reinterpret_cast<unsigned long long*>(ws);
    const dim3 grid(nb, n), block(Q_THREADS);
    if (vec) hipLaunchKernelGGL(k_q_reproj<true>, grid, block, 0, (hipStream_t)stream, left_gray, right_gray, W, H, (size_t)pitch, frame_stride, disp16, disp_stride, band_rows, 16 * bad_thr, part);
    else hipLaunchKernelGGL(k_q_reproj<false>, grid, block, 0, (hipStream_t)stream, left_gray, right_gray, W, H, (size_t)pitch, frame_stride, disp16, disp_stride, band_rows, 16 * bad_thr, part);
    V3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_q_sum<Q_RF>, dim3(n), block, 0, (hipStream_t)stream, part, nb, reinterpret_cast<unsigned long long*>(out));
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" size_t v3d_quality_flicker_ws_bytes(int T, int W, int H)
{
    if (q_check_common(T, 2, "frame count", W, H, nullptr, nullptr) != V3D_OK) return 0;
    return (size_t)(T - 1) * (size_t)q_bands(W, H, Q_FPX) * Q_FF * sizeof(uint64_t);
}

extern "C" int v3d_quality_flicker_batch(const float* depth, size_t depth_stride, const uint8_t* gray, size_t gray_stride, int T, int W,
                                         int H, int still, int jump16, uint64_t* out, void* ws, void* stream)
{
    if (!depth || !gray || !out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    const int rc = q_check_common(T, 2, "frame count", W, H, out, ws);
    if (rc != V3D_OK) return rc;
    const size_t npx = (size_t)W * (size_t)H;
    if (depth_stride < npx || gray_stride < npx) {
        v3d_set_error("depth stride %zu / gray stride %zu below the frame size %zu", depth_stride, gray_stride, npx);
        return V3D_ERR_ARG;
    }
    if (still < 0 || still > 255) { v3d_set_error("still %d outside [0, 255]", still); return V3D_ERR_ARG; }
    if (jump16 < 0 || jump16 > 32767) { v3d_set_error("jump16 %d outside [0, 32767]", jump16); return V3D_ERR_ARG; }
    const int band_rows = q_band_rows(W, Q_FPX), nb = q_bands(W, H, Q_FPX);
    const bool vec = ((uintptr_t)depth & 15) == 0 && ((uintptr_t)gray & 7) == 0 && (W & 7) == 0 && (depth_stride & 3) == 0 && (gray_stride & 7) == 0;
    unsigned long long* part = reinterpret_cast<unsigned long long*>(ws);
    const dim3 grid(nb, T - 1), block(Q_THREADS);
    if (vec) hipLaunchKernelGGL(k_q_flicker<true>, grid, block, 0, (hipStream_t)stream, depth, depth_stride, gray, gray_stride, W, H, band_rows, still, jump16, part);
    else hipLaunchKernelGGL(k_q_flicker<false>, grid, block, 0, (hipStream_t)stream, depth, depth_stride, gray, gray_stride, W, H, band_rows, still, jump16, part);
    V3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_q_sum<Q_FF>, dim3(T - 1), block, 0, (hipStream_t)stream, part, nb, reinterpret_cast<unsigned long long*>(out));
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
