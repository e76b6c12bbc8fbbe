// v3d_temporal.hip -- temporal depth stabilisation between sbs_to_disparity and the u16 normalisation (DESIGN.md section 4,
// "Temporal stabilisation" and "Motion-compensated window"; contract in include/v3d_hip.h, NumPy restatements in
// tests/temporal_ref.py and tests/temporal_mc_ref.py).  Per target frame t and pixel p, over the frames u = t+k of the window
// that no scene cut separates from t, frame u read at q = p (plain) or q = p + m (compensated, m the chained block vector):
//   d16_u = rint(16 D_u(q))  (valid iff >= 1)       s_k = 3x3 edge-replicated sum of |Y_u(q + .) - Y_t(p + .)|  (0..2295)
//   w_k = (R + 1 - |k|) * max(0, 256 - floor(256 s_k / (9 tau))) * valid      out16 = floor((2 sum w d16 + sum w) / (2 sum w))
// All integers, so the bits do not depend on any order of evaluation.  The closed forms are v3d_temporal_math.h's, d16 is
// v3d_depth_math.h's.  Cut flags and the clip-stable ranges are produced and consumed on the device: no entry synchronises.
// This file holds the cuts, the window range and the one filter kernel behind both filter entries; the block search that gives the
// compensated window its fields and cuts is v3d_temporal_mc.hip, the per-frame min/max (v3d_depth_minmax_batch) and the u16
// samples against the window range (v3d_depth_to_u16_range_batch) live in v3d_range.hip.
#include "v3d_temporal_internal.h"
#include "v3d_wave.h"

#define TP_MAX_R 8

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
    __shared__ unsigned long long part[4][1];
    const unsigned long long t[1] = { wave_sum_u64(acc) };
    const unsigned long long s = block_sum_u64<4, 1>(t, threadIdx.x & 63, threadIdx.x >> 6, threadIdx.x, part);
    if (threadIdx.x == 0) atomicAdd(sums + u, s);
}
__global__ void k_tp_cutflag(const unsigned long long* __restrict__ sums, int T, int c, size_t npx, uint8_t* __restrict__ cut)
{
    for (int u = blockIdx.x * 256 + threadIdx.x; u < T; u += gridDim.x * 256) cut[u] = (u >= 1 && v3d_tp_is_cut(sums[u], c, npx)) ? 1 : 0;
}
void v3d_tp_launch_zero(unsigned long long* sums, int T, hipStream_t st)
{
    hipLaunchKernelGGL(k_tp_zero, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, sums, T);
}
void v3d_tp_launch_cutflag(const unsigned long long* sums, int T, int c, size_t npx, uint8_t* cut, hipStream_t st)
{
    hipLaunchKernelGGL(k_tp_cutflag, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, sums, T, c, npx, cut);
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
    v3d_tp_launch_zero(sums, T, st);
    if (T > 1) {
        const int vec = (((uintptr_t)gray & 15) == 0 && (gray_stride & 15) == 0) ? 1 : 0;
        const size_t want = (npx + 4095) / 4096;                             // one 16-px step per lane fills a block with 4096 px
        const size_t per = (size_t)(2048 / (T - 1) > 32 ? 2048 / (T - 1) : 32);
        const int bx = (int)(want < per ? (want ? want : 1) : per);
        hipLaunchKernelGGL(k_tp_sad, dim3(bx, T - 1), dim3(256), 0, st, gray, gray_stride, npx, vec, sums);
    }
    v3d_tp_launch_cutflag(sums, T, c, npx, cut_out, st);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- clip-stable range: min of the minima and max of the maxima over the admissible window ----
__global__ void k_tp_range(const float* __restrict__ mm, const uint8_t* __restrict__ cut, int T, int t0, int n, int R,
                           float* __restrict__ lohi)
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        int a, b;
        v3d_tp_admissible(cut, T, t0 + j, R, &a, &b);
        float lo = mm[2 * a], hi = mm[2 * a + 1];
        bool nan = lo != lo || hi != hi;                    // ndarray.min() / .max(): a NaN bound in any frame of the window, at any
        for (int u = a + 1; u <= b; u++) {                  // position, makes both bounds of the target NaN
            const float l = mm[2 * u], h = mm[2 * u + 1];
            nan = nan || l != l || h != h;
            lo = l < lo ? l : lo;
            hi = h > hi ? h : hi;
        }
        lohi[2 * j] = nan ? __builtin_nanf("") : lo; lohi[2 * j + 1] = nan ? __builtin_nanf("") : hi;
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

// ---- the filter (the hot kernel), plain (MC = false: frame u read at p, the fields unused) and compensated (MC = true) ----
// One lane owns 4 horizontally adjacent pixels of one row of one target (one 16x16 block, so one vector m); a 64 x 4 workgroup
// covers 256 x 4 px.  A gray row segment is the dword of the 4 pixels plus its left and right neighbours (edge-replicated) packed
// into 48 bits {hi, lo}; pixel i's three horizontal neighbours are the 24-bit window (hi:lo) >> 8i, and |Y_u - Y_t| over them is
// one v_sad_u8 on the masked windows (the fourth byte is zero on both sides).  Three rows accumulate into the 3x3 sum.
// The window is walked as u = t, t+1 .. uhi, then t-1 .. ulo: the order in which a compensated lane chains m, one int16 pair per
// step, forward from t and then backward from t (integer sums: the order of the taps does not matter).
// VEC: W, both frame strides and all base addresses allow dword gray loads and 16-byte depth loads / stores; the other
// instantiation loads and stores element by element (odd widths, unaligned views).  A displaced segment starts at x + m.x, any
// alignment: VEC lanes whose columns lie inside the row take one unaligned dword, or one 16-byte depth load, every other lane
// goes column by column, gray clamped to the row, depth outside the row invalid (weight 0).
struct __attribute__((packed, aligned(1))) tp_u32u { uint32_t v; };
struct __attribute__((packed, aligned(4))) tp_f4u { float v[4]; };

template <bool VEC, bool MC>
__device__ __forceinline__ void tp_gray_row(const uint8_t* __restrict__ row, int x, int W, uint32_t& lo, uint32_t& hi)
{
    const int w1 = W - 1;
    uint32_t c;
    if (VEC && (!MC || (x >= 0 && x + 3 < W))) c = reinterpret_cast<const tp_u32u*>(row + x)->v;
    else c = (uint32_t)row[min(max(x, 0), w1)] | ((uint32_t)row[min(max(x + 1, 0), w1)] << 8)
             | ((uint32_t)row[min(max(x + 2, 0), w1)] << 16) | ((uint32_t)row[min(max(x + 3, 0), w1)] << 24);
    const uint32_t L = row[min(max(x - 1, 0), w1)], Rb = row[min(max(x + 4, 0), w1)];
    lo = L | (c << 8);
    hi = (c >> 24) | (Rb << 8);
}

// one step of the chain: m += the field's vector of the block that holds clamp(c_b + m)
__device__ __forceinline__ void tp_step(const int16_t* __restrict__ field, int BW, int W, int H, int cbx, int cby, int& mx, int& my)
{
    const int px = min(max(cbx + mx, 0), W - 1) >> 4, py = min(max(cby + my, 0), H - 1) >> 4;
    const int16_t* f = field + ((size_t)py * BW + px) * 2;
    mx += f[0];
    my += f[1];
}

template <bool VEC, bool MC>
__global__ __launch_bounds__(256) void k_tp_filter(const float* __restrict__ depth, size_t dstride, const uint8_t* __restrict__ gray,
                                                   size_t gstride, int T, int W, int H, int t0, int R, uint32_t mul, int fill,
                                                   const uint8_t* __restrict__ cut, const int16_t* __restrict__ mv_fwd,
                                                   const int16_t* __restrict__ mv_bwd, float* __restrict__ out)
{
    const int t = t0 + blockIdx.z;
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    const int y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H) return;
    int ulo, uhi;
    v3d_tp_admissible(cut, T, t, R, &ulo, &uhi);
    const int BW = (W + 15) >> 4, BH = (H + 15) >> 4;
    const size_t fsz = (size_t)BW * BH * 2;
    const int cbx = min((x & ~15) + 8, W - 1), cby = min((y & ~15) + 8, H - 1);

    uint32_t ref[3][4];
    {
        const uint8_t* g = gray + (size_t)t * gstride;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            uint32_t lo, hi;
            tp_gray_row<VEC, MC>(g + (size_t)min(max(y + r - 1, 0), H - 1) * W, x, W, lo, hi);
#pragma unroll
            for (int i = 0; i < 4; i++) ref[r][i] = alignbit(hi, lo, 8 * i) & 0xFFFFFFu;
        }
    }
    uint32_t Wsum[4] = { 0, 0, 0, 0 }, Dsum[4] = { 0, 0, 0, 0 };
    bool centre[4] = { false, false, false, false };
    const int nf = uhi - t, nb = t - ulo;
    int mx = 0, my = 0;                                     // stay 0 without MC
    for (int j = 0; j <= nf + nb; j++) {                    // u = t, t+1 .. uhi, then t-1 .. ulo
        const int u = j <= nf ? t + j : t - (j - nf);
        if (MC) {
            if (j == nf + 1) mx = my = 0;
            if (j > nf) tp_step(mv_bwd + (size_t)(u + 1) * fsz, BW, W, H, cbx, cby, mx, my);
            else if (j >= 1) tp_step(mv_fwd + (size_t)(u - 1) * fsz, BW, W, H, cbx, cby, mx, my);
        }
        const int qx = x + mx, qy = y + my;
        if (MC && (qy < 0 || qy >= H || qx + 3 < 0 || qx >= W)) continue;   // every tap outside the frame: weight 0
        uint32_t s[4] = { 0, 0, 0, 0 };
        if (u != t) {
            const uint8_t* g = gray + (size_t)u * gstride;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                uint32_t lo, hi;
                tp_gray_row<VEC, MC>(g + (size_t)min(max(qy + r - 1, 0), H - 1) * W, qx, W, lo, hi);
#pragma unroll
                for (int i = 0; i < 4; i++) s[i] = __builtin_amdgcn_sad_u8(alignbit(hi, lo, 8 * i) & 0xFFFFFFu, ref[r][i], s[i]);
            }
        }
        const float* dp = depth + (size_t)u * dstride + (size_t)qy * W;
        float d[4];
        if (VEC && (!MC || (qx >= 0 && qx + 3 < W))) {
            const tp_f4u v = *reinterpret_cast<const tp_f4u*>(dp + qx);
            d[0] = v.v[0]; d[1] = v.v[1]; d[2] = v.v[2]; d[3] = v.v[3];
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) d[i] = (qx + i >= 0 && qx + i < W) ? dp[qx + i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            // validity is decided on the float, as v3d_d16_tap decides it: NaN, -inf and every rint(16 D) < 1 are invalid whatever
            // the conversion makes of them, and an invalid tap's weight is 0.  Only the value keeps the bare conversion: v3d_d16_tap's
            // clamp to 32767 cost 3 to 4 % of this kernel ("Non-finite input"), so a tap above the domain D <= 2047.9375
            // (+inf included) is valid with a value that wraps: the header leaves such a pixel's value unspecified
            const float r16 = v3d_d16(d[i]);
            const bool valid = r16 >= 1.0f;
            const int d16 = (int)r16;
            if (u == t) centre[i] = valid;
            const uint32_t w = v3d_tp_weight(s[i], mul, R, u - t, valid ? 1 : 0);
            Wsum[i] += w;
            Dsum[i] += w * (uint32_t)d16;                   // w = 0 where d16 is invalid
        }
    }
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) o[i] = __fmul_rn((float)v3d_tp_quotient(Wsum[i], Dsum[i], fill, centre[i]), 0.0625f);
    float* op = out + (size_t)blockIdx.z * W * H + (size_t)y * W + x;
    if (VEC) *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
    else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (x + i < W) op[i] = o[i];
    }
}

// both filter entries: the checks, the VEC decision and the launch; `mc` adds the two fields
static int tp_filter(const float* depth, size_t depth_stride, const uint8_t* gray, size_t gray_stride, int T, int W, int H, int t0, int n,
                     int R, int tau, int fill, const uint8_t* cut, bool mc, const int16_t* mv_fwd, const int16_t* mv_bwd, float* out,
                     void* stream)
{
    if (!depth || !gray || !cut || !out || (mc && (!mv_fwd || !mv_bwd))) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (W < 1 || H < 1) { v3d_set_error("bad geometry %dx%d", W, H); return V3D_ERR_ARG; }
    if (tp_check_window(T, t0, n, R) != V3D_OK) return V3D_ERR_ARG;
    if (tau < 1 || tau > 255) { v3d_set_error("tau %d outside [1, 255]", tau); return V3D_ERR_ARG; }
    if (fill != 0 && fill != 1) { v3d_set_error("fill must be 0 or 1"); return V3D_ERR_ARG; }
    const size_t npx = (size_t)W * H;
    if (T > 1 && (depth_stride < npx || gray_stride < npx)) { v3d_set_error("frame stride below the frame size %zu", npx); return V3D_ERR_ARG; }
    if (mc && (((uintptr_t)mv_fwd | (uintptr_t)mv_bwd) & 1) != 0) { v3d_set_error("the fields must be 2-byte aligned"); return V3D_ERR_ARG; }
    if (v3d_cdiv(H, 4) > 65535) { v3d_set_error("height %d not supported", H); return V3D_ERR_UNSUPPORTED; }
    const bool vec = (W & 3) == 0 && (depth_stride & 3) == 0 && (gray_stride & 3) == 0 && ((uintptr_t)depth & 15) == 0
                     && ((uintptr_t)gray & 3) == 0 && ((uintptr_t)out & 15) == 0;
    const auto kernel = mc ? (vec ? k_tp_filter<true, true> : k_tp_filter<false, true>)
                           : (vec ? k_tp_filter<true, false> : k_tp_filter<false, false>);
    hipLaunchKernelGGL(kernel, dim3(v3d_cdiv(W, 256), v3d_cdiv(H, 4), n), dim3(64, 4), 0, (hipStream_t)stream, depth, depth_stride, gray,
                       gray_stride, T, W, H, t0, R, v3d_tp_rw_magic(tau), fill, cut, mv_fwd, mv_bwd, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_temporal_filter_batch(const float* depth, size_t depth_stride, const uint8_t* gray, size_t gray_stride, int T,
                                         int W, int H, int t0, int n, int R, int tau, int fill, const uint8_t* cut, float* out,
                                         void* stream)
{
    return tp_filter(depth, depth_stride, gray, gray_stride, T, W, H, t0, n, R, tau, fill, cut, false, nullptr, nullptr, out, stream);
}

extern "C" int v3d_temporal_filter_mc_batch(const float* depth, size_t depth_stride, const uint8_t* gray, size_t gray_stride, int T,
                                            int W, int H, int t0, int n, int R, int tau, int fill, const uint8_t* cut,
                                            const int16_t* mv_fwd, const int16_t* mv_bwd, float* out, void* stream)
{
    return tp_filter(depth, depth_stride, gray, gray_stride, T, W, H, t0, n, R, tau, fill, cut, true, mv_fwd, mv_bwd, out, stream);
}
