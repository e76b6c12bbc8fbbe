// v3d_register.hip -- spatial registration of the SBS eye and the 4K frame ("Spatial registration"; contract in
// include/v3d_hip.h, NumPy restatement in tests/register_ref.py).  Three entries: the row and column sums of a luma plane, the
// score of 1-D affine maps between two such profiles, and the u16 warp that applies the fitted map to the low-res depth.  All
// integers: no bit depends on a schedule.
#include "v3d_common.h"
#include "v3d_wave.h"

#define RG_THREADS 1024
#define RG_WAVES 16
#define RG_SEG 1024                 // columns of one wave: 64 lanes x 16 bytes
#define RG_MAX_LANE_ROWS 256        // 256 * 255 = 65280 < 2^16: what a packed 16-bit column sum holds
#define RG_TARGET_BLOCKS 1024

// ---- 1. profiles.  A plane's rows are cut into segments of 1024 columns, one wave each: nseg = ceil(W / 1024) segments, ny =
// 16 / nseg row phases per workgroup.  A workgroup takes a band of ny * L rows of one frame (L <= 256 rows per lane).  A lane owns
// one 16-byte column group of its segment and every ny-th row of the band: the row's 16 bytes fold to the wave's row sum
// (v_sad_u8, butterfly), the columns accumulate as packed 16-bit pairs like k_fm_signature's.  LDS gathers the segments of a row
// and the phases of a column; the band's column sums go to ws, a second launch adds the bands (no global atomics). ----
struct rg_plan { int nseg, ny, L, R, bands; };

static rg_plan rg_profile_plan(int n, int W, int H)
{
    rg_plan p;
    p.nseg = v3d_cdiv(W, RG_SEG);                                   // 1 .. 8
    p.ny = RG_WAVES / p.nseg;                                       // 16 .. 2
    const long long want = ((long long)H * n + (long long)p.ny * RG_TARGET_BLOCKS - 1) / ((long long)p.ny * RG_TARGET_BLOCKS);
    p.L = want < 8 ? 8 : want > RG_MAX_LANE_ROWS ? RG_MAX_LANE_ROWS : (int)want;
    p.R = p.L * p.ny;                                               // <= 4096, and R * nseg <= 4096
    p.bands = v3d_cdiv(H, p.R);
    return p;
}

__device__ __forceinline__ void rg_acc(uint32_t (&acc)[8], uint32_t& rs, const uint4 p)
{
    acc[0] += p.x & 0x00FF00FFu; acc[1] += (p.x >> 8) & 0x00FF00FFu;
    acc[2] += p.y & 0x00FF00FFu; acc[3] += (p.y >> 8) & 0x00FF00FFu;
    acc[4] += p.z & 0x00FF00FFu; acc[5] += (p.z >> 8) & 0x00FF00FFu;
    acc[6] += p.w & 0x00FF00FFu; acc[7] += (p.w >> 8) & 0x00FF00FFu;
    rs = __builtin_amdgcn_sad_u8(p.x, 0u, __builtin_amdgcn_sad_u8(p.y, 0u, __builtin_amdgcn_sad_u8(p.z, 0u, __builtin_amdgcn_sad_u8(p.w, 0u, 0u))));
}

template <bool VEC>
__global__ __launch_bounds__(RG_THREADS) void k_rg_profiles(const uint8_t* __restrict__ gray, int W, int H, size_t pitch, size_t stride,
                                                            int nseg, int ny, int L, uint32_t* __restrict__ part,
                                                            uint32_t* __restrict__ row_out)
{
    __shared__ uint32_t colp[8 * RG_SEG];                           // the band's column sums
    __shared__ uint32_t rowp[4096];                                 // [row of the band][segment]
    const int band = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = L * ny, r0 = band * R, r1 = min(r0 + R, H);
    for (int i = tid; i < nseg * RG_SEG; i += RG_THREADS) colp[i] = 0u;
    __syncthreads();
    const int ty = wave / nseg, sx = wave - ty * nseg;
    if (ty < ny) {                                                  // 16 is no multiple of 3, 5, 6, 7 segments: the last waves idle
        const int x0 = (sx * 64 + lane) * 16;
        const uint8_t* base = gray + (size_t)f * stride;
        uint32_t acc[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
        int r = r0 + ty, k = ty;
        for (; r + 3 * ny < r1; r += 4 * ny, k += 4 * ny) {         // four rows in flight per lane
            const uint4 a = row_load16<VEC>(base + (size_t)r * pitch, x0, W);
            const uint4 b = row_load16<VEC>(base + (size_t)(r + ny) * pitch, x0, W);
            const uint4 c = row_load16<VEC>(base + (size_t)(r + 2 * ny) * pitch, x0, W);
            const uint4 d = row_load16<VEC>(base + (size_t)(r + 3 * ny) * pitch, x0, W);
            uint32_t sa, sb, sc, sd;
            rg_acc(acc, sa, a); rg_acc(acc, sb, b); rg_acc(acc, sc, c); rg_acc(acc, sd, d);
            sa = wave_sum_u32(sa); sb = wave_sum_u32(sb); sc = wave_sum_u32(sc); sd = wave_sum_u32(sd);
            if (lane == 0) {
                rowp[k * nseg + sx] = sa; rowp[(k + ny) * nseg + sx] = sb;
                rowp[(k + 2 * ny) * nseg + sx] = sc; rowp[(k + 3 * ny) * nseg + sx] = sd;
            }
        }
        for (; r < r1; r += ny, k += ny) {
            uint32_t s;
            rg_acc(acc, s, row_load16<VEC>(base + (size_t)r * pitch, x0, W));
            s = wave_sum_u32(s);
            if (lane == 0) rowp[k * nseg + sx] = s;
        }
#pragma unroll
        for (int i = 0; i < 16; i++)                                // widen: a lane has summed at most 256 rows
            if (x0 + i < W) atomicAdd(&colp[x0 + i], (acc[2 * (i >> 2) + (i & 1)] >> (16 * ((i >> 1) & 1))) & 0xFFFFu);
    }
    __syncthreads();
    for (int x = tid; x < W; x += RG_THREADS) part[((size_t)f * gridDim.x + band) * W + x] = colp[x];
    for (int t = tid; t < r1 - r0; t += RG_THREADS) {
        uint32_t s = 0u;
        for (int g = 0; g < nseg; g++) s += rowp[t * nseg + g];
        row_out[(size_t)f * H + r0 + t] = s;
    }
}

__global__ __launch_bounds__(256) void k_rg_colsum(const uint32_t* __restrict__ part, int W, int bands, uint32_t* __restrict__ col_out)
{
    const int x = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (x >= W) return;
    uint32_t s = 0u;
    for (int b = 0; b < bands; b++) s += part[((size_t)f * bands + b) * W + x];
    col_out[(size_t)f * W + x] = s;
}

static bool rg_profile_args_ok(int n, int W, int H)
{
    return n >= 1 && n <= 65535 && W >= 1 && W <= 8192 && H >= 1 && H <= 8192;
}

extern "C" size_t v3d_plane_profiles_ws_bytes(int n, int W, int H)
{
    if (!rg_profile_args_ok(n, W, H)) return 0;
    return (size_t)n * rg_profile_plan(n, W, H).bands * W * sizeof(uint32_t);
}

extern "C" int v3d_plane_profiles_batch(const uint8_t* gray, int n, int W, int H, int pitch, size_t frame_stride, uint32_t* col_out,
                                        uint32_t* row_out, void* ws, void* stream)
{
    if (!gray || !col_out || !row_out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n < 1 || n > 65535) { v3d_set_error("frame count %d outside [1, 65535]", n); return V3D_ERR_ARG; }
    if (W < 1 || H < 1) { v3d_set_error("profiles of a %dx%d plane", W, H); return V3D_ERR_ARG; }
    if (W > 8192 || H > 8192) { v3d_set_error("profiles of a %dx%d plane not supported (at most 8192 x 8192)", W, H); return V3D_ERR_UNSUPPORTED; }
    if (pitch < W) { v3d_set_error("pitch %d below the width %d", pitch, W); return V3D_ERR_ARG; }
    if (n > 1 && frame_stride < (size_t)H * (size_t)pitch) {
        v3d_set_error("frame stride %zu below the frame size %zu", frame_stride, (size_t)H * (size_t)pitch);
        return V3D_ERR_ARG;
    }
    if (((uintptr_t)ws & 15) || ((uintptr_t)col_out & 3) || ((uintptr_t)row_out & 3)) {
        v3d_set_error("ws not 16-byte aligned or an output not 4-byte aligned");
        return V3D_ERR_ARG;
    }
    const rg_plan p = rg_profile_plan(n, W, H);
    const bool vec = ((uintptr_t)gray & 15) == 0 && (pitch & 15) == 0 && (n == 1 || (frame_stride & 15) == 0);
    const dim3 grid(p.bands, n), block(RG_THREADS);
    uint32_t* part = static_cast<uint32_t*>(ws);
    if (vec) hipLaunchKernelGGL(k_rg_profiles<true>, grid, block, 0, (hipStream_t)stream, gray, W, H, (size_t)pitch, frame_stride, p.nseg, p.ny, p.L, part, row_out);
    else hipLaunchKernelGGL(k_rg_profiles<false>, grid, block, 0, (hipStream_t)stream, gray, W, H, (size_t)pitch, frame_stride, p.nseg, p.ny, p.L, part, row_out);
    V3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rg_colsum, dim3(v3d_cdiv(W, 256), n), dim3(256), 0, (hipStream_t)stream, part, W, p.bands, col_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- 2. match.  First launch: the exclusive prefix sums of both profiles of every frame into ws as u64 [K][na + 1 + nb + 1]
// (pre[i] = sum of P[k], k < i; pre[n] the total).  A thread owns 8 consecutive samples; the sums of their low and high 16-bit
// halves are scanned apart (8192 * 65535 < 2^29 each: block_excl_add_u32 holds them) and joined in 64 bits.  Second launch: one
// wavefront per (frame, candidate), a lane takes the difference pairs j = lane, lane + 64, ...; the six sums fold by butterfly
// (two's complement: the wrap-around adds are exact). ----
#define RG_ITEMS 8

__global__ __launch_bounds__(RG_THREADS) void k_rg_prefix(const uint32_t* __restrict__ prof_a, int na, const uint32_t* __restrict__ prof_b, int nb,
                                                          unsigned long long* __restrict__ pre_out)
{
    __shared__ uint32_t tot_lo[RG_WAVES], tot_hi[RG_WAVES];
    const int which = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = which ? nb : na;
    const uint32_t* P = (which ? prof_b : prof_a) + (size_t)f * n;
    unsigned long long* pre = pre_out + (size_t)f * (na + nb + 2) + (which ? na + 1 : 0);
    uint32_t v[RG_ITEMS], lo = 0u, hi = 0u;
#pragma unroll
    for (int i = 0; i < RG_ITEMS; i++) {
        const int x = tid * RG_ITEMS + i;
        v[i] = x < n ? P[x] : 0u;
        lo += v[i] & 0xFFFFu; hi += v[i] >> 16;
    }
    const excl_total el = block_excl_add_u32<RG_WAVES>(lo, lane, wave, tot_lo);
    const excl_total eh = block_excl_add_u32<RG_WAVES>(hi, lane, wave, tot_hi);
    unsigned long long s = (unsigned long long)el.excl + ((unsigned long long)eh.excl << 16);
#pragma unroll
    for (int i = 0; i < RG_ITEMS; i++) {
        const int x = tid * RG_ITEMS + i;
        if (x < n) pre[x] = s;
        s += v[i];
    }
    if (tid == 0) pre[n] = (unsigned long long)el.total + ((unsigned long long)eh.total << 16);
}

// I(p) = pre[i] * 65536 + f * P[i], P[n] read as 0; 0 <= p <= n * 65536
__device__ __forceinline__ unsigned long long rg_integral(const uint32_t* __restrict__ P, const unsigned long long* __restrict__ pre, int n, long long p)
{
    const int i = (int)(p >> 16);
    const unsigned long long f = (unsigned long long)(p & 65535);
    return (pre[i] << 16) + f * (i < n ? P[i] : 0u);
}
__device__ __forceinline__ long long rg_mean(const uint32_t* __restrict__ P, const unsigned long long* __restrict__ pre, int n, long long lo, long long hi)
{
    return (long long)((rg_integral(P, pre, n, hi) - rg_integral(P, pre, n, lo)) / (unsigned long long)(hi - lo));
}

__global__ __launch_bounds__(64) void k_rg_match(const uint32_t* __restrict__ prof_a, int na, const uint32_t* __restrict__ prof_b, int nb,
                                                 const long long* __restrict__ cand, int C, int bins,
                                                 const unsigned long long* __restrict__ pre_all, long long* __restrict__ out)
{
    const int c = blockIdx.x, f = blockIdx.y, lane = threadIdx.x;
    const long long a = cand[2 * (size_t)c], b = cand[2 * (size_t)c + 1];
    long long* rec = out + ((size_t)f * C + c) * 6;
    if (a < (1ll << 12) || a > (1ll << 20) || b < -(1ll << 29) || b > (1ll << 29)) {   // outside the domain: the in-band refusal
        if (lane < 6) rec[lane] = lane == 0 ? -1 : 0;
        return;
    }
    const uint32_t* A = prof_a + (size_t)f * na;
    const uint32_t* B = prof_b + (size_t)f * nb;
    const unsigned long long* preA = pre_all + (size_t)f * (na + nb + 2);
    const unsigned long long* preB = preA + na + 1;
    const long long lim = (long long)na << 16;
    const unsigned long long scale = (unsigned long long)nb << 16;
    unsigned long long np = 0, sa = 0, sb = 0, sab = 0, saa = 0, sbb = 0;
    for (int j = lane; j < bins - 1; j += 64) {
        const long long t0 = (long long)(((unsigned long long)j * scale) / (unsigned)bins);
        const long long t1 = (long long)(((unsigned long long)(j + 1) * scale) / (unsigned)bins);
        const long long t2 = (long long)(((unsigned long long)(j + 2) * scale) / (unsigned)bins);
        const long long s0 = ((a * t0) >> 16) + b, s1 = ((a * t1) >> 16) + b, s2 = ((a * t2) >> 16) + b;
        if (s0 < 0 || s2 > lim) continue;                           // s0 < s1 < s2: both bins lie inside the source
        const long long da = rg_mean(A, preA, na, s1, s2) - rg_mean(A, preA, na, s0, s1);
        const long long db = rg_mean(B, preB, nb, t1, t2) - rg_mean(B, preB, nb, t0, t1);
        const unsigned long long ua = (unsigned long long)da, ub = (unsigned long long)db;     // unsigned products: samples of 2^21 and
        np += 1; sa += ua; sb += ub;                                                           // above wrap, as the header says
        sab += ua * ub; saa += ua * ua; sbb += ub * ub;
    }
    np = wave_sum_u64(np); sa = wave_sum_u64(sa); sb = wave_sum_u64(sb);
    sab = wave_sum_u64(sab); saa = wave_sum_u64(saa); sbb = wave_sum_u64(sbb);
    if (lane == 0) {
        rec[0] = (long long)np; rec[1] = (long long)sa; rec[2] = (long long)sb;
        rec[3] = (long long)sab; rec[4] = (long long)saa; rec[5] = (long long)sbb;
    }
}

static bool rg_match_args_ok(int K, int na, int nb)
{
    return K >= 1 && K <= 4096 && na >= 1 && na <= 8192 && nb >= 1 && nb <= 8192;
}

extern "C" size_t v3d_profile_match_ws_bytes(int K, int na, int nb)
{
    if (!rg_match_args_ok(K, na, nb)) return 0;
    return (size_t)K * (size_t)(na + nb + 2) * sizeof(unsigned long long);
}

extern "C" int v3d_profile_match_scores(const uint32_t* prof_a, int na, const uint32_t* prof_b, int nb, int K, const int64_t* cand, int C,
                                        int bins, int64_t* out, void* ws, void* stream)
{
    if (!prof_a || !prof_b || !cand || !out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (K < 1 || K > 4096) { v3d_set_error("frame count %d outside [1, 4096]", K); return V3D_ERR_ARG; }
    if (C < 1 || C > 65535) { v3d_set_error("candidate count %d outside [1, 65535]", C); return V3D_ERR_ARG; }
    if (na < 1 || nb < 1) { v3d_set_error("profile lengths %d, %d", na, nb); return V3D_ERR_ARG; }
    if (na > 8192 || nb > 8192) { v3d_set_error("profile lengths %d, %d above 8192", na, nb); return V3D_ERR_UNSUPPORTED; }
    if (bins < 8 || bins > 1024 || nb < bins) { v3d_set_error("%d bins outside [8, 1024] or above the target's %d samples", bins, nb); return V3D_ERR_ARG; }
    if (((uintptr_t)ws & 15) || ((uintptr_t)cand & 7) || ((uintptr_t)out & 7) || ((uintptr_t)prof_a & 3) || ((uintptr_t)prof_b & 3)) {
        v3d_set_error("ws not 16-byte aligned, cand or out not 8-byte aligned or a profile not 4-byte aligned");
        return V3D_ERR_ARG;
    }
    unsigned long long* pre = static_cast<unsigned long long*>(ws);
    hipLaunchKernelGGL(k_rg_prefix, dim3(2, K), dim3(RG_THREADS), 0, (hipStream_t)stream, prof_a, na, prof_b, nb, pre);
    V3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rg_match, dim3(C, K), dim3(64), 0, (hipStream_t)stream, prof_a, na, prof_b, nb,
                       reinterpret_cast<const long long*>(cand), C, bins, pre, reinterpret_cast<long long*>(out));
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- 3. warp.  One workgroup per 1024 output pixels of a row: a thread takes four neighbours, grouped so that a whole group
// starts on an 8-byte boundary of `out` (rows are only 2-byte aligned: the first group of a row holds the 0 .. 3 pixels before
// the boundary) and leaves in one 8-byte store; partial groups store pixel by pixel. ----
__device__ __forceinline__ uint32_t rg_sample(int Ws, long long u, const uint16_t* __restrict__ row0,
                                              const uint16_t* __restrict__ row1, uint32_t fy, uint32_t fill)
{
    if (u < 0 || u > ((long long)(Ws - 1) << 16)) return fill;
    const int i0 = (int)(u >> 16), i1 = min(i0 + 1, Ws - 1);
    const uint32_t fx = (uint32_t)(u >> 8) & 255u;
    const uint32_t top = (256u - fx) * row0[i0] + fx * row0[i1], bot = (256u - fx) * row1[i0] + fx * row1[i1];
    return ((256u - fy) * top + fy * bot + 32768u) >> 16;
}

__global__ __launch_bounds__(256) void k_rg_warp(const uint16_t* __restrict__ src, int Ws, int Hs, size_t src_stride, long long ax, long long bx,
                                                 long long ay, long long by, uint32_t fill, uint16_t* __restrict__ out, int Wo, int Ho)
{
    const int y = blockIdx.y, f = blockIdx.z;
    uint16_t* orow = out + ((size_t)f * Ho + y) * Wo;
    const int lead = (int)((8u - ((uintptr_t)orow & 7u)) & 7u) >> 1;               // pixels before the row's first 8-byte boundary
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int xa = g == 0 ? 0 : lead + 4 * (g - 1), xb = min(g == 0 ? lead : xa + 4, Wo);
    if (xa >= xb) return;
    const long long v = ay * y + by;
    const bool row_in = v >= 0 && v <= ((long long)(Hs - 1) << 16);
    const int j0 = row_in ? (int)(v >> 16) : 0, j1 = min(j0 + 1, Hs - 1);
    const uint32_t fy = (uint32_t)(v >> 8) & 255u;
    const uint16_t* frame = src + (size_t)f * src_stride;
    const uint16_t* row0 = frame + (size_t)j0 * Ws;
    const uint16_t* row1 = frame + (size_t)j1 * Ws;
    uint32_t px[4];
#pragma unroll
    for (int i = 0; i < 4; i++)
        px[i] = (row_in && xa + i < xb) ? rg_sample(Ws, ax * (xa + i) + bx, row0, row1, fy, fill) : fill;
    if (xb - xa == 4 && g > 0) {
        *reinterpret_cast<uint2*>(orow + xa) = make_uint2(px[0] | (px[1] << 16), px[2] | (px[3] << 16));
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (xa + i < xb) orow[xa + i] = (uint16_t)px[i];
    }
}

extern "C" int v3d_warp_u16_batch(const uint16_t* src, int n, int Ws, int Hs, size_t src_stride, int64_t ax, int64_t bx, int64_t ay, int64_t by,
                                  uint16_t fill, uint16_t* out, int Wo, int Ho, void* stream)
{
    if (!src || !out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n < 1 || n > 65535) { v3d_set_error("frame count %d outside [1, 65535]", n); return V3D_ERR_ARG; }
    if (Ws < 1 || Hs < 1 || Wo < 1 || Ho < 1) { v3d_set_error("warp of %dx%d to %dx%d", Ws, Hs, Wo, Ho); return V3D_ERR_ARG; }
    if (Ws > 8192 || Wo > 8192 || Hs > 65535 || Ho > 65535) {
        v3d_set_error("warp of %dx%d to %dx%d not supported (widths up to 8192, heights up to 65535)", Ws, Hs, Wo, Ho);
        return V3D_ERR_UNSUPPORTED;
    }
    if (n > 1 && src_stride < (size_t)Ws * (size_t)Hs) {
        v3d_set_error("source stride %zu below the frame size %zu", src_stride, (size_t)Ws * (size_t)Hs);
        return V3D_ERR_ARG;
    }
    const int64_t lo = (int64_t)1 << 12, hi = (int64_t)1 << 20, bmax = (int64_t)1 << 40;
    if (ax < lo || ax > hi || ay < lo || ay > hi || bx < -bmax || bx > bmax || by < -bmax || by > bmax) {
        v3d_set_error("warp map outside 2^12 <= ax, ay <= 2^20, |bx|, |by| <= 2^40");
        return V3D_ERR_ARG;
    }
    if (((uintptr_t)src & 1) || ((uintptr_t)out & 1)) { v3d_set_error("a plane not 2-byte aligned"); return V3D_ERR_ARG; }
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + 2 * ((size_t)(n - 1) * src_stride + (size_t)Ws * Hs);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 2 * (size_t)n * Wo * Ho;
    if (s0 < o1 && o0 < s1) { v3d_set_error("out overlaps src"); return V3D_ERR_ARG; }
    const int groups = 1 + v3d_cdiv(Wo, 4);                         // the lead group and every group that may follow it
    hipLaunchKernelGGL(k_rg_warp, dim3(v3d_cdiv(groups, 256), Ho, n), dim3(256), 0, (hipStream_t)stream, src, Ws, Hs, src_stride,
                       (long long)ax, (long long)bx, (long long)ay, (long long)by, (uint32_t)fill, out, Wo, Ho);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
