// v3d_pre.hip -- the per-frame steps either side of the matcher:
//   depth.py:250-268 split_sbs_frame (cv2.resize INTER_LANCZOS4 horizontal x2 "unsqueeze"), and the same for a top-bottom frame
//   (vertical x2, k_split_tb),
//   depth.py:274-275 + 337-338 cvtColor (BGR->RGB->GRAY), depth.py:341/374 (/16, clamp),
//   and the rounding of the 4K depth to the PNG sink's 16-bit sample.
// (depth.py:397-406 save_depth_map, min-max -> uint16, lives in v3d_range.hip with the other range entries.)
// All pure streaming kernels: one read of the input, one write of the output.
#include "v3d_common.h"
#include <math.h>

struct LanczosTaps { short t[2][8]; };   // [0]: even output columns (fx = 0.75), [1]: odd (fx = 0.25)

// host: the 8 int16 taps cv::resize builds for fractional offset fx (coefficients scaled by 2^11,
// rounded half-to-even like cvRound)
static void lanczos4_taps_host(float x, short* taps)
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[8][2] = { {1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45} };
    const double PI = 3.1415926535897932384626433832795;
    float c[8], sum = 0.f;
    const double y0 = -(x + 3) * PI * 0.25, s0 = sin(y0), c0 = cos(y0);
    for (int i = 0; i < 8; i++) {
        const float yi = (x + 3 - i);
        if (fabsf(yi) >= 1e-6f) { const double y = -yi * PI * 0.25; c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)); }
        else c[i] = 1e30f;
        sum += c[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) {
        long r = lrintf(c[i] * sum * 2048.f);
        taps[i] = (short)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
    }
}

__device__ __forceinline__ int gray_of(int b, int g, int r) { return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15; }

// Without unsqueeze one thread = one output pixel of one eye; a block covers 256 output pixels of one row.  The source span
// (256 + 8 BGR pixels when unsqueezing, 256 otherwise) is staged through LDS with coalesced dword loads:
// per-tap byte loads at a 3-byte stride straight from HBM ran at 0.3 TB/s.
// GRAY: write luma only; else write the BGR triple.
#ifndef SBS_ROWS
#define SBS_ROWS 8
#endif
//    // rows per workgroup: the per-row work is tiny, one workgroup per row was bound by dispatch
// Unsqueezing, a thread computes the output PAIR (2m, 2m+1): the two 8-tap windows (source pixels m-4..m+3 with the
// frac-0.75 taps, m-3..m+4 with the frac-0.25 taps) overlap in 7 of 8 pixels; a block covers 512 output pixels of one eye row.
//  - The 27 bytes of the 9 pixels come out of LDS as the 8 aligned dwords that cover them, shifted into place with
//    v_alignbit_b32 by the lane's byte phase.  The dwords reach at most 7 bytes past the staged span: inside sRow, and no
//    selector below names those bytes.
//  - One v_perm_b32 makes the int16 pair (pixel k, pixel k+1) of a channel; the 8-tap sum of an output is four
//    v_dot2_i32_i16 of such pairs with the packed taps, the first accumulating onto the rounding constant.  Pixels are 0..255
//    and the taps int16, so the i32 sum is exact: the same integer as eight multiply-adds.
//  - The pair leaves as 16-bit words where the plane starts on an even address (W is even: then every row and every pair does).
// (Two pairs per thread, 2m .. 2m+3 from 10 pixels, share the pairs (1,2) .. (7,8) between outputs 2m+1 and 2m+2 and store
//  dwords: 73 instead of 86 vector instructions per pair, but a row then needs 128 lanes.  With the waves taking rows in
//  turn it measured 2 % slower than one pair per thread -- DESIGN.md, "k_split_sbs: packed dot products".)

// the bytes of {hi, lo} that sel names, as v_perm_b32 does for the selectors used here: 0..3 a byte of lo, 4..7 a byte of hi,
// 0x0c the constant 0.  (The host definitions serve the builds of this file that have no device pass.)
__device__ __forceinline__ uint32_t split_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t v = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t b = (sel >> (8 * i)) & 255u;
        if (b < 8) r |= ((uint32_t)(v >> (8 * b)) & 255u) << (8 * i);
    }
    return r;
#endif
}
// acc + a.lo * b.lo + a.hi * b.hi on int16 halves, no saturation (v_dot2_i32_i16)
__device__ __forceinline__ int split_dot2(uint32_t a, uint32_t b, int acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short split_s2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(split_s2, a), __builtin_bit_cast(split_s2, b), acc, false);
#else
    return acc + (int)(int16_t)(a & 0xFFFFu) * (int)(int16_t)(b & 0xFFFFu) + (int)(int16_t)(a >> 16) * (int)(int16_t)(b >> 16);
#endif
}

template <bool GRAY>
__global__ __launch_bounds__(256) void k_split_sbs(const uint8_t* __restrict__ sbs, int W, int H, int pitch, int unsqueeze,
                                                   LanczosTaps taps, uint8_t* __restrict__ outL, uint8_t* __restrict__ outR,
                                                   size_t in_stride)
{
    __shared__ __attribute__((aligned(4))) uint8_t sRow[2][(256 + 8) * 3 + 16];
    const int hw = W >> 1, ow = unsqueeze ? W : hw;
    const int t = threadIdx.x;
    const int xb = blockIdx.x * (unsqueeze ? 512 : 256), eye = blockIdx.z & 1, f = blockIdx.z >> 1;
    const int ya = blockIdx.y * SBS_ROWS, yb = min(ya + SBS_ROWS, H);
    sbs += (size_t)f * in_stride;
    const size_t ostride = (size_t)ow * H * (GRAY ? 1 : 3);
    outL += f * ostride; outR += f * ostride;
    uint8_t* out = eye ? outR : outL;

    // source pixels [s0, s0 + ns) of the half row are needed by this block
    const int s0 = unsqueeze ? (xb >> 1) - 4 : xb;
    const int ns = unsqueeze ? 256 + 8 : 256;
    const bool interior = s0 >= 0 && (s0 + ns < hw || (eye == 0 && s0 + ns <= hw));
    uint32_t tpk[2][4];                                             // taps (2i, 2i+1) of either phase as one int16 pair
#pragma unroll
    for (int i = 0; i < 4; i++) {
        tpk[0][i] = (uint32_t)(uint16_t)taps.t[0][2 * i] | (uint32_t)(uint16_t)taps.t[0][2 * i + 1] << 16;
        tpk[1][i] = (uint32_t)(uint16_t)taps.t[1][2 * i] | (uint32_t)(uint16_t)taps.t[1][2 * i + 1] << 16;
    }
    // an unsqueezed pair leaves as 16-bit words when the plane starts on an even address and its rows are even: then every row
    // starts on one, and every pair (x is even) with it; bytes otherwise
    constexpr int CH = GRAY ? 1 : 3;
    const bool wide = ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)ow) & 1) == 0;

    // Staging plan of this thread, the same for every row of the band: interior blocks copy ONE aligned dword of the
    // span (the <= 3 bytes of over-read stay inside the image row); edge blocks copy up to four bytes from clamped
    // pixels (replicated border).  The plan's loads for row y+1 are issued before row y is computed: a row is ~140
    // instructions, a load ~1.5 us -- fetched at the top of its own row, every row waited for its bytes.
    // (Dword copies need a row-invariant alignment: pitch a multiple of 4.  A half row that starts at the row's first
    //  byte on an unaligned address would be read from up to 3 bytes BEFORE the row -- before the caller's buffer for
    //  row 0 of frame 0: such blocks take the byte plan.)
    const uint8_t* col0 = sbs + (size_t)eye * hw * 3;               // this eye's half row starts here in every row
    const uintptr_t a = reinterpret_cast<uintptr_t>(col0 + (size_t)max(s0, 0) * 3);
    const bool head_unaligned = (eye | s0) == 0 && (reinterpret_cast<uintptr_t>(col0) & 3) != 0;
    const bool fast = interior && !head_unaligned && (pitch & 3) == 0;
    const int soff = fast ? (int)(a & 3) : 0;                       // byte offset of pixel s0 inside sR
    const int nd = (soff + ns * 3 + 3) >> 2;
    int boff[4];                                                    // byte plan: source offsets inside the half row
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int i = min(t + 256 * k, ns * 3 - 1), px = i / 3, c = i - px * 3;
        boff[k] = min(max(s0 + px, 0), hw - 1) * 3 + c;
    }
    uint32_t pre[4] = { 0u, 0u, 0u, 0u };
    auto load_row = [&](int y) {
        const uint8_t* row = col0 + (size_t)y * pitch;
        if (fast) {
            if (t < nd) pre[0] = reinterpret_cast<const uint32_t*>((reinterpret_cast<uintptr_t>(row + (size_t)s0 * 3)) & ~(uintptr_t)3)[t];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) pre[k] = row[boff[k]];
        }
    };
    load_row(ya);
    for (int y = ya; y < yb; y++) {
        uint8_t* sR = sRow[y & 1];                                  // double-buffered: one barrier per row
        if (fast) { if (t < nd) reinterpret_cast<uint32_t*>(sR)[t] = pre[0]; }
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (t + 256 * k < ns * 3) sR[t + 256 * k] = (uint8_t)pre[k];
        }
        __syncthreads();
        if (y + 1 < yb) load_row(y + 1);                            // flies while this row is computed
        if (unsqueeze) {
            // source phase: fx = (x + 0.5) * 0.5 - 0.5 -> even x = 2m: sx = m - 1, frac 0.75; odd x = 2m + 1: sx = m, frac 0.25
            const int x = xb + 2 * t;                               // even member of the pair; m = x / 2 = s0 + 4 + t
            if (x >= ow) continue;
            constexpr int NW = 7;                                   // the window, pixels m-4 .. m+4, is 27 bytes: 7 dwords once shifted
            const int b0 = soff + 3 * t;                            // byte of pixel m - 4, <= 768: the 8 dwords end at byte 799 or below
            const uint32_t* dw = reinterpret_cast<const uint32_t*>(sR + (b0 & ~3));
            const uint32_t sh = (uint32_t)(b0 & 3) * 8;
            uint32_t d[NW + 1], w[NW];
#pragma unroll
            for (int i = 0; i <= NW; i++) d[i] = dw[i];
#pragma unroll
            for (int i = 0; i < NW; i++) w[i] = alignbit(d[i + 1], d[i], sh);
            uint32_t pr[8][3];                                      // [k][c]: channel c of window pixels (k, k+1), bytes 3k+c and 3k+3+c
#pragma unroll
            for (int k = 0; k < 8; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int j = 3 * k + c, a = j >> 2;            // a + 1 <= 6: byte 3k+3+c <= 26
                    pr[k][c] = split_perm(w[a + 1], w[a], 0x0c000c00u | (uint32_t)(j - 4 * a) | (uint32_t)(j + 3 - 4 * a) << 16);
                }
            uint32_t ob[2 * CH];                                    // the pair's output bytes in order
#pragma unroll
            for (int n = 0; n < 2; n++) {
                int v[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    // vertical pass is the identity tap (2048): (a * 2048 + 2^21) >> 22 == (a + 2^10) >> 11 exactly (floor
                    // of the same rational), so the descale stays in 32 bits; saturate to u8
                    int acc = 1024;
#pragma unroll
                    for (int i = 0; i < 4; i++) acc = split_dot2(pr[n + 2 * i][c], tpk[n][i], acc);
                    v[c] = min(max(acc >> 11, 0), 255);
                }
#pragma unroll
                for (int c = 0; c < CH; c++) ob[n * CH + c] = (uint32_t)(GRAY ? gray_of(v[0], v[1], v[2]) : v[c]);
            }
            uint8_t* o = out + ((size_t)y * ow + x) * CH;
            if (wide) {                                             // uniform; ow and x are even: both outputs exist
#pragma unroll
                for (int u = 0; u < CH; u++) reinterpret_cast<uint16_t*>(o)[u] = (uint16_t)(ob[2 * u] | ob[2 * u + 1] << 8);
            } else {
                const int nb = min(2, ow - x) * CH;
#pragma unroll
                for (int i = 0; i < 2 * CH; i++) if (i < nb) o[i] = (uint8_t)ob[i];
            }
        } else {
            const int x = xb + t;
            if (x >= ow) continue;
            const uint8_t* p = sR + soff + t * 3;
            const int b = p[0], g = p[1], r = p[2];
            if (GRAY) out[(size_t)y * ow + x] = (uint8_t)gray_of(b, g, r);
            else { uint8_t* o = out + ((size_t)y * ow + x) * 3; o[0] = (uint8_t)b; o[1] = (uint8_t)g; o[2] = (uint8_t)r; }
        }
    }
}

static int split_common(const uint8_t* sbs, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, bool gray, int n, size_t in_stride, hipStream_t st)
{
    if (n < 1) { v3d_set_error("bad batch"); return V3D_ERR_ARG; }
    if (!sbs || !L || !R) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (W % 2 != 0) { v3d_set_error("SBS frame width must be even"); return V3D_ERR_ARG; }
    if (W < 2 || H < 1 || pitch < W * 3) { v3d_set_error("bad SBS geometry %dx%d pitch %d", W, H, pitch); return V3D_ERR_ARG; }
    if (n > 1 && in_stride < (size_t)H * pitch) { v3d_set_error("frame stride %zu below the frame size %zu (H * pitch)", in_stride, (size_t)H * pitch); return V3D_ERR_ARG; }
    LanczosTaps taps;
    lanczos4_taps_host(0.75f, taps.t[0]);
    lanczos4_taps_host(0.25f, taps.t[1]);
    const int ow = unsqueeze ? W : W / 2;
    if (gray) hipLaunchKernelGGL(k_split_sbs<true>, dim3(v3d_cdiv(ow, unsqueeze ? 512 : 256), v3d_cdiv(H, SBS_ROWS), 2 * n), dim3(256), 0, st, sbs, W, H, pitch, unsqueeze, taps, L, R, in_stride);
    else hipLaunchKernelGGL(k_split_sbs<false>, dim3(v3d_cdiv(ow, unsqueeze ? 512 : 256), v3d_cdiv(H, SBS_ROWS), 2 * n), dim3(256), 0, st, sbs, W, H, pitch, unsqueeze, taps, L, R, in_stride);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_sbs_to_gray(const uint8_t* sbs, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_common(sbs, W, H, pitch, unsqueeze, L, R, true, 1, 0, (hipStream_t)stream);
}
extern "C" int v3d_split_sbs(const uint8_t* sbs, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_common(sbs, W, H, pitch, unsqueeze, L, R, false, 1, 0, (hipStream_t)stream);
}
// n frames: frame f at sbs + f*frame_stride (bytes); outputs packed [n][H][outW]
extern "C" int v3d_sbs_to_gray_batch(const uint8_t* sbs, int n, int W, int H, int pitch, size_t frame_stride, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_common(sbs, W, H, pitch, unsqueeze, L, R, true, n, frame_stride, (hipStream_t)stream);
}

// ---- top-bottom input: eye e is rows e*Hh .. e*Hh + Hh - 1 of the frame, Hh = H / 2 (left eye on top) ----
// The unsqueeze is the same resize with the axes swapped: the 8 taps run DOWN a column, so they act on bytes independently --
// no 3-byte stride, no LDS.  A thread owns 4 pixels (12 bytes, three dwords) of one eye and marches down a band of TB_BAND
// source rows with the nine rows m-4 .. m+4 in registers: output rows 2m (frac 0.75, rows m-4 .. m+3) and 2m+1 (frac 0.25,
// rows m-3 .. m+4) share seven of their eight input rows.  Rows are clamped to the eye: no tap of the top eye's last rows
// reads the bottom eye's first ones.  A band re-reads 8 halo rows (13 % at 60); 540 = 9 * 60, so a 1080p eye has no ragged
// band, and 2 eyes * 34 frames * 9 bands * 2 column blocks = 1224 workgroups fill 256 CUs at 4.8 waves per SIMD.
#ifndef TB_BAND
#define TB_BAND 60
#endif
template <bool GRAY>
__global__ __launch_bounds__(256) void k_split_tb(const uint8_t* __restrict__ tb, int W, int H, int pitch, int unsqueeze,
                                                  LanczosTaps taps, uint8_t* __restrict__ outL, uint8_t* __restrict__ outR,
                                                  size_t in_stride)
{
    const int Hh = H >> 1, oh = unsqueeze ? H : Hh;
    const int x = (blockIdx.x * 256 + threadIdx.x) * 4;             // first of this thread's pixels
    if (x >= W) return;
    const int np = min(4, W - x);                                   // < 4 in the last group of a row when W % 4 != 0
    const int eye = blockIdx.z & 1, f = blockIdx.z >> 1;
    const int ma = blockIdx.y * TB_BAND, mb = min(ma + TB_BAND, Hh);
    const uint8_t* src = tb + (size_t)f * in_stride + (size_t)eye * Hh * pitch + (size_t)x * 3;   // this thread's bytes of eye row 0
    uint8_t* out = (eye ? outR : outL) + (size_t)f * ((size_t)W * oh * (GRAY ? 1 : 3));
    int tp0[8], tp1[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { tp0[k] = taps.t[0][k]; tp1[k] = taps.t[1][k]; }

    // Load plan, the same for every row: three dwords when all four pixels exist and every row's copy of them is aligned (pitch a
    // multiple of 4 and an aligned start; 12 bytes per thread keep the alignment along the row).  Otherwise twelve byte loads, the
    // offsets clamped to the row's payload: nothing in front of the frame, in the pitch padding or behind the last row is read.
    const bool fast = np == 4 && (pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    const int last = np * 3 - 1;
    auto load_row = [&](int y, uint32_t* d) {
        const uint8_t* row = src + (size_t)y * pitch;
        if (fast) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(row);
            d[0] = p[0]; d[1] = p[1]; d[2] = p[2];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++)
                d[k] = (uint32_t)row[min(4 * k, last)] | (uint32_t)row[min(4 * k + 1, last)] << 8 |
                       (uint32_t)row[min(4 * k + 2, last)] << 16 | (uint32_t)row[min(4 * k + 3, last)] << 24;
        }
    };
    // one output row of this thread: v = its 12 channel values (b, g, r of four pixels).  Dword stores when the group is whole
    // and its first output byte is aligned (a dense output row of W or 3 W bytes may move the alignment from row to row)
    auto emit = [&](int yo, const int* v) {
        if (GRAY) {
            uint8_t* o = out + (size_t)yo * W + x;
            int g[4];
#pragma unroll
            for (int j = 0; j < 4; j++) g[j] = gray_of(v[3 * j], v[3 * j + 1], v[3 * j + 2]);
            if (np == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0)
                *reinterpret_cast<uint32_t*>(o) = (uint32_t)g[0] | (uint32_t)g[1] << 8 | (uint32_t)g[2] << 16 | (uint32_t)g[3] << 24;
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) if (j < np) o[j] = (uint8_t)g[j];
            }
        } else {
            uint8_t* o = out + ((size_t)yo * W + x) * 3;
            if (np == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    reinterpret_cast<uint32_t*>(o)[k] = (uint32_t)v[4 * k] | (uint32_t)v[4 * k + 1] << 8 | (uint32_t)v[4 * k + 2] << 16 | (uint32_t)v[4 * k + 3] << 24;
            } else {
#pragma unroll
                for (int i = 0; i < 12; i++) if (i <= last) o[i] = (uint8_t)v[i];
            }
        }
    };

    uint32_t pre[3] = { 0u, 0u, 0u };
    if (!unsqueeze) {                                               // the eye's rows as they are
        load_row(ma, pre);
        for (int m = ma; m < mb; m++) {
            const uint32_t cur[3] = { pre[0], pre[1], pre[2] };
            if (m + 1 < mb) load_row(m + 1, pre);                   // flies while this row is computed
            int v[12];
#pragma unroll
            for (int i = 0; i < 12; i++) v[i] = (cur[i >> 2] >> (8 * (i & 3))) & 255;
            emit(m, v);
        }
        return;
    }
    uint32_t r[9][3];                                               // rows m-4 .. m+4, clamped to the eye
#pragma unroll
    for (int k = 0; k < 9; k++) load_row(min(max(ma - 4 + k, 0), Hh - 1), r[k]);
    for (int m = ma; m < mb; m++) {
        // row m+5 is fetched before rows 2m and 2m+1 are computed, for k_split_sbs's reason: fetched where it is needed, every
        // step waits for its bytes
        if (m + 1 < mb) load_row(min(m + 5, Hh - 1), pre);
        int v0[12], v1[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            int a0 = 0, a1 = 0;
#pragma unroll
            for (int k = 0; k < 9; k++) {
                const int s = (r[k][i >> 2] >> (8 * (i & 3))) & 255;
                if (k < 8) a0 += s * tp0[k];
                if (k > 0) a1 += s * tp1[k - 1];
            }
            // the horizontal pass is the identity tap (2048): (a * 2048 + 2^21) >> 22 == (a + 2^10) >> 11, as in k_split_sbs
            v0[i] = min(max((a0 + 1024) >> 11, 0), 255);
            v1[i] = min(max((a1 + 1024) >> 11, 0), 255);
        }
        emit(2 * m, v0);
        emit(2 * m + 1, v1);
#pragma unroll
        for (int k = 0; k < 8; k++) { r[k][0] = r[k + 1][0]; r[k][1] = r[k + 1][1]; r[k][2] = r[k + 1][2]; }
        r[8][0] = pre[0]; r[8][1] = pre[1]; r[8][2] = pre[2];
    }
}

static int split_tb_common(const uint8_t* tb, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, bool gray, int n, size_t in_stride, hipStream_t st)
{
    if (n < 1) { v3d_set_error("bad batch"); return V3D_ERR_ARG; }
    if (!tb || !L || !R) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (H % 2 != 0) { v3d_set_error("top-bottom frame height must be even"); return V3D_ERR_ARG; }
    if (W < 1 || H < 2 || pitch < W * 3) { v3d_set_error("bad top-bottom geometry %dx%d pitch %d", W, H, pitch); return V3D_ERR_ARG; }
    if (n > 1 && in_stride < (size_t)H * pitch) { v3d_set_error("frame stride %zu below the frame size %zu (H * pitch)", in_stride, (size_t)H * pitch); return V3D_ERR_ARG; }
    LanczosTaps taps;
    lanczos4_taps_host(0.75f, taps.t[0]);
    lanczos4_taps_host(0.25f, taps.t[1]);
    const dim3 grid(v3d_cdiv(v3d_cdiv(W, 4), 256), v3d_cdiv(H / 2, TB_BAND), 2 * n);
    if (gray) hipLaunchKernelGGL(k_split_tb<true>, grid, dim3(256), 0, st, tb, W, H, pitch, unsqueeze, taps, L, R, in_stride);
    else hipLaunchKernelGGL(k_split_tb<false>, grid, dim3(256), 0, st, tb, W, H, pitch, unsqueeze, taps, L, R, in_stride);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_tb_to_gray(const uint8_t* tb, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_tb_common(tb, W, H, pitch, unsqueeze, L, R, true, 1, 0, (hipStream_t)stream);
}
extern "C" int v3d_split_tb(const uint8_t* tb, int W, int H, int pitch, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_tb_common(tb, W, H, pitch, unsqueeze, L, R, false, 1, 0, (hipStream_t)stream);
}
// n frames: frame f at tb + f*frame_stride (bytes); outputs packed [n][outH][W]
extern "C" int v3d_tb_to_gray_batch(const uint8_t* tb, int n, int W, int H, int pitch, size_t frame_stride, int unsqueeze, uint8_t* L, uint8_t* R, void* stream)
{
    return split_tb_common(tb, W, H, pitch, unsqueeze, L, R, true, n, frame_stride, (hipStream_t)stream);
}

__global__ __launch_bounds__(256) void k_bgr_to_gray(const uint8_t* __restrict__ bgr, size_t n, uint8_t* __restrict__ gray)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        gray[i] = (uint8_t)gray_of(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2]);
}
extern "C" int v3d_bgr_to_gray(const uint8_t* bgr, size_t n, uint8_t* gray, void* stream)
{
    if (!bgr || !gray) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n == 0) return V3D_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_bgr_to_gray, dim3(blocks), dim3(256), 0, (hipStream_t)stream, bgr, n, gray);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

__global__ __launch_bounds__(256) void k_disp_to_depth(const int16_t* __restrict__ d, size_t n, float* __restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float f = (float)d[i] / 16.0f;
        out[i] = f <= 0.f ? 0.f : f;
    }
}
extern "C" int v3d_disp_to_depth(const int16_t* disp16, size_t n, float* out, void* stream)
{
    if (!disp16 || !out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n == 0) return V3D_OK;
    const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    hipLaunchKernelGGL(k_disp_to_depth, dim3(blocks), dim3(256), 0, (hipStream_t)stream, disp16, n, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- 4K depth -> the 16-bit sample of the PNG sink: v3d_rint_u16 (v3d_depth_math.h) ----
__global__ __launch_bounds__(256) void k_round_u16(const float* __restrict__ d, size_t n, uint16_t* __restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = v3d_rint_u16(d[i]);
}
extern "C" int v3d_round_to_u16(const float* depth, size_t n, uint16_t* out, void* stream)
{
    if (!depth || !out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n == 0) return V3D_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(k_round_u16, dim3(blocks), dim3(256), 0, (hipStream_t)stream, depth, n, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
