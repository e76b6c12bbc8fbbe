// v3d_fuse.hip -- the rendered eye fused with the film's own stored eye: the low band from the stored eye, the detail above its
// resolution from the render (contract in include/v3d_hip.h; NumPy restatement in tests/fuse_ref.py; DESIGN.md section 4,
// "Source-fused right eye").
//   v3d_fuse_eye_source_batch   out = clamp(E - LP(E) + P, 0, 255), in place
// E is the eye as rendered, P the bilinear sample of v3d_render_stereo_source_batch's contract (the arithmetic is restated here:
// v3d_stereo.hip's and v3d_verify.hip's kernels are pinned and stay as they are), LP(E) the same bilinear sample taken from M, the
// means of E over the targets nearest to every stored sample.  Every number is an integer, so no order of evaluation can change a
// bit.  The entry neither synchronises nor allocates.
//
// Two launches, because the entry works in place: k_fuse_means reads the whole eye into M before k_fuse_apply writes any of it.
//   k_fuse_means   a workgroup owns FU_S samples of one sample row.  Their footprint is a run of target columns by a run of target
//                  rows; a thread owns a column of it (the lanes of a wave read 192 contiguous bytes of a row), sums it down the
//                  rows in registers and adds the three sums to its sample's bin in LDS once.  Under the clamps the footprint of
//                  a first or last sample has no bound but the image, hence the strided column loop, the 64-bit bins and the
//                  row sums flushed every FU_FLUSH rows.
//   k_fuse_apply   a thread owns FU_RUN consecutive targets of a row: their 12 bytes as three loads and three stores where the
//                  run is whole, and per target four taps of the stored eye and four of M, every pixel as its own three bytes.
#include <string.h>
#include "v3d_common.h"

#define FU_MAX_W 8192          // the render entries' bound on a row and on an eye
#define FU_S 64                // samples of a sample row per workgroup item (k_fuse_means)
#define FU_CHUNK 4             // rows whose loads a thread has in flight together
#define FU_FLUSH (1 << 20)     // rows a 32-bit column sum takes before it goes into the 64-bit one (255 * 2^20 < 2^32)
#define FU_RUN 4               // consecutive targets per thread (k_fuse_apply)
#define FU_LAUNCH_BLOCKS 2048  // workgroups per launch aimed at (8 per CU)
#define FU_FLOOR_BLOCKS 8      // per frame at least

struct FuArgs {
    uint8_t* eye;
    size_t eye_stride;                                         // bytes between frames
    const uint8_t* sbs;                                        // first byte of the sampled eye's half of row 0
    size_t sbs_stride;
    uint8_t* mean;                                             // M: [n][Hs][We][3], written for the populated range only
    size_t mean_stride;
    int eye_pitch, n, W, H, We, Hs, pitch;
    int ilo, ihi, jlo, jhi;                                    // the populated range: the nearest samples of the first and last target
    int chunks;                                                // groups of FU_S samples across [ilo, ihi]
    int xblocks;                                               // workgroups across a row of targets (k_fuse_apply)
    long long mean_items, apply_items;                         // per frame
    long long ax, bx, ay, by;
};

// a BGR pixel at p as 0x00RRGGBB: its three bytes and no other
V3D_HD static inline uint32_t fu_pixel(const uint8_t* p)
{
    uint16_t lo;
    memcpy(&lo, p, 2);
    return (uint32_t)lo | (uint32_t)p[2] << 16;
}

// four bytes at any address
V3D_HD static inline uint32_t fu_load4(const uint8_t* p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// an eye pixel read once: with a pixel behind it in its row (more), one 4-byte load whose fourth byte is dropped
V3D_HD static inline uint32_t fu_eye_pixel(const uint8_t* p, bool more)
{
    return more ? fu_load4(p) & 0xFFFFFFu : fu_pixel(p);
}

// the Q16 coordinate of target t on an axis of Ns samples, clamped to them
V3D_HD static inline long long fu_coord(long long a, long long b, int t, int Ns)
{
    const long long m = (long long)(Ns - 1) << 16, l = a * t + b;
    return l < 0 ? 0 : l > m ? m : l;
}

// the sample nearest to target t
V3D_HD static inline int fu_near(long long a, long long b, int t, int Ns)
{
    return (int)((fu_coord(a, b, t, Ns) + 32768) >> 16);
}

// the first of the Nd targets whose nearest sample is i or above, Nd if there is none.  lo, hi: the nearest samples of targets 0
// and Nd - 1.  For lo < i <= hi the clamps cannot decide (0 < (i << 16) - 32768 <= the upper clamp), so near(t) >= i iff
// a t + b >= (i << 16) - 32768, whose right side minus b is positive: near(0) < i says so
V3D_HD static inline int fu_first(int i, long long a, long long b, int lo, int hi, int Nd)
{
    if (i <= lo) return 0;
    if (i > hi) return Nd;
    const long long t = ((((long long)i << 16) - 32768 - b) + a - 1) / a;
    return t < Nd ? (int)t : Nd;
}

// the bilinear sample of four packed taps (a: column i0, b: column i1; 0: row j0, 1: row j1): the source entry's arithmetic
V3D_HD static inline uint32_t fu_blend(uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, int fx, int fy)
{
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const uint32_t top = (uint32_t)(256 - fx) * (a0 >> s & 255u) + (uint32_t)fx * (b0 >> s & 255u);
        const uint32_t bot = (uint32_t)(256 - fx) * (a1 >> s & 255u) + (uint32_t)fx * (b1 >> s & 255u);
        c |= (((uint32_t)(256 - fy) * top + (uint32_t)fy * bot + 32768u) >> 16) << s;
    }
    return c;
}

// clamp(e - lp + p, 0, 255) per channel of three packed pixels
V3D_HD static inline uint32_t fu_fuse(uint32_t e, uint32_t lp, uint32_t p)
{
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const int v = (int)(e >> s & 255u) - (int)(lp >> s & 255u) + (int)(p >> s & 255u);
        c |= (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v) << s;
    }
    return c;
}

// grid (workgroups of a frame, frames), both walked with the grid's stride.  An item: the samples [i0, i1) of sample row j
__global__ __launch_bounds__(256) void k_fuse_means(const FuArgs A)
{
    __shared__ unsigned long long sum[FU_S][3];
    __shared__ uint32_t cnt[FU_S];                             // target columns per sample
    const int tid = threadIdx.x;
    for (int f = blockIdx.y; f < A.n; f += gridDim.y) {
        const uint8_t* eye = A.eye + (size_t)f * A.eye_stride;
        uint8_t* mean = A.mean + (size_t)f * A.mean_stride;
        for (long long item = blockIdx.x; item < A.mean_items; item += gridDim.x) {
            const int j = A.jlo + (int)(item / A.chunks), i0 = A.ilo + (int)(item % A.chunks) * FU_S;
            const int i1 = min(i0 + FU_S, A.ihi + 1);
            const int ya = fu_first(j, A.ay, A.by, A.jlo, A.jhi, A.H), yz = fu_first(j + 1, A.ay, A.by, A.jlo, A.jhi, A.H);
            const int ta = fu_first(i0, A.ax, A.bx, A.ilo, A.ihi, A.W), tz = fu_first(i1, A.ax, A.bx, A.ilo, A.ihi, A.W);
            if (tid < FU_S) { sum[tid][0] = sum[tid][1] = sum[tid][2] = 0ull; cnt[tid] = 0u; }
            __syncthreads();
            for (int t = ta + tid; t < tz; t += 256) {
                const int bin = fu_near(A.ax, A.bx, t, A.We) - i0;
                const bool more = t + 1 < A.W;
                const uint8_t* col = eye + 3 * (size_t)t;
                unsigned long long s0 = 0, s1 = 0, s2 = 0;
                for (int yb = ya; yb < yz;) {
                    const int ye = yz - yb > FU_FLUSH ? yb + FU_FLUSH : yz;
                    uint32_t c0 = 0, c1 = 0, c2 = 0;
                    for (int yc = yb; yc < ye; yc += FU_CHUNK) {
                        uint32_t e[FU_CHUNK] = {};
#pragma unroll
                        for (int k = 0; k < FU_CHUNK; ++k)
                            if (yc + k < ye) e[k] = fu_eye_pixel(col + (size_t)(yc + k) * (size_t)A.eye_pitch, more);
#pragma unroll
                        for (int k = 0; k < FU_CHUNK; ++k) { c0 += e[k] & 255u; c1 += e[k] >> 8 & 255u; c2 += e[k] >> 16; }
                    }
                    s0 += c0; s1 += c1; s2 += c2;
                    yb = ye;
                }
                atomicAdd(&sum[bin][0], s0);
                atomicAdd(&sum[bin][1], s1);
                atomicAdd(&sum[bin][2], s2);
                atomicAdd(&cnt[bin], 1u);
            }
            __syncthreads();
            if (tid < 3 * (i1 - i0)) {
                const int k = tid / 3, c = tid - 3 * k;
                const unsigned long long N = (unsigned long long)cnt[k] * (unsigned long long)(yz - ya), v = 2 * sum[k][c] + N;
                if (N) {                                       // every sample of the populated range owns a target: always
                    const uint32_t m = (v >> 32) == 0 ? (uint32_t)v / (uint32_t)(2 * N) : (uint32_t)(v / (2 * N));
                    mean[((size_t)j * (size_t)A.We + (size_t)(i0 + k)) * 3 + c] = (uint8_t)m;
                }
            }
            __syncthreads();                                   // the next item's sums come into the same words
        }
    }
}

// grid (workgroups of a frame, frames), both walked with the grid's stride.  An item: 256 runs of FU_RUN targets of one row
__global__ __launch_bounds__(256) void k_fuse_apply(const FuArgs A)
{
    for (int f = blockIdx.y; f < A.n; f += gridDim.y) {
        uint8_t* eye = A.eye + (size_t)f * A.eye_stride;
        const uint8_t* sbs = A.sbs + (size_t)f * A.sbs_stride;
        const uint8_t* mean = A.mean + (size_t)f * A.mean_stride;
        for (long long item = blockIdx.x; item < A.apply_items; item += gridDim.x) {
            const int y = (int)(item / A.xblocks), t0 = ((int)(item % A.xblocks) * 256 + (int)threadIdx.x) * FU_RUN;
            if (t0 >= A.W) continue;
            const int cnt = min(FU_RUN, A.W - t0);
            // the row's taps: v is 64 bits wide (Hs has no bound but int's)
            const long long v = fu_coord(A.ay, A.by, y, A.Hs);
            const int j0 = (int)(v >> 16), j1 = min(j0 + 1, A.Hs - 1), fy = (int)(v >> 8) & 255;
            const uint8_t* s0 = sbs + (size_t)j0 * (size_t)A.pitch;
            const uint8_t* s1 = sbs + (size_t)j1 * (size_t)A.pitch;
            const uint8_t* m0 = mean + (size_t)min(max(j0, A.jlo), A.jhi) * (size_t)A.We * 3;
            const uint8_t* m1 = mean + (size_t)min(max(j1, A.jlo), A.jhi) * (size_t)A.We * 3;
            uint8_t* e = eye + (size_t)y * (size_t)A.eye_pitch + 3 * (size_t)t0;
            uint32_t px[FU_RUN] = {};
            if (cnt == FU_RUN) {
                const uint32_t w0 = fu_load4(e), w1 = fu_load4(e + 4), w2 = fu_load4(e + 8);
                px[0] = w0 & 0xFFFFFFu; px[1] = w0 >> 24 | (w1 & 0xFFFFu) << 8; px[2] = w1 >> 16 | (w2 & 0xFFu) << 16; px[3] = w2 >> 8;
            } else {
#pragma unroll
                for (int k = 0; k < FU_RUN - 1; ++k)
                    if (k < cnt) px[k] = fu_pixel(e + 3 * k);
            }
#pragma unroll
            for (int k = 0; k < FU_RUN; ++k) {
                if (k >= cnt) break;
                const int u = (int)fu_coord(A.ax, A.bx, t0 + k, A.We);                      // fits an int (We <= FU_MAX_W)
                const int i0 = u >> 16, i1 = min(i0 + 1, A.We - 1), fx = (u >> 8) & 255;
                const int o0 = 3 * i0, o1 = 3 * i1;
                const int n0 = 3 * min(max(i0, A.ilo), A.ihi), n1 = 3 * min(max(i1, A.ilo), A.ihi);
                const uint32_t p = fu_blend(fu_pixel(s0 + o0), fu_pixel(s0 + o1), fu_pixel(s1 + o0), fu_pixel(s1 + o1), fx, fy);
                const uint32_t lp = fu_blend(fu_pixel(m0 + n0), fu_pixel(m0 + n1), fu_pixel(m1 + n0), fu_pixel(m1 + n1), fx, fy);
                px[k] = fu_fuse(px[k], lp, p);
            }
            if (cnt == FU_RUN) {
                const uint32_t w0 = px[0] | px[1] << 24, w1 = px[1] >> 8 | px[2] << 16, w2 = px[2] >> 16 | px[3] << 8;
                memcpy(e, &w0, 4); memcpy(e + 4, &w1, 4); memcpy(e + 8, &w2, 4);
            } else {
#pragma unroll
                for (int k = 0; k < FU_RUN - 1; ++k)
                    if (k < cnt) { e[3 * k] = (uint8_t)px[k]; e[3 * k + 1] = (uint8_t)(px[k] >> 8); e[3 * k + 2] = (uint8_t)(px[k] >> 16); }
            }
        }
    }
}

extern "C" size_t v3d_fuse_eye_source_ws_bytes(int n, int Ws, int Hs)
{
    if (n < 1 || Ws < 2 || (Ws & 1) || Hs < 1 || Ws / 2 > FU_MAX_W) return 0;
    const size_t bytes = (size_t)n * (size_t)Hs * (size_t)(Ws / 2) * 3;
    return (bytes + 15) / 16 * 16;
}

extern "C" int v3d_fuse_eye_source_batch(uint8_t* eye_bgr, size_t eye_stride, int eye_pitch, int n, int W, int H,
                                         const uint8_t* sbs_bgr, size_t sbs_stride, int Ws, int Hs, int pitch, int eye, int64_t ax,
                                         int64_t bx, int64_t ay, int64_t by, void* ws, void* stream)
{
    const char* who = "v3d_fuse_eye_source_batch";
    if (!eye_bgr || !sbs_bgr || !ws) { v3d_set_error("%s: null pointer", who); return V3D_ERR_ARG; }
    if ((uintptr_t)ws % 16) { v3d_set_error("%s: ws must be 16-byte aligned", who); return V3D_ERR_ARG; }
    if (n < 1 || W < 1 || H < 1) { v3d_set_error("%s: bad geometry n=%d W=%d H=%d", who, n, W, H); return V3D_ERR_ARG; }
    if ((int64_t)eye_pitch < 3 * (int64_t)W) { v3d_set_error("%s: eye pitch %d < 3 W = %lld", who, eye_pitch, 3LL * W); return V3D_ERR_ARG; }
    if (n > 1 && eye_stride < (size_t)H * (size_t)eye_pitch) {
        v3d_set_error("%s: eye stride %zu B smaller than a frame", who, eye_stride);
        return V3D_ERR_ARG;
    }
    if (Ws < 2 || (Ws & 1) || Hs < 1) { v3d_set_error("%s: bad SBS geometry Ws=%d (even, >= 2) Hs=%d", who, Ws, Hs); return V3D_ERR_ARG; }
    if ((int64_t)pitch < 3 * (int64_t)Ws) { v3d_set_error("%s: pitch %d < 3 Ws = %lld", who, pitch, 3LL * Ws); return V3D_ERR_ARG; }
    if (n > 1 && sbs_stride < (size_t)Hs * (size_t)pitch) {
        v3d_set_error("%s: SBS stride %zu B smaller than a frame", who, sbs_stride);
        return V3D_ERR_ARG;
    }
    if (eye != 0 && eye != 1) { v3d_set_error("%s: eye %d is neither 0 nor 1", who, eye); return V3D_ERR_ARG; }
    const int64_t amin = 1 << 12, amax = 1 << 20, bmax = (int64_t)1 << 40;
    if (ax < amin || ax > amax || ay < amin || ay > amax || bx < -bmax || bx > bmax || by < -bmax || by > bmax) {
        v3d_set_error("%s: map (%lld, %lld, %lld, %lld) outside scale [2^12, 2^20], |offset| <= 2^40", who, (long long)ax,
                      (long long)bx, (long long)ay, (long long)by);
        return V3D_ERR_ARG;
    }
    if (W > FU_MAX_W) { v3d_set_error("%s: width %d > %d", who, W, FU_MAX_W); return V3D_ERR_UNSUPPORTED; }
    if (Ws / 2 > FU_MAX_W) { v3d_set_error("%s: eye width %d > %d", who, Ws / 2, FU_MAX_W); return V3D_ERR_UNSUPPORTED; }
    if (ax > 65536 || ay > 65536) {
        v3d_set_error("%s: map scales (%lld, %lld) above 65536: the stored eye is finer than the frame, fusing has nothing to add",
                      who, (long long)ax, (long long)ay);
        return V3D_ERR_UNSUPPORTED;
    }

    FuArgs A;
    A.eye = eye_bgr; A.eye_stride = eye_stride; A.eye_pitch = eye_pitch; A.n = n; A.W = W; A.H = H;
    A.We = Ws / 2; A.Hs = Hs; A.pitch = pitch;
    A.sbs = sbs_bgr + 3 * (size_t)eye * (size_t)A.We; A.sbs_stride = sbs_stride;
    A.mean = (uint8_t*)ws; A.mean_stride = (size_t)Hs * (size_t)A.We * 3;
    A.ax = ax; A.bx = bx; A.ay = ay; A.by = by;
    A.ilo = fu_near(ax, bx, 0, A.We); A.ihi = fu_near(ax, bx, W - 1, A.We);
    A.jlo = fu_near(ay, by, 0, Hs); A.jhi = fu_near(ay, by, H - 1, Hs);
    A.chunks = v3d_cdiv(A.ihi - A.ilo + 1, FU_S);
    A.mean_items = (long long)A.chunks * (A.jhi - A.jlo + 1);
    A.xblocks = v3d_cdiv(v3d_cdiv(W, FU_RUN), 256);
    A.apply_items = (long long)A.xblocks * H;
    // about FU_LAUNCH_BLOCKS workgroups per launch and at least FU_FLOOR_BLOCKS per frame, never more than there are items for
    const long long per = FU_LAUNCH_BLOCKS / n < FU_FLOOR_BLOCKS ? FU_FLOOR_BLOCKS : FU_LAUNCH_BLOCKS / n;
    const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fuse_means, dim3((unsigned)(A.mean_items < per ? A.mean_items : per), gy), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_fuse_apply, dim3((unsigned)(A.apply_items < per ? A.apply_items : per), gy), dim3(256), 0, st, A);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
