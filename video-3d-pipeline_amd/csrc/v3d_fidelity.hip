// v3d_fidelity.hip -- a rendered eye measured against the film's own stored eye (contract in include/v3d_hip.h; NumPy restatement
// in tests/fidelity_ref.py; DESIGN.md section 4, "Rendered-eye fidelity report").
//   v3d_eye_fidelity_batch   per frame: n_cells, sad, ssd, n_bad of the cell means and n_win, ssim_q20 of their luma
// E is the eye as rendered, P the bilinear sample of v3d_render_stereo_source_batch's contract, cells are those of
// v3d_verify_eye_source_batch (the sampling arithmetic is restated here as v3d_verify.hip restates it: that file and v3d_stereo.hip
// stay as they are).  Every number is an integer, so no order of evaluation can change a bit.  Both images are read only; the entry
// neither synchronises nor allocates and uses no atomic.
//
// Three launches.  k_fid_cells walks the cells as k_verify_eye's first pass does: one WAVE owns an item (VF-style: FF_ROWS rows of
// 64 / cx whole cells, one lane per target column), the two sums of a channel travel in one word (sum E below, sum P above: a cell
// has at most 256 targets, so either stays under 2^16) and are folded by lane shuffles; a cell's lane 0 forms the two means (a
// multiplication by a reciprocal from a 256-entry LDS table, exact for these ranges: see ff_recip), adds the colour record's terms
// to its own 64-bit counters and stores the cell's two lumas as ONE 16-bit word of the frame's cell plane in ws.  A workgroup's
// counters go to its own slot of ws.  k_fid_ssim tiles the cell plane: a workgroup owns 32 x 8 windows, forms the 33 x 9 sums of
// 4 x 4 cells they are made of once (one aligned 8-byte load per row of a block) in LDS, and each thread puts its window together
// from its 2 x 2 blocks and does the two 64-bit divisions.  k_fid_reduce adds the slots up, one workgroup per frame.
#include <string.h>
#include "v3d_wave.h"

#define FF_MAX_W 8192          // the render entries' bound on a row and on an eye
#define FF_ROWS 8              // rows a wave walks per item, at least
#define FF_CHUNK 4             // rows whose loads a lane has in flight together
#define FF_BLOCKS 256          // workgroups per frame and stage, at most: as many slots of partial sums
#define FF_TW 32               // windows of a stage-2 tile across
#define FF_TH 8                // and down: FF_TW * FF_TH threads
#define FF_C1 416              // round(0.01^2 255^2 64)
#define FF_C2 235963           // round(0.03^2 255^2 64 63)

struct FfPlan {
    int cx, cy, ncx, ncy, nwx, nwy;                            // cell size, cells, windows
    int bands, cw, nwaves;                                     // rows of cells per item, columns per wave, waves across a row
    long long items, tiles;                                    // stage-1 items and stage-2 tiles per frame
    int tx, g1, g2;                                            // tiles across, workgroups per frame of the two stages
    int ppitch;                                                // cells per row of the cell plane (a multiple of 4)
    size_t plane_bytes, off1, off2, total;                     // bytes per frame's plane; offsets of the two slot arrays; all of ws
};

struct FfArgs {
    const uint8_t* eye;
    size_t eye_stride;
    const uint8_t* sbs;                                        // first byte of the sampled eye's half of row 0
    size_t sbs_stride;
    int eye_pitch, n, W, H, We, Hs, pitch, bad_thr;
    FfPlan p;
    long long ax, bx, ay, by;
    uint16_t* planes;                                          // [n][ncy][ppitch]: Ya | Yb << 8
    unsigned long long* part1;                                 // [n][g1][3]: sad, ssd, n_bad
    unsigned long long* part2;                                 // [n][g2]: the sum of Q, two's complement
};

// a BGR pixel at p as 0x00RRGGBB: its three bytes and no other
V3D_HD static inline uint32_t ff_pixel(const uint8_t* p)
{
    uint16_t lo;
    memcpy(&lo, p, 2);
    return (uint32_t)lo | (uint32_t)p[2] << 16;
}

// an eye pixel: with a pixel behind it in its row (more), one 4-byte load whose fourth byte, the next pixel's first, is dropped
V3D_HD static inline uint32_t ff_eye_pixel(const uint8_t* p, bool more)
{
#ifdef __HIPCC__
    typedef uint32_t ff_u32_any __attribute__((aligned(1)));
    if (more) return __builtin_nontemporal_load(reinterpret_cast<const ff_u32_any*>(p)) & 0xFFFFFFu;
#else
    if (more) { uint32_t v; memcpy(&v, p, 4); return v & 0xFFFFFFu; }
#endif
    return ff_pixel(p);
}

// the taps of the two SBS rows a target row blends, kept from one target row to the next (as v3d_verify.hip's VfTaps)
struct FfTaps { long long j0, j1; uint32_t a0, b0, a1, b1; };

// P of target (t, y): the source entry's arithmetic
V3D_HD static inline uint32_t ff_sample(FfTaps& T, const uint8_t* sbs, int pitch, int Hs, long long ay, long long by, int y, int o0,
                                        int o1, int fx)
{
    const long long vm = (long long)(Hs - 1) << 16, vl = ay * y + by;
    const long long v = vl < 0 ? 0 : vl > vm ? vm : vl;
    const long long j0 = v >> 16, j1 = j0 + 1 < Hs ? j0 + 1 : Hs - 1;
    const int fy = (int)(v >> 8) & 255;
    if (j0 != T.j0) {
        if (j0 == T.j1) { T.a0 = T.a1; T.b0 = T.b1; }
        else { const uint8_t* row = sbs + (size_t)j0 * (size_t)pitch; T.a0 = ff_pixel(row + o0); T.b0 = ff_pixel(row + o1); }
        T.j0 = j0;
    }
    if (j1 != T.j1) {
        if (j1 == j0) { T.a1 = T.a0; T.b1 = T.b0; }
        else { const uint8_t* row = sbs + (size_t)j1 * (size_t)pitch; T.a1 = ff_pixel(row + o0); T.b1 = ff_pixel(row + o1); }
        T.j1 = j1;
    }
    uint32_t c = 0;
    for (int ch = 0; ch < 3; ++ch) {
        const int s = 8 * ch;
        const uint32_t top = (uint32_t)(256 - fx) * (T.a0 >> s & 255u) + (uint32_t)fx * (T.b0 >> s & 255u);
        const uint32_t bot = (uint32_t)(256 - fx) * (T.a1 >> s & 255u) + (uint32_t)fx * (T.b1 >> s & 255u);
        c |= (((uint32_t)(256 - fy) * top + (uint32_t)fy * bot + 32768u) >> 16) << s;
    }
    return c;
}

// floor(x / d) for d = 2 npix in [2, 512] and x = 2 S + npix < 2^18 as the high word of x * m, m = floor((2^32 - 1) / d) + 1:
// m d = 2^32 + e with 0 <= e <= d, and x e < 2^27 keeps the product's excess below one step of the quotient
V3D_HD static inline uint32_t ff_recip(int npix) { return 0xFFFFFFFFu / (uint32_t)(2 * npix) + 1u; }
V3D_HD static inline int ff_mean(uint32_t sum, int npix, uint32_t m) { return (int)(((uint64_t)(2u * sum + (uint32_t)npix) * m) >> 32); }
V3D_HD static inline int ff_luma(int b, int g, int r) { return (9798 * r + 19235 * g + 3735 * b + 16384) >> 15; }

// grid (workgroups of a frame, frames), both walked with the grid's stride.  Every workgroup writes its slot of every frame it walks
__global__ __launch_bounds__(256) void k_fid_cells(const FfArgs A)
{
    __shared__ uint32_t recip[256];                            // [cols - 1][rows - 1] of a cell
    __shared__ unsigned long long scratch[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cx = A.p.cx, cy = A.p.cy;
    const int pl = lane / cx, i = lane - pl * cx;              // the lane's cell of its wave, its column of the cell
    const int cpw = A.p.cw / cx;                               // cells per wave and row
    recip[tid] = ff_recip(((tid >> 4) + 1) * ((tid & 15) + 1));
    __syncthreads();
    for (int f = blockIdx.y; f < A.n; f += gridDim.y) {
        const uint8_t* eye = A.eye + (size_t)f * A.eye_stride;
        const uint8_t* sbs = A.sbs + (size_t)f * A.sbs_stride;
        uint16_t* plane = A.planes + (size_t)f * (A.p.plane_bytes / 2);
        unsigned long long t[3] = { 0ull, 0ull, 0ull };        // sad, ssd, n_bad of the cells this lane is lane 0 of
        for (long long item = (long long)blockIdx.x * 4 + wave; item < A.p.items; item += (long long)gridDim.x * 4) {
            const int wx = (int)(item % A.p.nwaves), bg = (int)(item / A.p.nwaves);
            const int tcol = wx * A.p.cw + lane;
            const bool live = lane < A.p.cw && tcol < A.W;
            const long long um = (long long)(A.We - 1) << 16, ul = A.ax * tcol + A.bx;
            const int u = (int)(ul < 0 ? 0 : ul > um ? um : ul);
            const int i0 = u >> 16, fx = (u >> 8) & 255, o0 = 3 * i0, o1 = 3 * min(i0 + 1, A.We - 1);
            const bool more = tcol + 1 < A.W;
            const int t0 = tcol - i, cols = min(cx, A.W - t0); // the cell's first column and its width (live lanes)
            const int r0 = bg * A.p.bands;                     // the item's first row of cells
            const int ya = r0 * cy, yz = (int)min((long long)min(A.p.ncy, r0 + A.p.bands) * cy, (long long)A.H);
            const uint8_t* col = eye + 3 * (size_t)tcol;
            FfTaps T = { -1, -1, 0u, 0u, 0u, 0u };
            uint32_t s0 = 0, s1 = 0, s2 = 0;                   // per channel: sum E | sum P << 16 of the band being walked
            int band = 0, yb = ya;
            for (int yc = ya; yc < yz; yc += FF_CHUNK) {
                uint32_t e[FF_CHUNK] = {};
                if (live) {
#pragma unroll
                    for (int k = 0; k < FF_CHUNK; ++k)
                        if (yc + k < yz) e[k] = ff_eye_pixel(col + (size_t)(yc + k) * (size_t)A.eye_pitch, more);
                }
#pragma unroll
                for (int k = 0; k < FF_CHUNK; ++k) {
                    const int y = yc + k, ye = min(yb + cy, yz);
                    if (y >= yz) break;
                    if (live) {
                        const uint32_t p = ff_sample(T, sbs, A.pitch, A.Hs, A.ay, A.by, y, o0, o1, fx);
                        s0 += (e[k] & 255u) | (p & 255u) << 16;
                        s1 += (e[k] >> 8 & 255u) | (p >> 8 & 255u) << 16;
                        s2 += (e[k] >> 16) | (p >> 16) << 16;
                    }
                    if (y + 1 != ye) continue;                 // wave-uniform: every lane meets the shuffles
                    for (int off = 1; off < cx; off <<= 1) {
                        const uint32_t v0 = __shfl_down(s0, off), v1 = __shfl_down(s1, off), v2 = __shfl_down(s2, off);
                        if (i + off < cx) { s0 += v0; s1 += v1; s2 += v2; }
                    }
                    if (live && i == 0) {
                        const int rows = ye - yb, npix = cols * rows;
                        const uint32_t m = recip[(cols - 1) * 16 + rows - 1];
                        const int a0 = ff_mean(s0 & 0xFFFFu, npix, m), b0 = ff_mean(s0 >> 16, npix, m);
                        const int a1 = ff_mean(s1 & 0xFFFFu, npix, m), b1 = ff_mean(s1 >> 16, npix, m);
                        const int a2 = ff_mean(s2 & 0xFFFFu, npix, m), b2 = ff_mean(s2 >> 16, npix, m);
                        const int d0 = abs(a0 - b0), d1 = abs(a1 - b1), d2 = abs(a2 - b2), d = d0 + d1 + d2;
                        t[0] += (unsigned)d;
                        t[1] += (unsigned)(d0 * d0 + d1 * d1 + d2 * d2);
                        t[2] += d > A.bad_thr;
                        plane[(size_t)(r0 + band) * (size_t)A.p.ppitch + (size_t)(wx * cpw + pl)] =
                            (uint16_t)(ff_luma(a0, a1, a2) | ff_luma(b0, b1, b2) << 8);
                    }
                    s0 = s1 = s2 = 0u; band++; yb = ye;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = wave_sum_u64(t[k]);
        const unsigned long long s = block_sum_u64<4, 3>(t, lane, wave, tid, scratch);
        if (tid < 3) A.part1[((size_t)f * A.p.g1 + blockIdx.x) * 3 + tid] = s;
        __syncthreads();                                       // the next frame's sums come into the same words
    }
}

// one window's Q from its four sums (include/v3d_hip.h): all operands below 2^31, the two quotients at most 2^20
V3D_HD static inline long long ff_window_q(long long s1, long long s2, long long ss, long long s12)
{
    const long long vars = 64 * ss - s1 * s1 - s2 * s2, covar = 64 * s12 - s1 * s2;
    const unsigned long long a = (unsigned long long)(2 * s1 * s2 + FF_C1), b = (unsigned long long)(s1 * s1 + s2 * s2 + FF_C1);
    const long long c = 2 * covar + FF_C2;
    const unsigned long long ca = (unsigned long long)(c < 0 ? -c : c), d = (unsigned long long)(vars + FF_C2);
    const unsigned long long q1 = (a << 20) / b, q2 = (ca << 20) / d;
    const long long q = (long long)((q1 * q2) >> 20);
    return c < 0 ? -q : q;
}

// grid (workgroups of a frame, frames).  A tile: FF_TW x FF_TH windows = (FF_TW + 1) x (FF_TH + 1) blocks of 4 x 4 cells; the
// block sums lie in three word planes whose rows are FF_TW + 1 = 33 words long, so the four reads of a window's thread are at
// consecutive words across a wave's lanes.  Blocks 0 .. nwx by 0 .. nwy exist, and all their cells do
__global__ __launch_bounds__(FF_TW * FF_TH) void k_fid_ssim(const FfArgs A)
{
    __shared__ uint32_t b12[FF_TH + 1][FF_TW + 1], bss[FF_TH + 1][FF_TW + 1], bxy[FF_TH + 1][FF_TW + 1];   // s1 | s2 << 16, ss, s12
    __shared__ unsigned long long scratch[4][1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wx = tid & (FF_TW - 1), wy = tid / FF_TW;
    for (int f = blockIdx.y; f < A.n; f += gridDim.y) {
        const uint16_t* plane = A.planes + (size_t)f * (A.p.plane_bytes / 2);
        long long q = 0;
        for (long long tile = blockIdx.x; tile < A.p.tiles; tile += gridDim.x) {
            const int bx0 = (int)(tile % A.p.tx) * FF_TW, by0 = (int)(tile / A.p.tx) * FF_TH;
            for (int b = tid; b < (FF_TW + 1) * (FF_TH + 1); b += FF_TW * FF_TH) {
                const int ly = b / (FF_TW + 1), lx = b - ly * (FF_TW + 1), gx = bx0 + lx, gy = by0 + ly;
                uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
                if (gx <= A.p.nwx && gy <= A.p.nwy) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint2 v = *reinterpret_cast<const uint2*>(plane + (size_t)(4 * gy + r) * (size_t)A.p.ppitch + 4 * (size_t)gx);
                        const uint32_t w[2] = { v.x, v.y };
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const uint32_t c = w[k >> 1] >> (16 * (k & 1)), ya = c & 255u, yb = c >> 8 & 255u;
                            s1 += ya; s2 += yb; ss += ya * ya + yb * yb; s12 += ya * yb;
                        }
                    }
                }
                b12[ly][lx] = s1 | s2 << 16; bss[ly][lx] = ss; bxy[ly][lx] = s12;
            }
            __syncthreads();
            if (bx0 + wx < A.p.nwx && by0 + wy < A.p.nwy) {
                const uint32_t p = b12[wy][wx] + b12[wy][wx + 1] + b12[wy + 1][wx] + b12[wy + 1][wx + 1];   // 64 x 255 < 2^16 a half
                const uint32_t ss = bss[wy][wx] + bss[wy][wx + 1] + bss[wy + 1][wx] + bss[wy + 1][wx + 1];
                const uint32_t s12 = bxy[wy][wx] + bxy[wy][wx + 1] + bxy[wy + 1][wx] + bxy[wy + 1][wx + 1];
                q += ff_window_q((long long)(p & 0xFFFFu), (long long)(p >> 16), (long long)ss, (long long)s12);
            }
            __syncthreads();                                   // the next tile's sums come into the same words
        }
        const unsigned long long t[1] = { wave_sum_u64((unsigned long long)q) };
        const unsigned long long s = block_sum_u64<4, 1>(t, lane, wave, tid, scratch);
        if (tid == 0) A.part2[(size_t)f * A.p.g2 + blockIdx.x] = s;
        __syncthreads();
    }
}

// one workgroup per frame (walked with the grid's stride): the slots of both stages added up, the record written whole
__global__ __launch_bounds__(256) void k_fid_reduce(const FfArgs A, long long* out)
{
    __shared__ unsigned long long scratch[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int f = blockIdx.x; f < A.n; f += gridDim.x) {
        unsigned long long t[4] = { 0ull, 0ull, 0ull, 0ull };
        for (int b = tid; b < A.p.g1; b += 256) {
            const unsigned long long* s = A.part1 + ((size_t)f * A.p.g1 + b) * 3;
            t[0] += s[0]; t[1] += s[1]; t[2] += s[2];
        }
        for (int b = tid; b < A.p.g2; b += 256) t[3] += A.part2[(size_t)f * A.p.g2 + b];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = wave_sum_u64(t[k]);
        const unsigned long long s = block_sum_u64<4, 4>(t, lane, wave, tid, scratch);
        long long* o = out + (size_t)f * V3D_FIDELITY_FIELDS;
        if (tid < 3) o[1 + tid] = (long long)s;
        if (tid == 3) o[5] = (long long)s;
        if (tid == 4) o[0] = (long long)A.p.ncx * A.p.ncy;
        if (tid == 5) o[4] = (long long)A.p.nwx * A.p.nwy;
        __syncthreads();
    }
}

// the geometry and the workspace of a call; false outside the entry's range (the caller has looked at everything else)
static bool ff_plan(int n, int W, int H, int64_t ax, int64_t ay, FfPlan* p)
{
    const int64_t amin = 1 << 12, amax = 1 << 20;
    if (n < 1 || W < 1 || H < 1 || W > FF_MAX_W || ax < amin || ax > amax || ay < amin || ay > amax) return false;
    p->cx = (int)((65536 + ax - 1) / ax); p->cy = (int)((65536 + ay - 1) / ay);          // 1 .. 16 each
    p->ncx = (W + p->cx - 1) / p->cx; p->ncy = (int)(((long long)H + p->cy - 1) / p->cy);
    p->nwx = p->ncx >= 8 ? (p->ncx - 8) / 4 + 1 : 0; p->nwy = p->ncy >= 8 ? (p->ncy - 8) / 4 + 1 : 0;
    if (!p->nwx || !p->nwy) p->nwx = p->nwy = 0;
    p->bands = p->cy >= FF_ROWS ? 1 : FF_ROWS / p->cy;
    p->cw = 64 / p->cx * p->cx; p->nwaves = (W + p->cw - 1) / p->cw;
    p->items = (long long)p->nwaves * ((p->ncy + p->bands - 1) / p->bands);
    p->tx = (p->nwx + FF_TW - 1) / FF_TW;
    p->tiles = (long long)p->tx * ((p->nwy + FF_TH - 1) / FF_TH);
    // about 2048 workgroups per launch (8 per CU), at most FF_BLOCKS and at least 8 per frame, never more than there is work for
    const int per = 2048 / n > FF_BLOCKS ? FF_BLOCKS : 2048 / n < 8 ? 8 : 2048 / n;
    const long long blocks = (p->items + 3) / 4;
    p->g1 = (int)(blocks < per ? blocks : per); p->g2 = (int)(p->tiles < per ? p->tiles : per);
    p->ppitch = (p->ncx + 3) / 4 * 4;
    p->plane_bytes = ((size_t)p->ncy * (size_t)p->ppitch * 2 + 15) / 16 * 16;
    p->off1 = (size_t)n * p->plane_bytes;
    p->off2 = p->off1 + (size_t)n * (size_t)p->g1 * 3 * 8;
    p->total = p->off2 + (size_t)n * (size_t)p->g2 * 8;
    return true;
}

extern "C" size_t v3d_eye_fidelity_ws_bytes(int n, int W, int H, int64_t ax, int64_t ay)
{
    FfPlan p;
    return ff_plan(n, W, H, ax, ay, &p) ? p.total : 0;
}

extern "C" int v3d_eye_fidelity_batch(const uint8_t* eye_bgr, size_t eye_stride, int eye_pitch, int n, int W, int H,
                                      const uint8_t* sbs_bgr, size_t sbs_stride, int Ws, int Hs, int pitch, int eye, int64_t ax,
                                      int64_t bx, int64_t ay, int64_t by, int bad_thr, int64_t* out, void* ws, void* stream)
{
    const char* who = "v3d_eye_fidelity_batch";
    if (!eye_bgr || !sbs_bgr || !out || !ws) { v3d_set_error("%s: null pointer", who); return V3D_ERR_ARG; }
    if ((uintptr_t)ws % 16 || (uintptr_t)out % 8) { v3d_set_error("%s: ws must be 16-byte and out 8-byte aligned", who); return V3D_ERR_ARG; }
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
    if (bad_thr < 0 || bad_thr > 765) { v3d_set_error("%s: bad threshold %d outside [0, 765]", who, bad_thr); return V3D_ERR_ARG; }
    if (W > FF_MAX_W) { v3d_set_error("%s: width %d > %d", who, W, FF_MAX_W); return V3D_ERR_UNSUPPORTED; }
    if (Ws / 2 > FF_MAX_W) { v3d_set_error("%s: eye width %d > %d", who, Ws / 2, FF_MAX_W); return V3D_ERR_UNSUPPORTED; }

    FfArgs A;
    if (!ff_plan(n, W, H, ax, ay, &A.p)) { v3d_set_error("%s: outside the entry's range", who); return V3D_ERR_UNSUPPORTED; }
    A.eye = eye_bgr; A.eye_stride = eye_stride; A.eye_pitch = eye_pitch; A.n = n; A.W = W; A.H = H;
    A.We = Ws / 2; A.Hs = Hs; A.pitch = pitch; A.bad_thr = bad_thr;
    A.sbs = sbs_bgr + 3 * (size_t)eye * (size_t)A.We; A.sbs_stride = sbs_stride;
    A.ax = ax; A.bx = bx; A.ay = ay; A.by = by;
    A.planes = (uint16_t*)ws;
    A.part1 = (unsigned long long*)((uint8_t*)ws + A.p.off1);
    A.part2 = (unsigned long long*)((uint8_t*)ws + A.p.off2);
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)(n < 65535 ? n : 65535);
    hipLaunchKernelGGL(k_fid_cells, dim3((unsigned)A.p.g1, gy), dim3(256), 0, st, A);
    if (A.p.g2) hipLaunchKernelGGL(k_fid_ssim, dim3((unsigned)A.p.g2, gy), dim3(FF_TW * FF_TH), 0, st, A);
    hipLaunchKernelGGL(k_fid_reduce, dim3(gy), dim3(256), 0, st, A, (long long*)out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
