// v3d_verify.hip -- the rendered eye checked against the film's own stored eye, cell by cell (contract in include/v3d_hip.h; NumPy
// restatement in tests/verify_ref.py; DESIGN.md section 4, "Source-verified right eye").
//   v3d_verify_eye_source_batch   per cell of cx x cy targets: m = sum over channels |sum E - sum P|; m > tau npix -> the cell takes P
// E is the eye as rendered, P the bilinear sample of v3d_render_stereo_source_batch's contract (the arithmetic is restated here:
// v3d_stereo.hip's instantiations are pinned and stay as they are).  Every number is an integer, so no order of evaluation can
// change a bit.  The entry neither synchronises nor allocates.
//
// One WAVE owns an item: rows of cells worth VF_ROWS rows by 64 / cx whole cells of them, one lane per target column, the lanes
// past the last whole cell idle (cx = 11: 55 of 64 at work).  A cell never leaves its wave, so its sums are folded by lane shuffles
// and the cells need neither LDS nor a barrier: the four waves of a workgroup share nothing but their count of replaced cells.
// Per row a lane loads its eye pixel and the taps of whichever of its two SBS rows the row before did not blend already (VfTaps), every pixel at its own
// address and no load behind a lane's own branch: nothing but a row's payload is touched in either image, whatever the alignment.
// The three sums of a column are of E - P (the contract's A_c - B_c, summed in another order).  An item is walked twice: first for
// every cell's verdict, with no store among the loads and the eye pixels of VF_CHUNK rows in flight together; then the lanes of
// replaced cells sample P again (the SBS rows are in cache) and store it, VF_CHUNK rows at a time.  Replaced cells are counted by
// one vector atomic per workgroup and frame, on the workgroup's number of them.
#include <string.h>
#include "v3d_common.h"

#define VF_MAX_W 8192          // the render entries' bound on a row and on an eye
#define VF_ROWS 8              // rows a wave walks per item, at least: VF_ROWS / cy bands of cells (one where cy is larger)
#define VF_CHUNK 4             // rows whose loads a lane has in flight together
#define VF_BLOCKS 256          // workgroups per frame, at most: as many atomics reach the frame's counter

struct VfArgs {
    uint8_t* eye;
    size_t eye_stride;                                         // bytes between frames
    const uint8_t* sbs;                                        // first byte of the sampled eye's half of row 0
    size_t sbs_stride;
    int eye_pitch, n, W, H, We, Hs, pitch, tau;
    int cx, cy, ncy, bands;                                    // cell size, rows of cells, rows of cells per item
    int cw, nwx;                                               // columns per wave (whole cells), waves across a row
    long long items;                                           // per frame
    long long ax, bx, ay, by;
    uint32_t* replaced;
};

// a BGR pixel at p as 0x00RRGGBB: its three bytes and no other (a 2-byte and a 1-byte load, wherever p lies)
V3D_HD static inline uint32_t vf_pixel(const uint8_t* p)
{
    uint16_t lo;
    memcpy(&lo, p, 2);
    return (uint32_t)lo | (uint32_t)p[2] << 16;
}

// an eye pixel read once: with a pixel behind it in its row (more), one 4-byte load at its own address whose fourth byte, the next
// pixel's first, is dropped; the row's last pixel as its three bytes
V3D_HD static inline uint32_t vf_eye_pixel(const uint8_t* p, bool more)
{
#ifdef __HIPCC__
    typedef uint32_t vf_u32_any __attribute__((aligned(1)));
    if (more) return __builtin_nontemporal_load(reinterpret_cast<const vf_u32_any*>(p)) & 0xFFFFFFu;
#else
    if (more) { uint32_t v; memcpy(&v, p, 4); return v & 0xFFFFFFu; }
#endif
    return vf_pixel(p);
}

// The taps of the two SBS rows a target row blends, kept from one target row to the next: under an enlarging map consecutive rows
// blend the same pair of rows or move on by one, and only a row that is new is loaded (four loads, none behind a lane's branch:
// the row indices depend on y alone).  j0, j1: the rows held, -1 for none
struct VfTaps { long long j0, j1; uint32_t a0, b0, a1, b1; };

// P of target (t, y): o0, o1 the byte offsets of the column's taps i0, i1, fx its fraction; v is 64 bits wide (Hs has no bound
// but int's).  16-bit products and a sum below 2^24 + 2^15: the source entry's arithmetic
V3D_HD static inline uint32_t vf_sample(VfTaps& T, const uint8_t* sbs, int pitch, int Hs, long long ay, long long by, int y, int o0,
                                        int o1, int fx)
{
    const long long vm = (long long)(Hs - 1) << 16, vl = ay * y + by;
    const long long v = vl < 0 ? 0 : vl > vm ? vm : vl;
    const long long j0 = v >> 16, j1 = j0 + 1 < Hs ? j0 + 1 : Hs - 1;
    const int fy = (int)(v >> 8) & 255;
    if (j0 != T.j0) {
        if (j0 == T.j1) { T.a0 = T.a1; T.b0 = T.b1; }
        else { const uint8_t* row = sbs + (size_t)j0 * (size_t)pitch; T.a0 = vf_pixel(row + o0); T.b0 = vf_pixel(row + o1); }
        T.j0 = j0;
    }
    if (j1 != T.j1) {
        if (j1 == j0) { T.a1 = T.a0; T.b1 = T.b0; }
        else { const uint8_t* row = sbs + (size_t)j1 * (size_t)pitch; T.a1 = vf_pixel(row + o0); T.b1 = vf_pixel(row + o1); }
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

__global__ void k_verify_zero(uint32_t* replaced, int n)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) replaced[i] = 0u;
}

// grid (workgroups of a frame, frames), both walked with the grid's stride: neither a tall image nor a long batch can pass a
// grid limit.  An item's waves across a row are neighbours in a workgroup, so their loads meet in the same cache lines.  A frame
// has at most VF_BLOCKS workgroups and each adds its count to the frame's counter ONCE: atomics on one address are served one
// after the other (one per wave and item group, 8100 to a 4K frame's counter, took 155 us per frame)
__global__ __launch_bounds__(256) void k_verify_eye(const VfArgs A)
{
    __shared__ uint32_t wave_count[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cx = A.cx, cy = A.cy;
    const int pl = lane / cx, i = lane - pl * cx;              // the lane's cell of its wave, its column of the cell
    for (int f = blockIdx.y; f < A.n; f += gridDim.y) {
        uint8_t* eye = A.eye + (size_t)f * A.eye_stride;
        const uint8_t* sbs = A.sbs + (size_t)f * A.sbs_stride;
        uint32_t count = 0;                                    // replaced cells this lane stands for (as a cell's lane 0)
        for (long long item = (long long)blockIdx.x * 4 + wave; item < A.items; item += (long long)gridDim.x * 4) {
            const int wx = (int)(item % A.nwx), bg = (int)(item / A.nwx);
            const int t = wx * A.cw + lane;
            const bool live = lane < A.cw && t < A.W;
            // the column's taps: u fits an int (We <= VF_MAX_W)
            const long long um = (long long)(A.We - 1) << 16, ul = A.ax * t + A.bx;
            const int u = (int)(ul < 0 ? 0 : ul > um ? um : ul);
            const int i0 = u >> 16, fx = (u >> 8) & 255, o0 = 3 * i0, o1 = 3 * min(i0 + 1, A.We - 1);
            const bool more = t + 1 < A.W;
            const int t0 = t - i, cols = min(cx, A.W - t0);    // the cell's first column and its width (live lanes)
            const int ya = bg * A.bands * cy, yz = min(min(A.ncy, (bg + 1) * A.bands) * cy, A.H);      // the item's rows
            uint8_t* col = eye + 3 * (size_t)t;
            // 1. the verdicts of the item's cells, no store yet: VF_CHUNK rows' eye pixels are in flight together, and a band of
            // cells ends after whichever row is its last (a wave-uniform test, so every lane meets the shuffles)
            uint32_t bad_bands = 0;                            // bit b: the lane's cell in the item's band b is replaced
            {
                VfTaps T = { -1, -1, 0u, 0u, 0u, 0u };
                int d0 = 0, d1 = 0, d2 = 0, band = 0, yb = ya; // the sums, number and first row of the band being walked
                for (int yc = ya; yc < yz; yc += VF_CHUNK) {
                    uint32_t e[VF_CHUNK] = {};
                    if (live) {
#pragma unroll
                        for (int k = 0; k < VF_CHUNK; ++k)
                            if (yc + k < yz) e[k] = vf_eye_pixel(col + (size_t)(yc + k) * (size_t)A.eye_pitch, more);
                    }
#pragma unroll
                    for (int k = 0; k < VF_CHUNK; ++k) {
                        const int y = yc + k, ye = min(yb + cy, yz);
                        if (y >= yz) break;
                        if (live) {
                            const uint32_t p = vf_sample(T, sbs, A.pitch, A.Hs, A.ay, A.by, y, o0, o1, fx);
                            d0 += (int)(e[k] & 255u) - (int)(p & 255u);
                            d1 += (int)(e[k] >> 8 & 255u) - (int)(p >> 8 & 255u);
                            d2 += (int)(e[k] >> 16) - (int)(p >> 16);
                        }
                        if (y + 1 != ye) continue;
                        // the cell's sums on its lane 0: after the step `off` a lane holds its own column and the next 2 off - 1
                        for (int off = 1; off < cx; off <<= 1) {
                            const int s0 = __shfl_down(d0, off), s1 = __shfl_down(d1, off), s2 = __shfl_down(d2, off);
                            if (i + off < cx) { d0 += s0; d1 += s1; d2 += s2; }
                        }
                        const int m = abs(d0) + abs(d1) + abs(d2);
                        const int verdict = __shfl_up((int)(m > A.tau * cols * (ye - yb)), i);           // that of the cell's lane 0
                        const bool bad = live && verdict != 0;
                        bad_bands |= (uint32_t)bad << band;
                        count += bad && i == 0;
                        d0 = d1 = d2 = 0; band++; yb = ye;
                    }
                }
            }
            // 2. the lanes of replaced cells walk the item again: VF_CHUNK rows sampled (the SBS rows are in cache), then stored,
            // so that a row's loads do not wait behind the row before's stores
            if (bad_bands) {
                VfTaps T = { -1, -1, 0u, 0u, 0u, 0u };
                int band = 0, yb = ya;
                for (int yc = ya; yc < yz; yc += VF_CHUNK) {
                    uint32_t p[VF_CHUNK] = {};
#pragma unroll
                    for (int k = 0; k < VF_CHUNK; ++k)
                        if (yc + k < yz) p[k] = vf_sample(T, sbs, A.pitch, A.Hs, A.ay, A.by, yc + k, o0, o1, fx);
#pragma unroll
                    for (int k = 0; k < VF_CHUNK; ++k) {
                        const int y = yc + k;
                        if (y >= yz) break;
                        if (bad_bands >> band & 1u) {
                            uint8_t* q = col + (size_t)y * (size_t)A.eye_pitch;
                            q[0] = (uint8_t)p[k]; q[1] = (uint8_t)(p[k] >> 8); q[2] = (uint8_t)(p[k] >> 16);
                        }
                        if (y + 1 == min(yb + cy, yz)) { band++; yb += cy; }
                    }
                }
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) count += (uint32_t)__shfl_xor((int)count, s);
        if (lane == 0) wave_count[wave] = count;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            if (total) atomicAdd(A.replaced + f, total);
        }
        __syncthreads();                                       // the next frame's counts come into the same words
    }
}

extern "C" int v3d_verify_eye_source_batch(uint8_t* eye_bgr, size_t eye_stride, int eye_pitch, int n, int W, int H,
                                           const uint8_t* sbs_bgr, size_t sbs_stride, int Ws, int Hs, int pitch, int eye, int64_t ax,
                                           int64_t bx, int64_t ay, int64_t by, int tau, uint32_t* replaced, void* stream)
{
    const char* who = "v3d_verify_eye_source_batch";
    if (!eye_bgr || !sbs_bgr || !replaced) { v3d_set_error("%s: null pointer", who); return V3D_ERR_ARG; }
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
    if (tau < 0 || tau > 765) { v3d_set_error("%s: tau %d outside [0, 765]", who, tau); return V3D_ERR_ARG; }
    if (W > VF_MAX_W) { v3d_set_error("%s: width %d > %d", who, W, VF_MAX_W); return V3D_ERR_UNSUPPORTED; }
    if (Ws / 2 > VF_MAX_W) { v3d_set_error("%s: eye width %d > %d", who, Ws / 2, VF_MAX_W); return V3D_ERR_UNSUPPORTED; }

    VfArgs A;
    A.eye = eye_bgr; A.eye_stride = eye_stride; A.eye_pitch = eye_pitch; A.n = n; A.W = W; A.H = H;
    A.We = Ws / 2; A.Hs = Hs; A.pitch = pitch; A.tau = tau;
    A.sbs = sbs_bgr + 3 * (size_t)eye * (size_t)A.We; A.sbs_stride = sbs_stride;
    A.cx = (int)((65536 + ax - 1) / ax); A.cy = (int)((65536 + ay - 1) / ay);        // 1 .. 16 each
    A.ncy = v3d_cdiv(H, A.cy);
    A.bands = A.cy >= VF_ROWS ? 1 : VF_ROWS / A.cy;
    A.cw = 64 / A.cx * A.cx; A.nwx = v3d_cdiv(W, A.cw);
    A.items = (long long)A.nwx * v3d_cdiv(A.ncy, A.bands);
    A.ax = ax; A.bx = bx; A.ay = ay; A.by = by; A.replaced = replaced;
    const long long blocks = (A.items + 3) / 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_verify_zero, dim3((unsigned)(n < 256 * 1024 ? v3d_cdiv(n, 256) : 1024)), dim3(256), 0, st, replaced, n);
    // about 2048 workgroups per launch (8 per CU), at most VF_BLOCKS and at least 8 per frame, never more than there are items for
    const int per = 2048 / n > VF_BLOCKS ? VF_BLOCKS : 2048 / n < 8 ? 8 : 2048 / n;
    hipLaunchKernelGGL(k_verify_eye, dim3((unsigned)(blocks < per ? blocks : per), (unsigned)(n < 65535 ? n : 65535)), dim3(256), 0, st, A);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
