// v3d_colour.hip -- colour matching between two releases of a film (contracts in include/v3d_hip.h; NumPy restatement in
// tests/colour_ref.py; DESIGN.md section 4, "Colour matching"): per-channel histograms of a rectangle of BGR frames, the
// histogram-matching table between two sets of them, and the table applied to a rectangle.
//   v3d_bgr_hist_batch     hist[f][c][v] = #{pixels of the rectangle whose byte c is v}
//   v3d_colour_lut_batch   lut[v] = the smallest u with Cf[u] Ns >= Cs[v] Nf   (inclusive prefix sums, exact 128-bit compare)
//   v3d_bgr_lut_batch      dst = lut[256 c + src] over the rectangle, in place or out of place
// Every number is an integer: neither the order of the atomics nor the grid can change a bit.  No entry synchronises or allocates.
//
// A row of the rectangle is its segment of nb = 3 (x1 - x0) bytes.  Both streaming kernels walk it in the ALIGNED 16-byte blocks
// that hold it, whatever the base address and the pitch: block b of a row starts `head` = (segment address & 15) bytes before
// the segment plus 16 b, so a byte of it is byte r = 16 b + i - head of the segment, counted iff 0 <= r < nb, and its channel is
// r mod 3 = (b + i + 48 - head) mod 3 (16 = 1 mod 3).  The blocks at a segment's two ends are handled byte by byte under that test;
// the blocks between them are whole.
#include "v3d_common.h"
#include "v3d_wave.h"

#define COL_BINS 768           // u32 [3][256] per frame
#define COL_CHUNK 48           // bytes a lane of the histogram owns: three blocks, 16 pixels, every channel 16 times

struct col_rect { int nb, rows; size_t first; };              // segment bytes, rows, byte offset of (x0, y0) in a frame
static int col_check_image(int n, int W, int H, int pitch, size_t frame_stride, int x0, int y0, int x1, int y1, const char* what,
                           col_rect* r)
{
    if (n < 1 || n > 65535) { v3d_set_error("bad batch %d", n); return V3D_ERR_ARG; }
    if (W < 1 || W > 65535 || H < 1 || H > 65535) { v3d_set_error("%s of %d x %d: sizes are 1 .. 65535", what, W, H); return V3D_ERR_ARG; }
    if (pitch < 3 * W) { v3d_set_error("%s pitch %d below the row's %d bytes", what, pitch, 3 * W); return V3D_ERR_ARG; }
    if (n > 1 && frame_stride < (size_t)H * (size_t)pitch) { v3d_set_error("%s frame stride %zu below the frame size %zu", what, frame_stride, (size_t)H * (size_t)pitch); return V3D_ERR_ARG; }
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x0 >= x1 || y0 >= y1) { v3d_set_error("rectangle [%d, %d) x [%d, %d) is empty or leaves the %d x %d image", x0, x1, y0, y1, W, H); return V3D_ERR_ARG; }
    r->nb = 3 * (x1 - x0); r->rows = y1 - y0; r->first = (size_t)y0 * (size_t)pitch + 3 * (size_t)x0;
    return V3D_OK;
}
// rows per workgroup of a (bands, n) grid: about 1024 workgroups per launch whatever n is (four per CU: one round, all resident),
// at least 8 per frame, and never so many that a workgroup has less than one step of its 256 lanes to do
static int col_band(int rows, int n, int nb, int bytes_per_lane)
{
    const int per = 1024 / n > 8 ? 1024 / n : 8;
    const int fill = v3d_cdiv(256 * bytes_per_lane, nb);
    const int band = v3d_cdiv(rows, per);
    return band > fill ? band : fill;
}

__global__ void k_col_zero(uint32_t* hist, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) hist[i] = 0u;
}

// the LDS word offsets of the channels of the bytes j = 0, 1, 2 (mod 3) of a block or chunk whose byte 0 has channel ph
struct col_off3 { int o[3]; };
__device__ __forceinline__ col_off3 col_offsets(int ph)
{
    col_off3 t;
    t.o[0] = 256 * ph; t.o[1] = ph == 2 ? 0 : 256 * ph + 256; t.o[2] = 768 - t.o[0] - t.o[1];
    return t;
}
#define COL_BYTE(w, j) (((w)[(j) >> 2] >> (8 * ((j) & 3))) & 255u)

// A lane's 48 bytes.  rel: the segment byte of the chunk's byte 0 (-15 .. nb; nb = nothing of it counts).  LDS atomics without a
// return value.  A chunk inside the segment walks each channel's 16 values and issues one atomic per RUN of equal neighbours: film
// frames are smooth and letterbox bars constant, so the lanes of a wave hit the same bin, and same-address atomics serialise.  The
// form that won its A/B (profiles/colour_match_ab.json): a constant 4K frame 10.6 us against 82.4 us for one atomic per
// byte, a real-looking one 7.6 against 9.0, noise 8.9 against 8.0.  A chunk at either end of a segment tests and counts every byte.
__device__ __forceinline__ void col_count48(uint32_t* h, const uint32_t (&w)[12], int rel, int nb)
{
    const col_off3 t = col_offsets((rel + 48) % 3);
    if (rel >= 0 && rel + COL_CHUNK <= nb) {
#pragma unroll
        for (int s = 0; s < 3; s++) {                          // the 16 values of one channel: equal neighbours share an atomic
            uint32_t cur = COL_BYTE(w, s), cnt = 1u;
#pragma unroll
            for (int j = s + 3; j < COL_CHUNK; j += 3) {
                const uint32_t v = COL_BYTE(w, j);
                if (v == cur) cnt++;
                else { atomicAdd(h + t.o[s] + cur, cnt); cur = v; cnt = 1u; }
            }
            atomicAdd(h + t.o[s] + cur, cnt);
        }
    } else {
#pragma unroll
        for (int j = 0; j < COL_CHUNK; j++)
            if ((unsigned)(rel + j) < (unsigned)nb) atomicAdd(h + t.o[j % 3] + COL_BYTE(w, j), 1u);
    }
}

// grid (bands, n), 256 lanes.  The items of a band are (row, chunk) pairs, cpr chunks to a row (the most any alignment needs), dealt
// to the lanes in order; a lane fetches the three blocks of two items before it counts either (six 16-byte loads in flight).  A
// block that holds nothing of the segment is not fetched: its lane reads the row's first block again, which always holds some.
__global__ __launch_bounds__(256) void k_bgr_hist(const uint8_t* __restrict__ seg, size_t frame_stride, int pitch, int nb, int rows,
                                                  int band, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[COL_BINS];
    const int tid = threadIdx.x;
    for (int i = tid; i < COL_BINS; i += 256) h[i] = 0u;
    __syncthreads();
    seg += blockIdx.y * frame_stride;
    hist += (size_t)blockIdx.y * COL_BINS;
    const int r0 = blockIdx.x * band, r1 = min(rows, r0 + band);
    const int cpr = (nb + 15 + COL_CHUNK - 1) / COL_CHUNK;
    const int drow = 256 / cpr, dc = 256 % cpr;
    int row = r0 + tid / cpr, c = tid % cpr;
    while (row < r1) {
        uint32_t w[2][12];
        int rel[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const bool live = row < r1;
            const uint8_t* p = seg + (size_t)(live ? row : r1 - 1) * (size_t)pitch;
            const int head = (int)((uintptr_t)p & 15), o = COL_CHUNK * c;
            const uint4* blk = reinterpret_cast<const uint4*>(p - head);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint4 v = ld_stream(blk + (live && o + 16 * k < head + nb ? 3 * c + k : 0));
                w[u][4 * k] = v.x; w[u][4 * k + 1] = v.y; w[u][4 * k + 2] = v.z; w[u][4 * k + 3] = v.w;
            }
            rel[u] = live && o < head + nb ? o - head : nb;
            row += drow; c += dc;
            if (c >= cpr) { c -= cpr; row++; }
        }
        col_count48(h, w[0], rel[0], nb);
        col_count48(h, w[1], rel[1], nb);
    }
    __syncthreads();
    for (int i = tid; i < COL_BINS; i += 256) {
        const uint32_t v = h[i];
        if (v) atomicAdd(hist + i, v);
    }
}

extern "C" int v3d_bgr_hist_batch(const uint8_t* bgr, size_t frame_stride, int n, int W, int H, int pitch, int x0, int y0, int x1,
                                  int y1, uint32_t* hist, void* stream)
{
    if (!bgr || !hist) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    col_rect r;
    if (col_check_image(n, W, H, pitch, frame_stride, x0, y0, x1, y1, "image", &r) != V3D_OK) return V3D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int band = col_band(r.rows, n, r.nb, COL_CHUNK);
    const size_t count = (size_t)n * COL_BINS;
    hipLaunchKernelGGL(k_col_zero, dim3((unsigned)(count / 256 < 1024 ? count / 256 : 1024)), dim3(256), 0, st, hist, count);
    hipLaunchKernelGGL(k_bgr_hist, dim3(v3d_cdiv(r.rows, band), n), dim3(256), 0, st, bgr + r.first, frame_stride, pitch, r.nb, r.rows,
                       band, hist);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- the table: grid (tables, 3), thread v owns level v.  The sums over a group's frames are below 2^32 * 65535 < 2^48, the two
// products of the compare below 2^96: 128-bit integers.  Cs is non-decreasing in v, so is the smallest u that reaches it: the
// table is monotone ----
__global__ __launch_bounds__(256) void k_colour_lut(const uint32_t* __restrict__ hist_src, const uint32_t* __restrict__ hist_dst, int n,
                                                    int group, uint8_t* __restrict__ lut)
{
    __shared__ unsigned long long Cf[256];
    __shared__ unsigned long long tot[2][4];
    const int v = threadIdx.x, lane = v & 63, wave = v >> 6, c = blockIdx.y;
    const int f0 = blockIdx.x * group, f1 = min(n, f0 + group);
    unsigned long long s = 0, d = 0;
    for (int f = f0; f < f1; f++) {
        s += hist_src[((size_t)f * 3 + c) * 256 + v];
        d += hist_dst[((size_t)f * 3 + c) * 256 + v];
    }
    const incl_total64 cs = block_incl_add_u64<4>(s, lane, wave, tot[0]);
    const incl_total64 cf = block_incl_add_u64<4>(d, lane, wave, tot[1]);
    Cf[v] = cf.incl;
    __syncthreads();
    const unsigned long long Ns = cs.total, Nf = cf.total;
    int u = v;
    if (Ns != 0 && Nf != 0) {
        const unsigned __int128 want = (unsigned __int128)cs.incl * Nf;
        int lo = 0, hi = 255;                                  // Cf[255] Ns = Nf Ns >= Cs[v] Nf: the answer exists
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned __int128)Cf[mid] * Ns >= want) hi = mid; else lo = mid + 1;
        }
        u = lo;
    }
    lut[((size_t)blockIdx.x * 3 + c) * 256 + v] = (uint8_t)u;
}

extern "C" int v3d_colour_lut_batch(const uint32_t* hist_src, const uint32_t* hist_dst, int n, int group, uint8_t* lut, void* stream)
{
    if (!hist_src || !hist_dst || !lut) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n < 1 || n > 65535) { v3d_set_error("bad batch %d", n); return V3D_ERR_ARG; }
    if (group < 1 || group > n) { v3d_set_error("group %d outside [1, %d]", group, n); return V3D_ERR_ARG; }
    hipLaunchKernelGGL(k_colour_lut, dim3(v3d_cdiv(n, group), 3), dim3(256), 0, (hipStream_t)stream, hist_src, hist_dst, n, group, lut);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- the table applied: grid (bands, n), the items of a band are (row, block) pairs over the DESTINATION's aligned blocks.
// SAME: source and destination rows sit at the same byte of a 16-byte block (always so in place), a whole block is one aligned
// load; else its 16 source bytes are read one by one.  A whole block is one 16-byte store, the ends of a row byte stores ----
template <bool SAME>
__global__ __launch_bounds__(256) void k_bgr_lut(const uint8_t* src, size_t src_stride, int src_pitch, const uint8_t* __restrict__ lut,
                                                 int lut_stride, uint8_t* dst, size_t dst_stride, int dst_pitch, int nb, int rows, int band)
{
    __shared__ uint8_t t[COL_BINS];
    const int tid = threadIdx.x;
    lut += (size_t)blockIdx.y * (size_t)lut_stride;
    for (int i = tid; i < COL_BINS; i += 256) t[i] = lut[i];
    __syncthreads();
    src += blockIdx.y * src_stride; dst += blockIdx.y * dst_stride;
    const int r0 = blockIdx.x * band, r1 = min(rows, r0 + band);
    const int bpr = (nb + 15 + 15) / 16;
    const int drow = 256 / bpr, db = 256 % bpr;
    int row = r0 + tid / bpr, b = tid % bpr;
    while (row < r1) {
        const uint8_t* p = src + (size_t)row * (size_t)src_pitch;
        uint8_t* q = dst + (size_t)row * (size_t)dst_pitch;
        const int head = (int)((uintptr_t)q & 15), rel = 16 * b - head;
        if (rel < nb) {
            const col_off3 o = col_offsets((rel + 48) % 3);
            if (rel >= 0 && rel + 16 <= nb) {
                uint32_t w[4];
                if (SAME) {
                    const uint4 v = ld_stream(reinterpret_cast<const uint4*>(p + rel));
                    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        w[i] = (uint32_t)p[rel + 4 * i] | (uint32_t)p[rel + 4 * i + 1] << 8 | (uint32_t)p[rel + 4 * i + 2] << 16 | (uint32_t)p[rel + 4 * i + 3] << 24;
                }
                uint32_t g[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
                for (int j = 0; j < 16; j++) g[j >> 2] |= (uint32_t)t[o.o[j % 3] + COL_BYTE(w, j)] << (8 * (j & 3));
                st_stream(reinterpret_cast<uint4*>(q + rel), make_uint4(g[0], g[1], g[2], g[3]));
            } else {
#pragma unroll
                for (int j = 0; j < 16; j++)
                    if ((unsigned)(rel + j) < (unsigned)nb) q[rel + j] = t[o.o[j % 3] + p[rel + j]];
            }
        }
        row += drow; b += db;
        if (b >= bpr) { b -= bpr; row++; }
    }
}

extern "C" int v3d_bgr_lut_batch(const uint8_t* src, size_t src_stride, int n, int W, int H, int pitch, int x0, int y0, int x1, int y1,
                                 const uint8_t* lut, int lut_stride, uint8_t* dst, size_t dst_stride, int dst_pitch, void* stream)
{
    if (!src || !lut || !dst) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    col_rect r, rd;
    if (col_check_image(n, W, H, pitch, src_stride, x0, y0, x1, y1, "source", &r) != V3D_OK) return V3D_ERR_ARG;
    if (col_check_image(n, W, H, dst_pitch, dst_stride, x0, y0, x1, y1, "destination", &rd) != V3D_OK) return V3D_ERR_ARG;
    if (lut_stride != 0 && lut_stride < COL_BINS) { v3d_set_error("table stride %d: 0 (one table) or at least %d", lut_stride, COL_BINS); return V3D_ERR_ARG; }
    const size_t se = (size_t)(n - 1) * src_stride + (size_t)(H - 1) * (size_t)pitch + 3 * (size_t)W;
    const size_t de = (size_t)(n - 1) * dst_stride + (size_t)(H - 1) * (size_t)dst_pitch + 3 * (size_t)W;
    const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
    const bool in_place = s == d && pitch == dst_pitch && (n == 1 || src_stride == dst_stride);
    if (!in_place && s < d + de && d < s + se) { v3d_set_error("destination overlaps the source without being the source"); return V3D_ERR_ARG; }
    const bool same = ((s + r.first) & 15) == ((d + rd.first) & 15) && ((pitch - dst_pitch) & 15) == 0 &&
                      (n == 1 || ((src_stride - dst_stride) & 15) == 0);
    const int band = col_band(r.rows, n, r.nb, 16);
    const dim3 grid(v3d_cdiv(r.rows, band), n);
    hipStream_t st = (hipStream_t)stream;
    if (same) hipLaunchKernelGGL(k_bgr_lut<true>, grid, dim3(256), 0, st, src + r.first, src_stride, pitch, lut, lut_stride, dst + rd.first, dst_stride, dst_pitch, r.nb, r.rows, band);
    else hipLaunchKernelGGL(k_bgr_lut<false>, grid, dim3(256), 0, st, src + r.first, src_stride, pitch, lut, lut_stride, dst + rd.first, dst_stride, dst_pitch, r.nb, r.rows, band);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
