// v3d_fill.hip -- opt-in hole filling of the matcher's int16 disparity (contract in include/v3d_hip.h; NumPy restatement in
// tests/fill_ref.py; DESIGN.md section 4, "Hole filling").  A pixel is a hole iff d < 0.
//   rows:        a hole takes min(nearest valid to its left, nearest valid to its right) of the INPUT row, or the only one;
//   empty rows:  a row without a valid pixel copies the filled nearest non-empty row (ties: the row above);
//   a frame without a valid pixel is copied unchanged.
//
// k_fill_rows: one workgroup of 256 threads marches a band of rows.  A row is read as the aligned 16-byte chunks that cover it
// (any 2-byte row offset: the loads are unconditional, lanes past the last chunk re-read it); thread t owns chunks
// t*NC .. t*NC+NC-1, i.e. the PPT = 8 NC consecutive chunk positions p = (row offset in elements) + x.  The next row's chunks
// are in flight while the current row is scanned.  The scans carry the VALUE with the index, so the row is never staged in LDS:
//   nearest valid left of my run  = max-scan over the threads of ((p + 1) << 16) | d       (0: none)
//   nearest valid right of my run = max-scan, other direction, of ((WP - p) << 16) | d
// (wave shuffles, then the four wave totals through LDS: 2 x 4 words per row, written by one lane per wave and read as a
// broadcast -- no bank conflict; two buffers by row parity make one barrier per row enough).  The selection runs in registers
// and every full chunk leaves as the widest store its address allows; the row's first and last chunk go element by element.
// k_fill_empty_rows: second, small launch; reads only non-empty rows of `out` and writes only empty ones.
#include "v3d_common.h"
#include "v3d_wave.h"

#define FH_THREADS 256
#define FH_WAVES (FH_THREADS / 64)
#define FH_MAX_W 8192
#define FH_MAX_H 65535
#define FH_EROWS 32               // rows per workgroup of the empty-row pass
#define FH_NONE 0xFFFFu           // "no valid neighbour": above every valid value (0 .. 32767) as an unsigned 16-bit number

namespace {

template <int NC>
__device__ __forceinline__ uint32_t fh_word(const uint4 (&c)[NC], int w)
{
    const uint4 v = c[w >> 2];
    return (w & 3) == 0 ? v.x : (w & 3) == 1 ? v.y : (w & 3) == 2 ? v.z : v.w;
}

// 8 filled elements (4 words) of one full chunk -> the widest stores the address allows (uniform over a row's full chunks)
__device__ __forceinline__ void fh_store_chunk(int16_t* p, const uint32_t (&w)[4])
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if ((a & 15) == 0) {
        st_stream(reinterpret_cast<uint4*>(p), make_uint4(w[0], w[1], w[2], w[3]));
    } else if ((a & 7) == 0) {
        st_stream(reinterpret_cast<uint2*>(p), make_uint2(w[0], w[1]));
        st_stream(reinterpret_cast<uint2*>(p) + 1, make_uint2(w[2], w[3]));
    } else if ((a & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t*>(p)[q] = w[q];
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = (int16_t)(w[i >> 1] >> (16 * (i & 1)));
    }
}

}  // namespace

template <int NC>
__global__ __launch_bounds__(FH_THREADS) void k_fill_rows(const int16_t* in, size_t in_stride, int W, int H, int band, int16_t* out,
                                                          uint8_t* __restrict__ flags)   // in == out is allowed: no __restrict__ on them
{
    constexpr int PPT = 8 * NC, WP = PPT * FH_THREADS;
    __shared__ uint32_t sTot[2][2][FH_WAVES];                  // [row parity][prefix | suffix][wave]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y;
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, H);
    const int16_t* fin = in + (size_t)f * in_stride;
    int16_t* fout = out + (size_t)f * W * H;
    uint8_t* frow_flags = flags + (size_t)f * H;
    const int p0 = tid * PPT;

    uint4 nxt[NC];
    auto load_row = [&](int y) {
        const uintptr_t rs = reinterpret_cast<uintptr_t>(fin + (size_t)y * W);
        const uint4* base = reinterpret_cast<const uint4*>(rs & ~(uintptr_t)15);
        const int nch = (int)(((rs & 15) + 2 * (uintptr_t)W + 15) >> 4);
#pragma unroll
        for (int k = 0; k < NC; ++k) nxt[k] = ld_stream(base + min(tid * NC + k, nch - 1));
    };

    load_row(y0);
    for (int y = y0; y < y1; ++y) {
        uint4 cur[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) cur[k] = nxt[k];
        if (y + 1 < y1) load_row(y + 1);                       // in flight while this row is scanned

        const uintptr_t rs = reinterpret_cast<uintptr_t>(fin + (size_t)y * W);
        const int off = (int)(rs & 15) >> 1;                   // the row's first pixel sits at chunk position `off`
        const int lo = off - p0, hi = off + W - p0;            // my pixels are the run elements i with lo <= i < hi

        // my run: last valid as ((p + 1) << 16) | d, first valid as ((WP - p) << 16) | d
        uint32_t lastk = 0, firstk = 0;
#pragma unroll
        for (int i = PPT - 1; i >= 0; --i) {
            const uint32_t d = (fh_word<NC>(cur, i >> 1) >> (16 * (i & 1))) & 0xFFFFu;
            if (d < 0x8000u && i >= lo && i < hi) {
                if (!lastk) lastk = ((uint32_t)(p0 + i + 1) << 16) | d;
                firstk = ((uint32_t)(WP - (p0 + i)) << 16) | d;
            }
        }
        near2 nn = near2_incl(lastk, firstk, lane);
        uint32_t (*tot)[FH_WAVES] = sTot[y & 1];
        if (lane == 63) tot[0][wave] = nn.pre;
        if (lane == 0) tot[1][wave] = nn.suf;
        nn = near2_excl(nn, lane);
        __syncthreads();
        const near2_any fo = near2_fold<FH_WAVES>(nn, wave, tot[0], tot[1]);
        const uint32_t pre = fo.pre, suf = fo.suf, any = fo.any;
        if (tid == 0) frow_flags[y] = any ? 1 : 0;

        // select in registers: la = nearest valid at or left of i, rb[i] = nearest valid right of i
        uint32_t rb[PPT];
        uint32_t nb = suf ? (suf & 0xFFFFu) : FH_NONE;
#pragma unroll
        for (int i = PPT - 1; i >= 0; --i) {
            const uint32_t d = (fh_word<NC>(cur, i >> 1) >> (16 * (i & 1))) & 0xFFFFu;
            rb[i] = nb;
            if (d < 0x8000u && i >= lo && i < hi) nb = d;
        }
        uint32_t na = pre ? (pre & 0xFFFFu) : FH_NONE;
        uint32_t res[PPT / 2];
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const uint32_t d = (fh_word<NC>(cur, i >> 1) >> (16 * (i & 1))) & 0xFFFFu;
            uint32_t r = d;
            if (d < 0x8000u) { if (i >= lo && i < hi) na = d; }
            else { const uint32_t m = min(na, rb[i]); r = m < 0x8000u ? m : d; }
            if (i & 1) res[i >> 1] |= r << 16; else res[i >> 1] = r;
        }

        int16_t* orow = fout + (size_t)y * W;                  // chunk position p lands at orow + (p - off)
        const int q0 = p0 - off;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c0 = 8 * k;                              // run elements c0 .. c0 + 7
            const uint32_t w4[4] = { res[4 * k], res[4 * k + 1], res[4 * k + 2], res[4 * k + 3] };
            if (c0 >= lo && c0 + 8 <= hi) {
                fh_store_chunk(orow + (q0 + c0), w4);
            } else if (c0 < hi && c0 + 8 > lo) {               // the row's first or last chunk
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (c0 + i >= lo && c0 + i < hi) orow[q0 + c0 + i] = (int16_t)(w4[i >> 1] >> (16 * (i & 1)));
            }
        }
    }
}

// grid (cdiv(H, FH_EROWS), n).  An empty row looks for the nearest flagged row, 256 distances per round (the candidate
// 2d for the row above, 2d + 1 for the row below: the minimum is the nearest, ties above), and copies it from `out`.
__global__ __launch_bounds__(FH_THREADS) void k_fill_empty_rows(int16_t* __restrict__ out, const uint8_t* __restrict__ flags, int W, int H)
{
    __shared__ uint32_t sBest;
    const int tid = threadIdx.x, f = blockIdx.y;
    const uint8_t* fl = flags + (size_t)f * H;
    int16_t* fout = out + (size_t)f * W * H;
    const int y0 = blockIdx.x * FH_EROWS, y1 = min(y0 + FH_EROWS, H);
    const int mine = y0 + tid < y1 ? !fl[y0 + tid] : 0;
    if (!__syncthreads_or(mine)) return;                       // no empty row in this band: the usual case
    for (int y = y0; y < y1; ++y) {
        if (fl[y]) continue;                                   // uniform over the workgroup
        const int far = max(y, H - 1 - y);
        uint32_t best = 0xFFFFFFFFu;
        for (int base = 1; base <= far; base += FH_THREADS) {
            const int d = base + tid;
            uint32_t cand = 0xFFFFFFFFu;
            if (y - d >= 0 && fl[y - d]) cand = 2u * (uint32_t)d;
            else if (y + d < H && fl[y + d]) cand = 2u * (uint32_t)d + 1u;
            if (tid == 0) sBest = 0xFFFFFFFFu;
            __syncthreads();
            if (cand != 0xFFFFFFFFu) atomicMin(&sBest, cand);
            __syncthreads();
            best = sBest;
            __syncthreads();
            if (best != 0xFFFFFFFFu) break;
        }
        if (best == 0xFFFFFFFFu) continue;                     // the whole frame is invalid: stays as the row pass copied it
        const int src = (best & 1u) ? y + (int)(best >> 1) : y - (int)(best >> 1);
        const int16_t* sp = fout + (size_t)src * W;
        int16_t* dp = fout + (size_t)y * W;
        const uintptr_t sa = reinterpret_cast<uintptr_t>(sp), da = reinterpret_cast<uintptr_t>(dp);
        if (((sa ^ da) & 15) == 0) {                           // same 16-byte phase: head, 16-byte body, tail
            const int head = min(W, (int)(((16 - (da & 15)) & 15) >> 1));
            const int nv = (W - head) >> 3;
            if (tid < head) dp[tid] = sp[tid];
            const uint4* s4 = reinterpret_cast<const uint4*>(sp + head);
            uint4* d4 = reinterpret_cast<uint4*>(dp + head);
            for (int i = tid; i < nv; i += FH_THREADS) d4[i] = s4[i];
            for (int i = head + 8 * nv + tid; i < W; i += FH_THREADS) dp[i] = sp[i];
        } else {
            for (int i = tid; i < W; i += FH_THREADS) dp[i] = sp[i];
        }
    }
}

static int fill_check_dims(int n, int W, int H)
{
    if (n < 1 || n > 65535 || W < 1 || H < 1) { v3d_set_error("v3d_fill_holes: bad geometry n=%d W=%d H=%d", n, W, H); return V3D_ERR_ARG; }
    if (W > FH_MAX_W || H > FH_MAX_H) { v3d_set_error("v3d_fill_holes: W=%d > %d or H=%d > %d", W, FH_MAX_W, H, FH_MAX_H); return V3D_ERR_UNSUPPORTED; }
    return V3D_OK;
}

extern "C" size_t v3d_fill_holes_ws_bytes(int n, int H)
{
    if (n < 1 || n > 65535 || H < 1 || H > FH_MAX_H) return 0;
    return ((size_t)n * (size_t)H + 15) & ~(size_t)15;         // one non-empty flag per row
}

template <int NC>
static void launch_fill_rows(const int16_t* in, size_t stride, int n, int W, int H, int band, int16_t* out, uint8_t* flags, hipStream_t st)
{
    hipLaunchKernelGGL(k_fill_rows<NC>, dim3(v3d_cdiv(H, band), n), dim3(FH_THREADS), 0, st, in, stride, W, H, band, out, flags);
}

extern "C" int v3d_fill_holes_disp16_batch(const int16_t* disp16, size_t disp_stride, int n, int W, int H, int16_t* out, void* ws,
                                           void* stream)
{
    if (!disp16 || !out || !ws) { v3d_set_error("v3d_fill_holes_disp16_batch: null pointer"); return V3D_ERR_ARG; }
    const int rc = fill_check_dims(n, W, H);
    if (rc == V3D_ERR_ARG) return rc;
    const size_t frame = (size_t)W * (size_t)H;
    if (n > 1 && disp_stride < frame) { v3d_set_error("v3d_fill_holes_disp16_batch: frame stride %zu below the frame size %zu", disp_stride, frame); return V3D_ERR_ARG; }
    if (((uintptr_t)ws & 15) != 0) { v3d_set_error("v3d_fill_holes_disp16_batch: workspace must be 16-byte aligned"); return V3D_ERR_ARG; }
    if (out == disp16 && n > 1 && disp_stride != frame) {
        v3d_set_error("v3d_fill_holes_disp16_batch: in place needs n == 1 or a dense batch (stride %zu, frame %zu)", disp_stride, frame);
        return V3D_ERR_ARG;
    }
    if (rc != V3D_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* flags = reinterpret_cast<uint8_t*>(ws);
    // about one round of the resident workgroup slots (8 per CU), at least 4 rows per workgroup so that the prefetch has a row to hide
    const size_t rows = (size_t)n * (size_t)H;
    int band = (int)((rows + 2047) / 2048);
    band = band < 4 ? 4 : band > 64 ? 64 : band;
    // the padded run row must hold the row at any 2-byte offset inside its first chunk: 7 + W <= 256 * 8 NC
    if (W + 7 <= 8 * FH_THREADS) launch_fill_rows<1>(disp16, disp_stride, n, W, H, band, out, flags, st);
    else if (W + 7 <= 16 * FH_THREADS) launch_fill_rows<2>(disp16, disp_stride, n, W, H, band, out, flags, st);
    else if (W + 7 <= 32 * FH_THREADS) launch_fill_rows<4>(disp16, disp_stride, n, W, H, band, out, flags, st);
    else launch_fill_rows<5>(disp16, disp_stride, n, W, H, band, out, flags, st);
    hipLaunchKernelGGL(k_fill_empty_rows, dim3(v3d_cdiv(H, FH_EROWS), n), dim3(FH_THREADS), 0, st, out, flags, W, H);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
