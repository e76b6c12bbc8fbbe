// v3d_framematch.hip -- frame signatures and their exact integer correlation ("Frame matching"; contract in
// include/v3d_hip.h, NumPy restatement in tests/framematch_ref.py).  A signature is the 64 x 36 grid of cell means of a luma
// plane in 8.8 fixed point: sig[cy*64 + cx] = floor(256 S / c) over the cell's c pixels.  The grid is relative to the plane, so
// a squeezed eye, an unsqueezed eye and a 4K frame land on comparable cells.  The scores are
//   num[i][j] = G sum(a_i b_j) - sum(a_i) sum(b_j),   var[i] = G sum(a_i^2) - (sum a_i)^2,   G = 2304,
// in 64-bit integers (every term < 2.3e16 < 2^63), so no bit depends on a schedule; the host divides.
#include "v3d_common.h"
#include "v3d_wave.h"

#define FM_GW V3D_SIG_GW
#define FM_GH V3D_SIG_GH
#define FM_G V3D_SIG_CELLS
#define FM_THREADS 1024

// ---- signature: one workgroup per (cell row, frame).  A lane owns one 16-byte column group and every ny-th row of the cell
// row; it keeps the 16 column sums as packed 16-bit pairs in 8 registers (a cell row has at most ceil(8192 / 36) = 228 rows:
// 228 * 255 = 58140 < 2^16), then adds each run of columns that share a cell to the cell's sum in LDS (integer adds: the order
// does not reach the result).  VEC: base, pitch and stride allow v3d_wave.h's row_load16 its aligned 16-byte loads.
__device__ __forceinline__ void fm_acc(uint32_t (&acc)[8], const uint4 p)
{
    acc[0] += p.x & 0x00FF00FFu; acc[1] += (p.x >> 8) & 0x00FF00FFu;
    acc[2] += p.y & 0x00FF00FFu; acc[3] += (p.y >> 8) & 0x00FF00FFu;
    acc[4] += p.z & 0x00FF00FFu; acc[5] += (p.z >> 8) & 0x00FF00FFu;
    acc[6] += p.w & 0x00FF00FFu; acc[7] += (p.w >> 8) & 0x00FF00FFu;
}

template <bool VEC>
__global__ __launch_bounds__(FM_THREADS) void k_fm_signature(const uint8_t* __restrict__ gray, int W, int H, size_t pitch, size_t stride,
                                                             int ngroups, int ny, uint16_t* __restrict__ sig)
{
    __shared__ uint32_t cells[FM_GW];
    const int cy = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    if (tid < FM_GW) cells[tid] = 0u;
    __syncthreads();
    const int r0 = (cy * H) / FM_GH, r1 = ((cy + 1) * H) / FM_GH;
    const int ty = tid / ngroups, tx = tid - ty * ngroups;
    if (ty < ny) {
        const int x0 = tx * 16;
        const uint8_t* base = gray + (size_t)f * stride;
        uint32_t acc[8] = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };
        int r = r0 + ty;
        for (; r + 3 * ny < r1; r += 4 * ny) {                     // four rows in flight per lane
            const uint4 a = row_load16<VEC>(base + (size_t)r * pitch, x0, W);
            const uint4 b = row_load16<VEC>(base + (size_t)(r + ny) * pitch, x0, W);
            const uint4 c = row_load16<VEC>(base + (size_t)(r + 2 * ny) * pitch, x0, W);
            const uint4 d = row_load16<VEC>(base + (size_t)(r + 3 * ny) * pitch, x0, W);
            fm_acc(acc, a); fm_acc(acc, b); fm_acc(acc, c); fm_acc(acc, d);
        }
        for (; r < r1; r += ny) fm_acc(acc, row_load16<VEC>(base + (size_t)r * pitch, x0, W));
        // column x belongs to cell (64 x + 63) / W: the largest cx with floor(cx W / 64) <= x
        int c = (64 * x0 + 63) / W, nb = ((c + 1) * W) >> 6;
        uint32_t run = 0u;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (x0 + i < W) {
                if (x0 + i >= nb) {                                 // cells are at least one column wide: one step at most
                    atomicAdd(&cells[c], run);
                    run = 0u; c++; nb = ((c + 1) * W) >> 6;
                }
                run += (acc[2 * (i >> 2) + (i & 1)] >> (16 * ((i >> 1) & 1))) & 0xFFFFu;
            }
        }
        atomicAdd(&cells[c], run);
    }
    __syncthreads();
    if (tid < FM_GW) {
        const uint32_t cnt = (uint32_t)(r1 - r0) * (uint32_t)((((tid + 1) * W) >> 6) - ((tid * W) >> 6));
        sig[((size_t)f * FM_GH + cy) * FM_GW + tid] = (uint16_t)((cells[tid] << 8) / cnt);     // 256 * 255 * c < 2^31
    }
}

extern "C" int v3d_frame_signature_batch(const uint8_t* gray, int n, int W, int H, int pitch, size_t frame_stride, uint16_t* sig_out,
                                         void* stream)
{
    if (!gray || !sig_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (n < 1 || n > 65535) { v3d_set_error("frame count %d outside [1, 65535]", n); return V3D_ERR_ARG; }
    if (W < FM_GW || W > 8192 || H < FM_GH || H > 8192) {
        v3d_set_error("signature of a %dx%d plane not supported (64..8192 x 36..8192)", W, H);
        return V3D_ERR_UNSUPPORTED;
    }
    if (pitch < W) { v3d_set_error("pitch %d below the width %d", pitch, W); return V3D_ERR_ARG; }
    if (n > 1 && frame_stride < (size_t)H * (size_t)pitch) {
        v3d_set_error("frame stride %zu below the frame size %zu", frame_stride, (size_t)H * (size_t)pitch);
        return V3D_ERR_ARG;
    }
    const int ngroups = v3d_cdiv(W, 16);                            // <= 512
    int ny = FM_THREADS / ngroups;                                  // row phases of a workgroup, >= 2
    const int max_rows = v3d_cdiv(H, FM_GH) + 1;
    if (ny > max_rows) ny = max_rows;
    const bool vec = ((uintptr_t)gray & 15) == 0 && (pitch & 15) == 0 && (n == 1 || (frame_stride & 15) == 0);
    const dim3 grid(FM_GH, n), block(FM_THREADS);
    if (vec) hipLaunchKernelGGL(k_fm_signature<true>, grid, block, 0, (hipStream_t)stream, gray, W, H, (size_t)pitch, frame_stride, ngroups, ny, sig_out);
    else hipLaunchKernelGGL(k_fm_signature<false>, grid, block, 0, (hipStream_t)stream, gray, W, H, (size_t)pitch, frame_stride, ngroups, ny, sig_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- scores: one wavefront per pair (i, j), 36 cells per lane; the pair's sums fold by butterfly ----
__global__ __launch_bounds__(64) void k_fm_scores(const uint16_t* __restrict__ sa, const uint16_t* __restrict__ sb, int nb,
                                                  long long* __restrict__ num, long long* __restrict__ var_a,
                                                  long long* __restrict__ var_b)
{
    const int j = blockIdx.x, i = blockIdx.y;
    const uint16_t* a = sa + (size_t)i * FM_G;
    const uint16_t* b = sb + (size_t)j * FM_G;
    unsigned long long ab = 0, aa = 0, bb = 0;
    unsigned s_a = 0, s_b = 0;                                      // <= 2304 * 65280 < 2^28
    for (int k = threadIdx.x; k < FM_G; k += 64) {
        const unsigned x = a[k], y = b[k];
        s_a += x; s_b += y;
        ab += (unsigned long long)x * y;
        aa += (unsigned long long)x * x;
        bb += (unsigned long long)y * y;
    }
    ab = wave_sum_u64(ab);
    const unsigned long long ta = wave_sum_u64(s_a), tb = wave_sum_u64(s_b);
    if (j == 0) aa = wave_sum_u64(aa);
    if (i == 0) bb = wave_sum_u64(bb);
    if (threadIdx.x == 0) {
        num[(size_t)i * nb + j] = (long long)(FM_G * ab) - (long long)(ta * tb);
        if (j == 0) var_a[i] = (long long)(FM_G * aa - ta * ta);
        if (i == 0) var_b[j] = (long long)(FM_G * bb - tb * tb);
    }
}

extern "C" int v3d_signature_scores(const uint16_t* sig_a, int na, const uint16_t* sig_b, int nb, int64_t* num_out, int64_t* var_a_out,
                                    int64_t* var_b_out, void* stream)
{
    if (!sig_a || !sig_b || !num_out || !var_a_out || !var_b_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (na < 1 || na > 4096 || nb < 1 || nb > 4096) { v3d_set_error("signature counts %d, %d outside [1, 4096]", na, nb); return V3D_ERR_ARG; }
    hipLaunchKernelGGL(k_fm_scores, dim3(nb, na), dim3(64), 0, (hipStream_t)stream, sig_a, sig_b, nb,
                       reinterpret_cast<long long*>(num_out), reinterpret_cast<long long*>(var_a_out),
                       reinterpret_cast<long long*>(var_b_out));
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
