// v3d_temporal_mc.hip -- the block search behind the motion-compensated temporal window (`--temporal-motion S`; DESIGN.md
// section 4, "Motion-compensated window"; contract in include/v3d_hip.h, NumPy restatement in tests/temporal_mc_ref.py).
//   v3d_temporal_motion  block-matching fields between adjacent frames of the buffer, the compensated residual and the scene
//                        cuts it gives (the zeroing of the residual and the cut flags are v3d_temporal.hip's kernels).
// The filter that reads along the fields, v3d_temporal_filter_mc_batch, is k_tp_filter<VEC, true> in v3d_temporal.hip.
// Blocks are 16x16 luma pixels anchored at (0,0), edge blocks clipped.  All integers: the bits do not depend on any order.
#include "v3d_temporal_internal.h"
#include "v3d_wave.h"

#define MC_MAX_S 32
#define MC_NB 4                                            // horizontally adjacent blocks per workgroup: one wavefront each
#define MC_WIN_ROWS (16 + 2 * MC_MAX_S)
#define MC_WIN_PITCH (16 * MC_NB + 2 * MC_MAX_S + 4)       // bytes; + 4: the fifth dword a shifted 16-byte row read touches

// ---- the search (the hot kernel) ----
// A workgroup of four wavefronts owns four horizontally adjacent blocks of frame u in one direction (v = u + 1 or u - 1); grid
// x = 2 * block group + direction, y = block row, z = u.  The (16 + 2S) x (64 + 2S) search window of Y_v is staged in LDS byte by
// byte with the edge clamp applied, so the inner loop has none and needs no alignment of the frames; Y_u's four blocks are staged
// too, pixels outside the frame as 0.  Wavefront w then holds its block's 16 rows as 64 dwords in registers, its lanes own the
// candidates (rank = (dy+S)(2S+1) + (dx+S), 64 per sweep): per row five aligned LDS dwords, four v_alignbit_b32 by the lane's
// byte shift and four v_sad_u8.  A clipped block masks the window's bytes where the block has no pixel (|0 - 0| = 0) and skips the
// missing rows.  The key cost * 8192 + rank is minimised per lane, then across the wavefront: integer min, no order.
template <bool CLIPPED>
__device__ __forceinline__ uint32_t mc_block_sad(const uint32_t* __restrict__ win, int word, uint32_t sh, const uint32_t (&yu)[16][4],
                                                 int bh, const uint32_t (&msk)[4])
{
    uint32_t sad = 0;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        if (!CLIPPED || r < bh) {
            const uint32_t* p = win + r * (MC_WIN_PITCH / 4) + word;
            const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4];
            uint32_t v0 = alignbit(a1, a0, sh), v1 = alignbit(a2, a1, sh), v2 = alignbit(a3, a2, sh), v3 = alignbit(a4, a3, sh);
            if (CLIPPED) { v0 &= msk[0]; v1 &= msk[1]; v2 &= msk[2]; v3 &= msk[3]; }
            sad = __builtin_amdgcn_sad_u8(v0, yu[r][0], sad);
            sad = __builtin_amdgcn_sad_u8(v1, yu[r][1], sad);
            sad = __builtin_amdgcn_sad_u8(v2, yu[r][2], sad);
            sad = __builtin_amdgcn_sad_u8(v3, yu[r][3], sad);
        }
    }
    return sad;
}

__global__ __launch_bounds__(256) void k_mc_search(const uint8_t* __restrict__ gray, size_t gstride, int T, int W, int H, int S, int BW,
                                                   int BH, int16_t* __restrict__ mv_fwd, int16_t* __restrict__ mv_bwd,
                                                   unsigned long long* __restrict__ resid)
{
    __shared__ uint32_t win[MC_WIN_ROWS * MC_WIN_PITCH / 4];
    __shared__ uint32_t cur[MC_NB * 64];
    __shared__ uint32_t part[MC_NB][1];
    const int dir = blockIdx.x & 1, grp = blockIdx.x >> 1, by = blockIdx.y, u = blockIdx.z;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bx = grp * MC_NB + wave;
    int16_t* mv = (dir ? mv_bwd : mv_fwd) + ((size_t)((size_t)u * BH + by) * BW) * 2;
    const int v = dir ? u - 1 : u + 1;
    if (v < 0 || v >= T) {                                  // F_{T-1} and Bk_0 are zero
        if (lane == 0 && bx < BW) { mv[2 * bx] = 0; mv[2 * bx + 1] = 0; }
        return;
    }
    const int x0 = grp * MC_NB * 16, y0 = by * 16;
    {   // Y_v's window: LDS (r, c) = Y_v(clamp(x0 - S + c), clamp(y0 - S + r)); columns past 64 + 2S are never selected
        const uint8_t* gv = gray + (size_t)v * gstride;
        uint8_t* wb = reinterpret_cast<uint8_t*>(win);
        const int wcols = 16 * MC_NB + 2 * S, wrows = 16 + 2 * S;
        for (int i = tid; i < wrows * wcols; i += 256) {
            const int r = i / wcols, c = i - r * wcols;
            const int yy = min(max(y0 - S + r, 0), H - 1), xx = min(max(x0 - S + c, 0), W - 1);
            wb[r * MC_WIN_PITCH + c] = gv[(size_t)yy * W + xx];
        }
        for (int i = tid; i < wrows * 4; i += 256) wb[(i >> 2) * MC_WIN_PITCH + wcols + (i & 3)] = 0;
        const uint8_t* gu = gray + (size_t)u * gstride;
        uint8_t* cb = reinterpret_cast<uint8_t*>(cur);
        for (int i = tid; i < MC_NB * 256; i += 256) {      // block w, row r, column c at cur byte w*256 + r*16 + c
            const int w = i >> 8, r = (i >> 4) & 15, c = i & 15;
            const int yy = y0 + r, xx = x0 + w * 16 + c;
            cb[i] = (yy < H && xx < W) ? gu[(size_t)yy * W + xx] : (uint8_t)0;
        }
    }
    __syncthreads();
    uint32_t best = 0xFFFFFFFFu;
    int pen = 0;
    const int n1 = 2 * S + 1;
    if (bx < BW) {
        uint32_t yu[16][4];
#pragma unroll
        for (int r = 0; r < 16; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) yu[r][j] = cur[wave * 64 + r * 4 + j];
        const int bw = min(16, W - bx * 16), bh = min(16, H - y0);
        pen = max((bw * bh) >> 2, 1);
        uint32_t msk[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = bw - 4 * j;                        // valid bytes of dword j
            msk[j] = k >= 4 ? 0xFFFFFFFFu : k <= 0 ? 0u : (1u << (8 * k)) - 1u;
        }
        const bool clipped = bw < 16 || bh < 16;
        for (int cand = lane; cand < n1 * n1; cand += 64) {
            const int cy = cand / n1, cx = cand - cy * n1;  // dy + S, dx + S
            const int colbyte = wave * 16 + cx;
            const uint32_t* wrow = win + cy * (MC_WIN_PITCH / 4);
            const uint32_t sad = clipped ? mc_block_sad<true>(wrow, colbyte >> 2, (colbyte & 3) * 8, yu, bh, msk)
                                         : mc_block_sad<false>(wrow, colbyte >> 2, (colbyte & 3) * 8, yu, bh, msk);
            const int adx = cx >= S ? cx - S : S - cx, ady = cy >= S ? cy - S : S - cy;
            const uint32_t key = (sad + (uint32_t)(pen * (adx + ady))) * 8192u + (uint32_t)cand;
            best = key < best ? key : best;
        }
    }
    best = wave_min_u32(best);
    uint32_t sad = 0;
    if (bx < BW) {
        const int cand = (int)(best & 8191u);
        const int cy = cand / n1, cx = cand - cy * n1;
        const int adx = cx >= S ? cx - S : S - cx, ady = cy >= S ? cy - S : S - cy;
        sad = (best >> 13) - (uint32_t)(pen * (adx + ady));
        if (lane == 0) { mv[2 * bx] = (int16_t)(cx - S); mv[2 * bx + 1] = (int16_t)(cy - S); }
    }
    if (dir) {                                              // resid[u]: the unpenalised SAD of Bk_u's choices, one atomic per workgroup
        const uint32_t t[1] = { sad };
        const unsigned long long r = block_sum_u64<MC_NB, 1>(t, lane, wave, tid, part);
        if (tid == 0) atomicAdd(resid + u, r);
    }
}

extern "C" int v3d_temporal_motion(const uint8_t* gray, size_t gray_stride, int T, int W, int H, int S, int c, int16_t* mv_fwd,
                                   int16_t* mv_bwd, unsigned long long* resid, uint8_t* cut_out, void* stream)
{
    if (!gray || !mv_fwd || !mv_bwd || !resid || !cut_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (T < 1 || T > 65535 || W < 1 || H < 1) { v3d_set_error("bad geometry T=%d %dx%d", T, W, H); return V3D_ERR_ARG; }
    if (S < 1 || S > MC_MAX_S) { v3d_set_error("motion search radius %d outside [1, %d]", S, MC_MAX_S); return V3D_ERR_ARG; }
    if (c < 0 || c > 256) { v3d_set_error("cut threshold %d outside [0, 256]", c); return V3D_ERR_ARG; }
    const size_t npx = (size_t)W * H;
    if (T > 1 && gray_stride < npx) { v3d_set_error("gray stride %zu below the frame size %zu", gray_stride, npx); return V3D_ERR_ARG; }
    if (((uintptr_t)resid & 7) != 0 || (((uintptr_t)mv_fwd | (uintptr_t)mv_bwd) & 1) != 0) {
        v3d_set_error("resid must be 8-byte aligned, the fields 2-byte aligned");
        return V3D_ERR_ARG;
    }
    const int BW = v3d_cdiv(W, 16), BH = v3d_cdiv(H, 16);
    if (BH > 65535) { v3d_set_error("frame %dx%d not supported", W, H); return V3D_ERR_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream;
    v3d_tp_launch_zero(resid, T, st);
    hipLaunchKernelGGL(k_mc_search, dim3(2 * v3d_cdiv(BW, MC_NB), BH, T), dim3(256), 0, st, gray, gray_stride, T, W, H, S, BW, BH, mv_fwd,
                       mv_bwd, resid);
    v3d_tp_launch_cutflag(resid, T, c, npx, cut_out, st);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
