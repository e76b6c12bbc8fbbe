// v3d_sgbm_cost.hip -- the SGBM's cost front end (a-4): x-Sobel pre-filter records of both images, then the Birchfield-Tomasi
// pixel cost summed over the 5x5 block into the 12-bit cost volume C (layout and codec: v3d_sgbm_internal.h).
#include "v3d_sgbm_internal.h"

// ------------------------------------------------------------------------------------------------
// a-4 (i): x-Sobel pre-filter + raw plane + Birchfield-Tomasi half-sample intervals, both images.
// ------------------------------------------------------------------------------------------------
// A workgroup owns 252 output columns (+2 halo each side, one thread per column) and marches down a band of rows:
// per row a thread loads ONE byte per image (the row entering the 3-row Sobel window), the x+-1 neighbours come
// from LDS, and the horizontal differences of the two older rows ride along in registers -- 2 byte loads per pixel
// instead of the 14 a one-row-per-workgroup version issues (that one was bound by its VMEM instruction count).
// The records trail the gradients by one row so that both LDS exchanges of a step share a single barrier.
#ifndef PF_BAND
#define PF_BAND 64
#endif
__global__ __launch_bounds__(256) void k_prefilter(const uint8_t* __restrict__ img1, const uint8_t* __restrict__ img2,
                                                   int W, int H, int pitch, size_t frame_stride, int ft,
                                                   uint4* __restrict__ rec)
{
    __shared__ uint8_t sI[2][2][256];              // [step parity][image][column] bytes of the entering row
    __shared__ unsigned short sGR[2][2][256];      // [step parity][image][column] grad | raw << 8 of the row one step back
    const int t = threadIdx.x, f = blockIdx.z;
    const int x = blockIdx.x * 252 - 2 + t;        // bytes valid for all t, gradients for t in [1, 254], records for [2, 253]
    const int xc = min(max(x, 0), W - 1);
    const bool xin = x > 0 && x < W - 1;           // else tab[0] = ft for both planes (OpenCV leaves the border columns at zero gradient)
    const int ya = blockIdx.y * PF_BAND, yb = min(ya + PF_BAND, H);
    const uint8_t* I0 = img1 + f * frame_stride + xc;
    const uint8_t* I1 = img2 + f * frame_stride + xc;
    auto ld = [&](int y) -> uint32_t {             // both images' bytes of row clamp(y), unconditional loads
        const size_t o = (size_t)min(max(y, 0), H - 1) * pitch;
        return (uint32_t)I0[o] | ((uint32_t)I1[o] << 8);
    };
    // rows clamp(ya-1) and ya prime the window; their horizontal differences need an exchange each
    int dm[2], d0[2], r0[2];                       // dh(row y-1), dh(row y), raw(row y) per image
    {
        const uint32_t vm = ld(ya - 1), v0 = ld(ya);
        sI[0][0][t] = (uint8_t)vm; sI[0][1][t] = (uint8_t)(vm >> 8);
        sI[1][0][t] = (uint8_t)v0; sI[1][1][t] = (uint8_t)(v0 >> 8);
        __syncthreads();
        const int tl = max(t - 1, 0), tr = min(t + 1, 255);
#pragma unroll
        for (int im = 0; im < 2; im++) {
            dm[im] = (int)sI[0][im][tr] - (int)sI[0][im][tl];
            d0[im] = (int)sI[1][im][tr] - (int)sI[1][im][tl];
            r0[im] = (v0 >> (8 * im)) & 0xFF;
        }
        __syncthreads();
    }
    uint32_t nxt = ld(ya + 1);
    int gp[2] = { 0, 0 }, rp[2] = { 0, 0 };         // grad / raw of the previous row (whose record is still owed)
    const int tl = max(t - 1, 0), tr = min(t + 1, 255);
    for (int y = ya; y <= yb; y++) {                // one extra step flushes the last row's record
        const int par = y & 1;
        const uint32_t ve = nxt;                    // row clamp(y+1)
        nxt = ld(y + 2);
        sI[par][0][t] = (uint8_t)ve; sI[par][1][t] = (uint8_t)(ve >> 8);
        sGR[par][0][t] = (unsigned short)(gp[0] | (rp[0] << 8));
        sGR[par][1][t] = (unsigned short)(gp[1] | (rp[1] << 8));
        __syncthreads();
        uint32_t out[4];
#pragma unroll
        for (int im = 0; im < 2; im++) {
            // ---- record of row y-1 from its own and its neighbours' (grad, raw) ----
            const int g = gp[im], r = rp[im];
            const int lo = sGR[par][im][tl], hi = sGR[par][im][tr];
            int gl = g, gr = g, rl = r, rr = r;
            if (x > 0) { gl = (g + (lo & 0xFF)) >> 1; rl = (r + (lo >> 8)) >> 1; }
            if (x < W - 1) { gr = (g + (hi & 0xFF)) >> 1; rr = (r + (hi >> 8)) >> 1; }
            const int g0 = min(min(gl, gr), g), g1 = max(max(gl, gr), g);
            const int q0 = min(min(rl, rr), r), q1 = max(max(rl, rr), r);
            out[2 * im] = (uint32_t)g | ((uint32_t)g0 << 8) | ((uint32_t)g1 << 16);
            out[2 * im + 1] = (uint32_t)r | ((uint32_t)q0 << 8) | ((uint32_t)q1 << 16);
            // ---- gradient of row y: 2*dh(y) + dh(y-1) + dh(y+1), rows replicated at the image border ----
            const int de = (int)sI[par][im][tr] - (int)sI[par][im][tl];
            const int dup = y > 0 ? dm[im] : d0[im];                        // row y-1 clamps to row 0
            const int ddn = y < H - 1 ? de : d0[im];                        // row y+1 clamps to row H-1
            gp[im] = xin ? min(max(2 * d0[im] + dup + ddn, -ft), ft) + ft : ft;
            rp[im] = xin ? r0[im] : ft;
            dm[im] = d0[im]; d0[im] = de; r0[im] = (ve >> (8 * im)) & 0xFF;
        }
        if (y > ya && t >= 2 && t <= 253 && x < W)
            st_stream(rec + ((size_t)f * H + (y - 1)) * W + x, make_uint4(out[0], out[1], out[2], out[3]));   // 1.1 GB per launch, read by the NEXT kernel: streaming (0.353 -> 0.325 ms)
    }
}

// ------------------------------------------------------------------------------------------------
// a-4 (ii,iii): BT pixel cost + 5x5 box sum -> C.  One workgroup = a strip of 60 output columns
// (+2 halo each side) marching down a band of rows; lane = (column, 8 disparities).
// Per row: BT cost bytes -> LDS row, 5-tap horizontal sum from LDS, 5-row vertical sum in registers.
// ------------------------------------------------------------------------------------------------
// strip geometry for LPC lanes per column (each lane owns 64/LPC disparities): 512 threads = 512/LPC columns,
// two halo columns each side; the right image needs 64 more staged records than the left
template <int LPC> struct CostGeo {
    static constexpr int EP = 64 / LPC, NP = EP / 2, COLS = 512 / LPC, OUT = COLS - 4, NREC = COLS + 64;
};
#ifndef V3D_COST_LPC
#define V3D_COST_LPC 8
#endif

__device__ __forceinline__ uint32_t bt_pair(uint32_t U, uint32_t U0, uint32_t U1, uint32_t V, uint32_t V0, uint32_t V1)
{
    // min(max(0, u - v1, v0 - u), max(0, v - u1, u0 - v)) on two disparities at once; all operands are 0..255, so
    // unsigned saturating subtracts give the max(0, .) for free: 7 packed ops
    const uint32_t a = pk_max(pk_subu_sat(U, V1), pk_subu_sat(V0, U));
    const uint32_t b = pk_max(pk_subu_sat(V, U1), pk_subu_sat(U0, V));
    return pk_min(a, b);
}

#ifndef V3D_COST_WAVES
#define V3D_COST_WAVES 6
#endif
template <int LPC>
__global__ __launch_bounds__(512, V3D_COST_WAVES) void k_cost(const uint4* __restrict__ rec,
                                              int W, int H, int W1, int lofs, int band_h, int P2, unsigned char* __restrict__ C, int xcd_order)
{
    typedef CostGeo<LPC> G;
    constexpr int EP = G::EP, NP = G::NP, COLS = G::COLS, OUT = G::OUT, NREC = G::NREC;
    typedef typename VecT<EP>::type vec_t;
    // right-image planes of one row, per quantity, as REVERSED u16 arrays (index grows with d) in two
    // alignments (copy 1 is copy 0 shifted by one element) so that the packed pair (d, d+1) is always an
    // aligned dword: no byte extraction in the hot loop.  Left-image values are stored pre-broadcast.
    // RCOPY (dwords between the copies) = 3 (mod 4) at LPC 8 / = 0 (mod 4) at LPC 16: the columns of one 32-lane
    // ds_read2_b32 group then fall on distinct LDS bank residues (measured: 48 -> 0 conflict cycles per wave-row).
    constexpr int RROW = (NREC + 4) / 2, RCOPY = 6 * RROW + (LPC == 8 ? 3 : 0), RBUF = 2 * RCOPY;
    __shared__ __attribute__((aligned(8))) uint32_t sRV[2 * RBUF];
    __shared__ __attribute__((aligned(8))) uint32_t sUL[2][COLS][6];
    __shared__ vec_t sPix[2][COLS][LPC];                        // BT cost of EP disparities as packed u16 pairs

    const int tid = threadIdx.x, col = tid / LPC, dq = tid % LPC;
    // XCD-aware tile order (v3d_common.h): neighbouring strips re-read each other's halo records (128 staged columns
    // per 60 outputs); on one XCD those re-reads hit its L2 (k_cost FETCH_SIZE -64 %, 2.2 -> 2.0 ms per 30 frames)
    int bxi = blockIdx.x, byi = blockIdx.y, bzi = blockIdx.z;
    if (xcd_order) xcd_tile(bxi, byi, bzi);
    const int xr0 = bxi * OUT;
    const int ys = byi * band_h, ye = min(ys + band_h, H);
    const int f = bzi;
    const uint32_t* rf = reinterpret_cast<const uint32_t*>(rec + (size_t)f * H * W);   // 4 dwords per pixel
    unsigned char* Cf = C + (size_t)f * c_frame(H, W1);
    static_assert(LPC == 8, "the store packs a lane's 8 disparities into one 12-byte field");

    const int xrc = min(max(xr0 - 2 + col, 0), W1 - 1);        // clamped cost-region column of this lane
    // staged record i <-> image column xr0 - 1 + i; reversed element k = NREC-1 - i.  d = EP*dq + j reads record
    // i0 - j with i0 = xrc - xr0 + 65 - EP*dq, i.e. reversed elements k0 + j, k0 = NREC-66 - (xrc - xr0) + EP*dq.
    const int k0 = NREC - 66 - (xrc - xr0) + EP * dq;
    const int rcopy = k0 & 1, rk = k0 - rcopy;                  // even element offset inside copy `rcopy`
    const int rv_off = rcopy * RCOPY + rk / 2;                  // dword offset of this lane's first pair (quantity 0, buffer 0)
    const bool out_col = (col >= 2) && (col < 2 + OUT) && (xr0 - 2 + col < W1);
    const int hc = min(max(col, 2), COLS - 3);                  // centre of the 5-tap window this lane sums
    const int nrows = (ye - ys) + 4;

    // Staging, spread over six of the eight waves (the workgroup moves at the pace of its slowest wave): a thread
    // owns HALF a record (dword 0 = gradient triple, dword 1 = raw triple).  Right image, threads 0..2*NREC-1:
    // record i and its left neighbour i-1 give the packed pair (element k, k+1) of three quantities with one
    // v_perm_b32 each, written as ONE dword to copy (k & 1) -- together the threads fill both copies.  Left
    // image, threads 256..256+2*COLS-1: three pre-broadcast dwords.  Records are fetched two rows ahead of
    // their use so the wait for row k+1's record can leave the youngest loads and the C stores of the last rows
    // in flight (vmcnt counts stores too on CDNA).
    // (A dedicated 9th staging wave was tried: 576-thread blocks drop a workgroup per CU and lose.)
    const int half = tid & 1, ri = tid >> 1, lt = (tid - 256) >> 1;
    const bool ld_right = ri < NREC, ld_left = tid >= 256 && lt < COLS;
    uint32_t ld_a = 0, ld_b = 0;                                // dword offsets inside a record row (uniform row base + these)
    int st_off = 0;                                             // dword offset of this thread's staging writes (buffer 0)
    if (ld_right) {
        ld_a = 4 * min(max(xr0 - 1 + ri, 0), W - 1) + 2 + half;
        ld_b = 4 * min(max(xr0 - 2 + ri, 0), W - 1) + 2 + half;
        const int k = NREC - 1 - ri;
        st_off = (k & 1) * RCOPY + 3 * half * RROW + (k >> 1);
    } else if (ld_left) {
        ld_a = ld_b = 4 * (min(max(xr0 - 2 + lt, 0), W1 - 1) + lofs) + half;      // lofs = 64 + minDisparity: cost column x1 <-> left image column x1 + lofs
        st_off = lt * 6 + 3 * half;
    }
    const bool ld_any = ld_right || ld_left;
    auto stage = [&](int b, uint2 rec) {                        // rec.x = own half-record, rec.y = left neighbour's
        if (ld_right) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                sRV[b * RBUF + st_off + j * RROW] = __builtin_amdgcn_perm(rec.y, rec.x, 0x0c000c00u | (uint32_t)j | ((uint32_t)(4 + j) << 16));
        } else if (ld_left) {
#pragma unroll
            for (int j = 0; j < 3; j++)
                (&sUL[b][0][0])[st_off + j] = __builtin_amdgcn_perm(rec.x, rec.x, 0x0c000c00u | (uint32_t)j | ((uint32_t)j << 16));
        }
    };
    // every VMEM instruction of the row loop is issued unconditionally (v3d_common.h: raw buffer access): threads
    // that stage nothing, halo columns and the warm-up rows are switched off through an out-of-range offset
    const __amdgpu_buffer_rsrc_t rs_rec = buf_rsrc(rf, (uint32_t)H * W * 16u), rs_c = buf_rsrc(Cf, (uint32_t)c_frame(H, W1));
    const uint32_t la = ld_any ? ld_a * 4u : V3D_BUF_OOB, lb = ld_any ? ld_b * 4u : V3D_BUF_OOB;   // + row offset < 2^31: bit 31 survives
    auto fetch = [&](int k) -> uint2 {
        const uint32_t ro = (uint32_t)min(max(ys - 2 + min(k, nrows - 1), 0), H - 1) * W * 16u;
        return make_uint2(buf_load_u32(rs_rec, ro + la), buf_load_u32(rs_rec, ro + lb));
    };
    if (ld_any) stage(0, fetch(0));
    // records in flight: nr[p] holds the row whose index has parity p; a slot is refilled (row + 2) right after the
    // stage that consumed it, so both are statically indexed and each load has two row times to land
    uint2 nr[2];
    nr[1] = fetch(1); nr[0] = fetch(2);
    __syncthreads();

    uint32_t ring[5][NP], vs[NP];                               // last five rows' horizontal sums + their running sum
#pragma unroll
    for (int j = 0; j < NP; j++) { vs[j] = 0u;                                // C holds the box sum alone; the readers add P2
#pragma unroll
        for (int i = 0; i < 5; i++) ring[i][j] = 0u; }
    // C store offsets: per-thread part (out-of-range marker for halo columns) + uniform row part
    const uint32_t st_col = out_col ? (uint32_t)((xr0 - 2 + col) * C_PXB + c_lane_off<EP>(dq)) : V3D_BUF_OOB;

    for (int k10 = 0; k10 < nrows; k10 += 10) {
#pragma unroll
      for (int s10 = 0; s10 < 10; s10++) {                      // ring slot and LDS buffer are compile-time: no register
        const int k = k10 + s10;                                // shifts, every LDS address is base + immediate
        if (k >= nrows) break;                                  // uniform
        const int slot = s10 % 5, buf = s10 & 1;

        // ---- BT cost of (xrc, d = EP*dq .. +EP-1) on row clamp(ys - 2 + k): quantities g, g_lo, g_hi, r, r_lo, r_hi ----
        // the two planes (gradient, raw) one after the other, fenced: all 6 x NP right-image dwords in flight at once
        // cost a dozen more registers than the 80 that three workgroups per CU leave
        uint32_t pix[NP];
#pragma unroll
        for (int pl = 0; pl < 2; pl++) {
            uint32_t U[3], V[3][NP];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                U[i] = sUL[buf][col][3 * pl + i];
                const uint32_t* pr = &sRV[buf * RBUF + rv_off + (3 * pl + i) * RROW];
#pragma unroll
                for (int j = 0; j < NP; j++) V[i][j] = pr[j];
            }
#pragma unroll
            for (int j = 0; j < NP; j++) {
                const uint32_t c = bt_pair(U[0], U[1], U[2], V[0][j], V[1][j], V[2][j]);
                pix[j] = pl == 0 ? c : pix[j] + pk_shr_u(c, 2);     // gradient + raw / 4; each half <= 93
            }
            if (pl == 0) { if (NP == 4) asm volatile("" : "+v"(pix[0]), "+v"(pix[1]), "+v"(pix[NP - 2]), "+v"(pix[NP - 1]) :: "memory");
                           else asm volatile("" : "+v"(pix[0]), "+v"(pix[NP - 1]) :: "memory"); }
        }
        sPix[buf][col][dq] = Packer<NP>::go(pix);

        if (k + 1 < nrows && ld_any) stage(buf ^ 1, nr[buf ^ 1]);     // row k+1 has parity buf^1 (k10 is even)
        nr[buf ^ 1] = fetch(k + 3);
        __syncthreads();

        // ---- 5-tap horizontal sum on packed u16 pairs, 5-row vertical running sum ----
        {
            uint32_t h[NP], w[NP];
            vec_unpack<NP>(sPix[buf][hc - 2][dq], h);               // (halo lanes re-sum a neighbour's window; never stored)
#pragma unroll
            for (int t = -1; t <= 2; t++) {
                vec_unpack<NP>(sPix[buf][hc + t][dq], w);
#pragma unroll
                for (int j = 0; j < NP; j++) h[j] += w[j];      // halves <= 5 * 189: no carry
            }
#pragma unroll
            for (int j = 0; j < NP; j++) { vs[j] += h[j] - ring[slot][j]; ring[slot][j] = h[j]; }   // add row k, drop row k - 5
            const uint32_t st_row = k >= 4 ? (uint32_t)c_row(ys + k - 4, W1) : V3D_BUF_OOB;     // uniform
            const uint32_t st_off = __builtin_elementwise_add_sat(st_col, st_row);                        // saturating: marker + marker stays out of range
            {   // 8 x 12 bits -> three dwords, one 12-byte store per lane (a wave's store covers 8 whole pixels: 768 contiguous bytes)
                uint32_t t[NP];
#pragma unroll
                for (int j = 0; j < NP; j++)                                                           // halves < 4096: 24 bits per pair = (vs & 0xFFF) | (vs >> 4 & ~0xFFF):
                    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(t[j]) : "s"(0xFFFu), "v"(vs[j]), "v"(vs[j] >> 4));   //   one shift + one bit-field insert (the compiler's own form takes three ops)
                // four 3-byte values -> three dwords, a v_perm_b32 each
                const v3d_u32x3_a4 pk = { __builtin_amdgcn_perm(t[1], t[0], 0x04020100u), __builtin_amdgcn_perm(t[2], t[1], 0x05040201u),
                                          __builtin_amdgcn_perm(t[NP - 1], t[2], 0x06050402u) };
                __builtin_amdgcn_raw_buffer_store_b96(pk, rs_c, st_off, 0, 2);    // streaming, like buf_store_stream
            }
        }
      }
    }
}

// parity-test export of C as int16 (v3d_sgbm_debug_cost_volume): 8 lanes per pixel, 8 disparities each
__global__ __launch_bounds__(256) void k_c_export(const unsigned char* __restrict__ C, size_t npx, int P2, int16_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, px = i >> 3;
    const int dl = (int)(i & 7);
    if (px >= npx) return;
    const uint4 v = c_unpack(*reinterpret_cast<const typename CRaw<8>::type*>(C + px * C_PXB + c_lane_off<8>(dl)), dl, pk_bcast(P2));
    *reinterpret_cast<uint4*>(out + px * V3D_D + 8 * dl) = v;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int sgbm_cost_volume(v3d_sgbm* h, const uint8_t* left, const uint8_t* right, int n, int W, int H, int pitch, size_t frame_stride, hipStream_t st)
{
    const int W1 = W - V3D_D;
    prof_mark(h, ST_PREFILTER, st);
    hipLaunchKernelGGL(k_prefilter, dim3(v3d_cdiv(W, 252), v3d_cdiv(H, PF_BAND), n), dim3(256), 0, st, left, right, W, H, pitch, frame_stride, h->ftzero, h->rec);
    prof_mark(h, ST_COST, st);
    constexpr int COST_OUT = CostGeo<V3D_COST_LPC>::OUT;
    hipLaunchKernelGGL((k_cost<V3D_COST_LPC>), dim3(v3d_cdiv(W1, COST_OUT), v3d_cdiv(H, h->cost_band), n), dim3(512), 0, st, h->rec, W, H, W1, V3D_D + h->prm.minDisparity, h->cost_band, h->P2, h->C, h->cost_xcd);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

int sgbm_export_cost(const v3d_sgbm* h, int W, int H, int16_t* C_out, hipStream_t st)
{
    const size_t npx = (size_t)(W - V3D_D) * H;
    hipLaunchKernelGGL(k_c_export, dim3((unsigned)((npx * 8 + 255) / 256)), dim3(256), 0, st, h->C, npx, h->P2, C_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
