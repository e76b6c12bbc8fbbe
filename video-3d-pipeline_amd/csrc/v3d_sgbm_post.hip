// v3d_sgbm_post.hip -- the SGBM's post-processing (a-6's right-view map, a-7, a-8): WTA records -> L-R check -> 3x3 median ->
// speckle filter.  Also the two public entries that need no handle: v3d_median3x3_i16 and v3d_filter_speckles.
#include "v3d_sgbm_internal.h"

// ------------------------------------------------------------------------------------------------
// a-8: medianBlur(3) on int16 with replicated borders (the invalid value takes part like any other).
// ------------------------------------------------------------------------------------------------
// The 19-exchange median-of-9 network: sort2(a, b) leaves (min, max) in (a, b); the median ends in p[4], which is returned.
// Run on int (one pixel) and on two int16 pixels packed in a dword.
struct sort2_int { __device__ __forceinline__ void operator()(int& a, int& b) const { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; } };
struct sort2_pk { __device__ __forceinline__ void operator()(uint32_t& a, uint32_t& b) const { const uint32_t lo = pk_min(a, b), hi = pk_max(a, b); a = lo; b = hi; } };
template <typename T, typename X>
__device__ __forceinline__ T median9(T (&p)[9], X sort2)
{
    sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]); sort2(p[0], p[1]);
    sort2(p[3], p[4]); sort2(p[6], p[7]); sort2(p[1], p[2]); sort2(p[4], p[5]);
    sort2(p[7], p[8]); sort2(p[0], p[3]); sort2(p[5], p[8]); sort2(p[4], p[7]);
    sort2(p[3], p[6]); sort2(p[1], p[4]); sort2(p[2], p[5]); sort2(p[4], p[7]);
    sort2(p[4], p[2]); sort2(p[6], p[4]); sort2(p[4], p[2]);
    return p[4];
}
__global__ __launch_bounds__(256) void k_median3x3(const int16_t* __restrict__ src, int W, int H, int16_t* __restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= W) return;
    const int16_t* s = src + (size_t)f * H * W;
    const int xm = max(x - 1, 0), xp = min(x + 1, W - 1);
    const int16_t* r0 = s + (size_t)max(y - 1, 0) * W;
    const int16_t* r1 = s + (size_t)y * W;
    const int16_t* r2 = s + (size_t)min(y + 1, H - 1) * W;
    int p[9] = { r0[xm], r0[x], r0[xp], r1[xm], r1[x], r1[xp], r2[xm], r2[x], r2[xp] };
    dst[(size_t)f * H * W + (size_t)y * W + x] = (int16_t)median9(p, sort2_int());
}

// the L-R check of a valid left-view disparity d1 (x16) at image column x against its row's right-view keys (min S << 6 | 63 - d,
// 0xFFFFFFFF = no source): stereosgbm.cpp invalidates the pixel when BOTH roundings of the disparity find a right-view disparity
// further than d12 away.  key(c) reads the key of image column c (a reader, not a pointer: an LDS array handed over as a pointer
// reaches the compiler as a generic address); x - da, x - db lie in [x - 63, x]: always inside the row
template <typename KEY>
__device__ __forceinline__ int lr_check(int d1, int x, int d12, KEY key)
{
    const int da = d1 >> 4, db = (d1 + 15) >> 4;
    const uint32_t ka = key(x - da), kb = key(x - db);
    const bool bad = (ka != 0xFFFFFFFFu) && (abs(63 - (int)(ka & 63u) - da) > d12) &&
                     (kb != 0xFFFFFFFFu) && (abs(63 - (int)(kb & 63u) - db) > d12);
    return bad ? V3D_INVALID16 : d1;
}

// ------------------------------------------------------------------------------------------------
// a-6 (right-view map) + a-7 + a-8: disp2, L-R check and 3x3 median in one launch.
//
// The WTA tail leaves ONE 32-bit record per cost-region pixel (wta_word): min S, the sub-pixel disparity and the
// winning d.  OpenCV's right-view map -- disp2[x2] = the d of the cheapest pixel x with x - d == x2, later-processed
// (smaller) x losing ties -- is the minimum of the keys (min S << 6 | 63 - d) over the 64 source pixels x2 .. x2 + 63.
// Rounds 1-2 formed it with a global atomicMin per pixel inside the WTA tail (60 M L2 atomics per 30 frames: 0.3 ms of
// k_hfused's 4.9, measured by a build without them); now a block of this kernel stages the records of 256 source
// columns x 18 rows ONCE (coalesced dword loads instead of two gathers per pixel), min-scatters their keys into an
// LDS row of right-view targets (ds_min_u32), and checks / medians out of LDS.  Same minimum over the same key set:
// bit-identical, schedule-independent.
// Tile: 128 x 16 outputs + a one-pixel ring; sources x0 - 64 .. x0 + 191 (one per thread), targets x0 - 64 .. x0 + 128.
// ------------------------------------------------------------------------------------------------
#define LRM_TX 128
#define LRM_TY 16
#define LRM_NS (LRM_TX + 2 * V3D_D)        // source columns per row  (256 = one per thread)
#define LRM_NT (LRM_TX + V3D_D + 1)        // right-view targets per row
template <bool MED>
__global__ __launch_bounds__(256) void k_lrcheck_median(const uint32_t* __restrict__ wta, int W, int H, int d12, int m, int16_t* __restrict__ out)
{
    static_assert(LRM_NS == 256, "one source column per thread");
    constexpr int NR = LRM_TY + 2;
    __shared__ uint32_t sW[NR][LRM_NS];
    __shared__ uint32_t sD2[NR][LRM_NT + 3];
    __shared__ short sT[NR][LRM_TX + 2];
    const int t = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * LRM_TX, y0 = blockIdx.y * LRM_TY;
    const size_t fo = (size_t)f * H * W;
    // minDisparity m <= 0: the records, the keys and the check live in RELATIVE columns xr = x1 + 64 (what the WTA tail wrote);
    // output column x shows relative column x - m, columns whose x - m falls outside [64, W) are invalid, and the value
    // written last is relative + 16 m (invalid: -16 + 16 m = 16 (m - 1)); the median commutes with the constant
    const int xbase = x0 - m - V3D_D;                                        // relative column of source / target index 0
    // ---- 1. this thread's source column, all rows in flight together (unconditional loads from clamped addresses;
    //         columns left of the cost region were never written: masked below) ----
    const int xs = xbase + t;
    const bool src_in = xs >= V3D_D && xs < W;
    const int xsc = min(max(xs, 0), W - 1);
    uint32_t wv[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) wv[r] = wta[fo + (size_t)min(max(y0 - 1 + r, 0), H - 1) * W + xsc];   // replicated image border
    for (int i = t; i < NR * (LRM_NT + 3); i += 256) (&sD2[0][0])[i] = 0xFFFFFFFFu;
    __syncthreads();
    // ---- 2. records -> LDS, keys -> min-scatter at target x - d ----
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const uint32_t v = src_in ? wv[r] : 0u;
        sW[r][t] = v;
        const int best = (int)(v & 63u), i = t - best;                        // target column xs - best
        if ((v & 0x1FFC0u) != 0u && i >= 0 && i < LRM_NT) atomicMin(&sD2[r][i], ((v >> 17) << 6) | (uint32_t)(63 - best));
    }
    __syncthreads();
    // ---- 3. L-R check of the tile + ring (stereosgbm.cpp: both roundings of the disparity must disagree) ----
    constexpr int NIT = (NR * (LRM_TX + 2) + 255) / 256;
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int i = t + 256 * it;
        if (i < NR * (LRM_TX + 2)) {
            const int ty = i / (LRM_TX + 2), tx = i - ty * (LRM_TX + 2);
            const int x = min(max(x0 - 1 + tx, 0), W - 1);
            const int xr = x - m;
            int d1 = V3D_INVALID16;
            if (xr >= V3D_D && xr < W) {
                d1 = wta_d16(sW[ty][xr - xbase]);
                if (d1 != V3D_INVALID16) d1 = lr_check(d1, xr, d12, [&](int c) { return sD2[ty][c - xbase]; });
            }
            sT[ty][tx] = (short)d1;
        }
    }
    __syncthreads();
    // ---- 4. 3x3 median (19-exchange network), 8 outputs per thread ----
    const int tx = t & (LRM_TX - 1), x = x0 + tx;
    if (x >= W) return;
#pragma unroll
    for (int ty = t >> 7; ty < LRM_TY; ty += 2) {
        const int y = y0 + ty;
        if (y >= H) break;
        if (!MED) { out[fo + (size_t)y * W + x] = (int16_t)(sT[ty + 1][tx + 1] + 16 * m); continue; }
        int p[9] = { sT[ty][tx], sT[ty][tx + 1], sT[ty][tx + 2], sT[ty + 1][tx], sT[ty + 1][tx + 1], sT[ty + 1][tx + 2],
                     sT[ty + 2][tx], sT[ty + 2][tx + 1], sT[ty + 2][tx + 2] };
        out[fo + (size_t)y * W + x] = (int16_t)(median9(p, sort2_int()) + 16 * m);
    }
}

// ------------------------------------------------------------------------------------------------
// The same three steps as a ROW MARCH (round 3; the default for even W <= 4096).  The tile form above stages 256 source columns x 18
// rows for 128 x 16 outputs: every record is fetched 2.25 times, and a block's 36 KB of LDS leave few blocks per CU.  Here
// a 256-thread block owns a band of rows at the full image width and marches down it: per row each thread loads its own
// records (coalesced, every record read once per band + 2 halo rows per band), the right-view keys are min-scattered into ONE
// LDS row, the checked disparities go into a three-row LDS ring and the median of the previous row comes out of it.  10 bytes
// of LDS per column (19 KB at 1920), the next row's records fly while the current row is processed.  Same minimum over the
// same key set, same median network (run on two adjacent outputs at once in packed int16): bit-identical to the tile form.
// ------------------------------------------------------------------------------------------------
#define LRR_BAND 15
template <bool MED, int NPP>      // NPP: pixel PAIRS per thread and row (columns 2t, 2t+1, 2t + 512, ...): 4 covers W <= 2048, 8 W <= 4096; W even
__global__ __launch_bounds__(256) void k_lrcheck_median_rows(const uint32_t* __restrict__ wta, int W, int H, int d12, int m, int16_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lrr_smem[];
    uint32_t* sD2 = reinterpret_cast<uint32_t*>(lrr_smem);                    // [W] right-view keys of the current row
    uint32_t* sT = reinterpret_cast<uint32_t*>(lrr_smem + (size_t)W * 4);     // [3][W/2] checked disparities, two per word: ring of rows
    const int t = threadIdx.x, f = blockIdx.z, W2 = W >> 1;
    const int ya = blockIdx.x * LRR_BAND, yb = min(ya + LRR_BAND, H);
    const size_t fo = (size_t)f * H * W;
    auto load_row = [&](int y, uint2 (&r)[NPP]) {                              // records of image row clamp(y); columns < 64 were never written
        const uint2* src = reinterpret_cast<const uint2*>(wta + fo + (size_t)min(max(y, 0), H - 1) * W);
#pragma unroll
        for (int i = 0; i < NPP; i++) r[i] = src[min(t + 256 * i, W2 - 1)];
    };
    uint2 nx[NPP];
    const int y_first = MED ? ya - 1 : ya, y_last = MED ? yb : yb - 1;
    load_row(y_first, nx);
    // rows ya-1 .. yb (median needs a row above and below; replicated at the image border = the clamped load)
    for (int y = y_first; y <= y_last; y++) {
        uint32_t rec[2 * NPP];
#pragma unroll
        for (int i = 0; i < NPP; i++) {
            const int x = 2 * (t + 256 * i);
            rec[2 * i] = (x >= V3D_D && x < W) ? nx[i].x : 0u; rec[2 * i + 1] = (x >= V3D_D && x < W) ? nx[i].y : 0u;
        }
        load_row(y + 1, nx);                                                   // the next row's records fly during this row (clamped: always in range)
        for (int x = t; x < W; x += 256) sD2[x] = 0xFFFFFFFFu;
        __syncthreads();
        // ---- right-view keys: the d of the cheapest source pixel of every target column (ties: larger d), by LDS min-scatter ----
#pragma unroll
        for (int i = 0; i < 2 * NPP; i++) {
            const uint32_t v = rec[i];
            const int best = (int)(v & 63u);
            if ((v & 0x1FFC0u) != 0u) atomicMin(&sD2[2 * (t + 256 * (i >> 1)) + (i & 1) - best], ((v >> 17) << 6) | (uint32_t)(63 - best));
        }
        __syncthreads();
        // ---- L-R check (stereosgbm.cpp: both roundings of the disparity must disagree) ----
        // minDisparity m <= 0 (see k_lrcheck_median): a thread checks its own RELATIVE columns xr and places the result at output
        // column xr + m; the 64 relative columns left of the cost region carry no record and fill the output columns no
        // relative column lands on, [0, 64 + m) and [W + m, W), with the invalid value.  64, W and an even m keep a pair (xr, xr + 1)
        // a pair: one 32-bit write; an odd m splits it over two words: two 16-bit writes
        uint32_t* row = sT + (size_t)((y + 3) % 3) * W2;
#pragma unroll
        for (int i = 0; i < NPP; i++) {
            const int x0 = 2 * (t + 256 * i);
            if (x0 < W) {
                int dd[2];
#pragma unroll
                for (int n = 0; n < 2; n++) {
                    const int xr = x0 + n;
                    int d1 = V3D_INVALID16;
                    if (xr >= V3D_D) {
                        d1 = wta_d16(rec[2 * i + n]);
                        if (d1 != V3D_INVALID16) d1 = lr_check(d1, xr, d12, [sD2](int c) { return sD2[c]; });
                    }
                    dd[n] = d1;
                }
                auto place = [&](int xr) { return xr >= V3D_D ? xr + m : (xr < V3D_D + m ? xr : xr - V3D_D + W); };   // output column of relative column xr
                if (!MED) {
                    out[fo + (size_t)y * W + place(x0)] = (int16_t)(dd[0] + 16 * m); out[fo + (size_t)y * W + place(x0 + 1)] = (int16_t)(dd[1] + 16 * m);
                } else if ((m & 1) == 0) {                                    // uniform
                    row[place(x0) >> 1] = ((uint32_t)dd[0] & 0xFFFFu) | ((uint32_t)dd[1] << 16);
                } else {
                    short* row16 = reinterpret_cast<short*>(row);
                    row16[place(x0)] = (short)dd[0]; row16[place(x0 + 1)] = (short)dd[1];
                }
            }
        }
        __syncthreads();
        if (!MED) continue;
        // ---- 3x3 median of row y-1 from ring rows y-2, y-1, y: two adjacent outputs per 19-exchange network in packed int16 ----
        const int yo = y - 1;
        if (yo >= ya && yo < yb) {                                             // uniform
            // at the image border the missing row is the replicated one: row -1 was loaded as row 0, row H as row H-1
            const uint32_t* rr[3] = { sT + (size_t)((yo - 1 + 3) % 3) * W2, sT + (size_t)((yo + 3) % 3) * W2, sT + (size_t)((yo + 1 + 3) % 3) * W2 };
#pragma unroll
            for (int i = 0; i < NPP; i++) {
                const int xw = t + 256 * i;                                    // word index: outputs 2 xw, 2 xw + 1
                if (xw < W2) {
                    uint32_t p[9];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const uint32_t w0 = rr[r][xw];
                        const uint32_t wl = xw > 0 ? rr[r][xw - 1] : (w0 << 16);              // column -1 replicates column 0
                        const uint32_t wr = xw + 1 < W2 ? rr[r][xw + 1] : (w0 >> 16);         // column W replicates column W-1
                        p[3 * r] = alignbit(w0, wl, 16); p[3 * r + 1] = w0; p[3 * r + 2] = alignbit(wr, w0, 16);   // (x-1, x), (x, x+1), (x+1, x+2)
                    }
                    *reinterpret_cast<uint32_t*>(out + fo + (size_t)yo * W + 2 * xw) = pk_add(median9(p, sort2_pk()), pk_bcast(16 * m));    // relative -> true disparity at the last write
                }
            }
        }
        // (no barrier here: the next trip first refills sD2 -- its last readers finished before the barrier above -- and overwrites
        //  ring row (y+1) % 3, the row this median read as its first, only behind its own two barriers)
    }
}

int sgbm_lrcheck_median(const v3d_sgbm* h, int n, int W, int H, int16_t* out, bool med, hipStream_t st)
{
    const uint32_t* wta = h->wta;
    const int d12 = h->d12, m = h->prm.minDisparity;
    // the row march reads record pairs and writes disparity pairs: even widths, 8-byte aligned buffers
    const bool rows_ok = !h->lrm_tiles && W <= 4096 && (W & 1) == 0 && (reinterpret_cast<uintptr_t>(wta) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
    if (rows_ok) {
        const dim3 grid(v3d_cdiv(H, LRR_BAND), 1, n);
        const size_t smem = (size_t)W * 4 + (size_t)3 * (W / 2) * 4;
        if (W <= 2048) {
            if (med) hipLaunchKernelGGL((k_lrcheck_median_rows<true, 4>), grid, dim3(256), smem, st, wta, W, H, d12, m, out);
            else hipLaunchKernelGGL((k_lrcheck_median_rows<false, 4>), grid, dim3(256), smem, st, wta, W, H, d12, m, out);
        } else {
            if (med) hipLaunchKernelGGL((k_lrcheck_median_rows<true, 8>), grid, dim3(256), smem, st, wta, W, H, d12, m, out);
            else hipLaunchKernelGGL((k_lrcheck_median_rows<false, 8>), grid, dim3(256), smem, st, wta, W, H, d12, m, out);
        }
    } else {
        const dim3 grid(v3d_cdiv(W, LRM_TX), v3d_cdiv(H, LRM_TY), n);
        if (med) hipLaunchKernelGGL(k_lrcheck_median<true>, grid, dim3(256), 0, st, wta, W, H, d12, m, out);
        else hipLaunchKernelGGL(k_lrcheck_median<false>, grid, dim3(256), 0, st, wta, W, H, d12, m, out);
    }
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ------------------------------------------------------------------------------------------------
// a-8: filterSpeckles as run-based connected-component labelling.  Components are the 4-connected
// sets of valid pixels joined where |a - b| <= maxDiff; components of at most maxSpeckleSize pixels
// are invalidated.  (1) every row is cut into horizontal runs by a block-wide scan (no atomics);
// a run is named by the index of its first pixel, carries its length, and is appended to its row's
// RUN LIST.  (2) runs of adjacent rows are joined with a lock-free union-find, one union per overlapping
// run pair instead of one per pixel.  (3) run lengths are added at the roots, (4) small components are
// erased -- (3) and (4) walk the run lists (tens of runs per row), not the pixels.
// The outcome is schedule-independent: union-find yields the same partition in any order, and
// sizes are only ever compared against the threshold.
//   lab  [n]: run start for non-start pixels (constant); parent pointer for run starts; -1 invalid   (dense)
//   runs [n]: per row, the run starts of that row in x order, ended by -1 if the row has fewer than W runs
//   csz  [n]: at run starts only: the run's length, and at a root the running size of its component
// Dense traffic per pixel: img read + lab write (k_ccl_runs), two img rows read (k_ccl_vmerge); the round-1 form also
// wrote and re-read dense length / size planes and re-read lab per pixel (~40 B per pixel, 0.81 ms per 30 frames).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int ccl_ld(const int* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ccl_find(const int* L, int i)
{
    int p = ccl_ld(L, i);
    while (p != i) { i = p; p = ccl_ld(L, i); }
    return i;
}
// find with path halving: every visited node is re-pointed at its grandparent.  Safe next to concurrent
// atomicMin hooks: a node is only ever re-pointed at one of its own ancestors, never at a slot seen as a root.
__device__ __forceinline__ int ccl_find_halve(int* L, int i)
{
    for (;;) {
        const int p = ccl_ld(L, i);
        if (p == i) return i;
        const int gp = ccl_ld(L, p);
        if (gp == p) return p;
        __hip_atomic_store(L + i, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = gp;
    }
}
__device__ __forceinline__ void ccl_union(int* L, int a, int b)
{
    for (;;) {
        a = ccl_find_halve(L, a); b = ccl_find_halve(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang the larger root under the smaller
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;                                               // a was re-rooted meanwhile: carry on from its old parent
    }
}
__device__ __forceinline__ bool ccl_conn(int a, int b, int newVal, int maxDiff) { return a != newVal && b != newVal && abs(a - b) <= maxDiff; }

// one WAVE per image row (four rows per block), 256 pixels per step -- FOUR consecutive pixels per lane (one 8-byte load,
// one 16-byte label store): "latest run start at or before x" is a 3-step max inside the lane + an inclusive max-scan of
// the lane totals over the wave (DPP row shifts + row broadcasts, no LDS), "run starts before x" four ballots + popcounts;
// the carry from step to step rides in SGPRs, no barrier.  A 1920-pixel row is 8 steps.  (Round 2's one-pixel-per-lane
// form ran 30 steps per row with six ds_bpermute exchanges each: 0.157 ms per 30 frames.)
#define V3D_DPP_ROW_BCAST15 0x142
#define V3D_DPP_ROW_BCAST31 0x143
__device__ __forceinline__ uint32_t wave_incl_max_u32(uint32_t v)      // inclusive max-scan over the 64 lanes, identity 0
{
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(1)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(2)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(4)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(8)>(0u, v));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, V3D_DPP_ROW_BCAST15, 0xA, 0xF, false));   // rows 1, 3 take lane 15 / 47
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, V3D_DPP_ROW_BCAST31, 0xC, 0xF, false));   // rows 2, 3 take lane 31
    return v;
}
__global__ __launch_bounds__(256) void k_ccl_runs(const int16_t* __restrict__ img, int W, int H, int newVal, int maxDiff,
                                                  int* __restrict__ lab, int* __restrict__ runs, int* __restrict__ csz)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;                                        // wave-uniform
    const size_t fo = (size_t)blockIdx.z * W * H + (size_t)y * W;
    const int16_t* row = img + fo;
    const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(img) & 7) | (reinterpret_cast<uintptr_t>(lab) & 15)) == 0;   // rows (and frames) start aligned: vector loads / stores
    int carry = 0, nrun = 0;                                   // (latest run start so far) + 1, runs so far (wave-uniform)
    int last_v = newVal;                                       // value of the pixel left of this step's first one
    auto ld4 = [&](int x0, int (&v)[4]) {                      // pixels x0 .. x0+3 (newVal beyond the row)
        if (vec) {
            if (x0 < W) { const uint2 t = *reinterpret_cast<const uint2*>(row + x0);
                          v[0] = (short)(t.x & 0xFFFFu); v[1] = (short)(t.x >> 16); v[2] = (short)(t.y & 0xFFFFu); v[3] = (short)(t.y >> 16); }
            else { v[0] = v[1] = v[2] = v[3] = newVal; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = x0 + k < W ? (int)row[x0 + k] : newVal;
        }
    };
    int nx[4];
    ld4(4 * lane, nx);
    for (int xs = 0; xs < W; xs += 256) {
        const int x0 = xs + 4 * lane;
        int v[4] = { nx[0], nx[1], nx[2], nx[3] };
        ld4(x0 + 256, nx);                                     // next step's pixels fly during this step
        // neighbours across the lane boundary: left of v[0] = lane-1's v[3], right of v[3] = lane+1's v[0]
        int pv = __shfl_up(v[3], 1), nv = __shfl_down(v[0], 1);
        const int vn0 = __builtin_amdgcn_readfirstlane(nx[0]); // first pixel of the next step
        pv = lane == 0 ? last_v : pv;
        nv = lane == 63 ? vn0 : nv;
        last_v = __builtin_amdgcn_readlane(v[3], 63);
        bool valid[4], start[4];
        uint32_t c[4];                                         // inclusive (latest start + 1) inside the lane
#pragma unroll
        for (int k = 0; k < 4; k++) {
            valid[k] = x0 + k < W && v[k] != newVal;
            start[k] = valid[k] && !ccl_conn(k ? v[k - 1] : pv, v[k], newVal, maxDiff);
            const uint32_t m = start[k] ? (uint32_t)(x0 + k + 1) : 0u;
            c[k] = k ? max(c[k - 1], m) : m;
        }
        const uint32_t incl = wave_incl_max_u32(c[3]);
        uint32_t excl = (uint32_t)__shfl_up((int)incl, 1);
        excl = max(lane == 0 ? 0u : excl, (uint32_t)carry);    // latest start + 1 left of this lane's pixels
        carry = max(carry, (int)__builtin_amdgcn_readlane((int)incl, 63));
        int before = nrun;                                     // run starts left of this lane's pixels
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long sm = __builtin_amdgcn_ballot_w64(start[k]);
            before += __popcll(sm & ((1ull << lane) - 1ull));
            nrun += __popcll(sm);
        }
        int labv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int cur = (int)max(c[k], excl) - 1;          // run start of pixel x0+k (if valid)
            labv[k] = valid[k] ? y * W + cur : -1;
            if (start[k]) { runs[fo + before] = y * W + x0 + k; before++; }
            const int right = k < 3 ? v[k + 1] : nv;
            if (valid[k] && !(x0 + k + 1 < W && ccl_conn(v[k], right, newVal, maxDiff))) csz[fo + cur] = x0 + k - cur + 1;   // the run's last pixel: its length
        }
        if (vec) { if (x0 < W) *reinterpret_cast<int4*>(lab + fo + x0) = make_int4(labv[0], labv[1], labv[2], labv[3]); }
        else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (x0 + k < W) lab[fo + x0 + k] = labv[k];
        }
    }
    if (lane == 0 && nrun < W) runs[fo + nrun] = -1;           // end of the row's run list
}

// Two launches: LEVEL 0 joins the row pairs inside bands of VM_BAND rows (trees at most VM_BAND deep), LEVEL 1 the
// band boundaries.  The partition is the same in any order; what changes is the depth of the parent chains the
// racing unions build, i.e. how many dependent global loads a find costs.
// A thread tests EIGHT consecutive pixels of a row pair (two 16-byte loads + the pair left of them); one wave covers 512
// columns.  (Round 2's one-pixel-per-thread form launched a million 30-instruction waves per batch: 0.21 ms per 30 frames,
// bound by wave launch, not by its loads.)
#ifndef VM_BAND
#define VM_BAND 16
#endif
template <int LEVEL>
__global__ __launch_bounds__(64) void k_ccl_vmerge(const int16_t* __restrict__ img, int W, int H, int newVal, int maxDiff, int* __restrict__ lab)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    const int y = LEVEL == 0 ? blockIdx.y + blockIdx.y / (VM_BAND - 1) : blockIdx.y * VM_BAND + VM_BAND - 1;
    if (x0 >= W || y + 1 >= H) return;
    const size_t fo = (size_t)blockIdx.z * W * H;
    const int16_t* im = img + fo; int* L = lab + fo;
    const int i0 = y * W + x0;
    int v[9], u[9];                                            // [0] = the pixel pair left of this thread's eight (itself at x0 = 0)
    v[0] = im[i0 - (x0 > 0 ? 1 : 0)]; u[0] = im[i0 + W - (x0 > 0 ? 1 : 0)];
    if ((W & 7) == 0 && (reinterpret_cast<uintptr_t>(img) & 15) == 0) {   // rows start 16-byte aligned
        const uint4 a = *reinterpret_cast<const uint4*>(im + i0), b = *reinterpret_cast<const uint4*>(im + i0 + W);
        const uint32_t aw[4] = { a.x, a.y, a.z, a.w }, bw[4] = { b.x, b.y, b.z, b.w };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[1 + 2 * k] = (short)(aw[k] & 0xFFFFu); v[2 + 2 * k] = (short)(aw[k] >> 16);
            u[1 + 2 * k] = (short)(bw[k] & 0xFFFFu); u[2 + 2 * k] = (short)(bw[k] >> 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++) { const int xc = min(x0 + k, W - 1) - x0; v[1 + k] = im[i0 + xc]; u[1 + k] = im[i0 + W + xc]; }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (x0 + k >= W) break;
        if (!ccl_conn(v[1 + k], u[1 + k], newVal, maxDiff)) continue;
        // the pixel to my left joins the same two runs: it (or one further left) does the union
        if (x0 + k > 0 && ccl_conn(v[k], u[k], newVal, maxDiff) && ccl_conn(v[k], v[1 + k], newVal, maxDiff) && ccl_conn(u[k], u[1 + k], newVal, maxDiff)) continue;
        ccl_union(L, L[i0 + k], L[i0 + k + W]);
    }
}

// (3) and (4): one WAVE per image row walks that row's run list, 64 runs per step.
// count: every non-root run adds its length to its root (a root's own length is already there).  Only "<= maxSize or
// not" matters: stop adding once the root is known to be large.
__global__ __launch_bounds__(256) void k_ccl_count(int W, int H, int maxSize, int* __restrict__ lab, const int* __restrict__ runs, int* __restrict__ csz)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;                                        // wave-uniform
    const size_t fo = (size_t)blockIdx.z * W * H;
    int* L = lab + fo; int* C = csz + fo;
    const int* rl = runs + fo + (size_t)y * W;
    for (int k0 = 0; k0 < W; k0 += 64) {
        const int k = k0 + lane;
        const int s = k < W ? rl[k] : -1;
        // entries behind the end marker are stale: a lane counts only if every entry before it in this step is a run
        const unsigned long long endm = __builtin_amdgcn_ballot_w64(s < 0);
        const int first_end = endm ? __builtin_ctzll(endm) : 64;
        if (lane < first_end) {
            const int r = ccl_find(L, s);
            if (r != s) {
                L[s] = r;                                      // path compression (the forest is final here)
                if (__hip_atomic_load(C + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= maxSize) atomicAdd(C + r, C[s]);
            }
        }
        if (first_end < 64) break;                             // wave-uniform
    }
}

// apply: a run whose component is small is overwritten pixel by pixel (at most maxSize of them: the loop is short and rare)
__global__ __launch_bounds__(256) void k_ccl_apply(int16_t* __restrict__ img, int W, int H, int newVal, int maxSize,
                                                   const int* __restrict__ lab, const int* __restrict__ runs, const int* __restrict__ csz)
{
    const int y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;                                        // wave-uniform
    const size_t fo = (size_t)blockIdx.z * W * H;
    const int* L = lab + fo;
    const int* rl = runs + fo + (size_t)y * W;
    const int row_end = (y + 1) * W;
    for (int k0 = 0; k0 < W; k0 += 64) {
        const int k = k0 + lane;
        const int s = k < W ? rl[k] : -1;
        const unsigned long long endm = __builtin_amdgcn_ballot_w64(s < 0);
        const int first_end = endm ? __builtin_ctzll(endm) : 64;
        if (lane < first_end) {
            const int r = ccl_find(L, s);
            if (csz[fo + r] <= maxSize) {
                img[fo + s] = (int16_t)newVal;
                for (int i = s + 1; i < row_end && L[i] == s; i++) img[fo + i] = (int16_t)newVal;    // non-start pixels carry their run's start
            }
        }
        if (first_end < 64) break;                             // wave-uniform
    }
}

// the five launches; ws = 3 * n_pixels * frames int32
static int launch_speckles(int16_t* img, int W, int H, int frames, int newVal, int maxSize, int maxDiff, int32_t* ws, hipStream_t st)
{
    const int px = W * H;
    int* lab = ws; int* runs = ws + (size_t)px * frames; int* csz = ws + (size_t)px * frames * 2;
    hipLaunchKernelGGL(k_ccl_runs, dim3(v3d_cdiv(H, 4), 1, frames), dim3(256), 0, st, img, W, H, newVal, maxDiff, lab, runs, csz);
    // rows y with (y % VM_BAND) != VM_BAND-1 first (blockIdx.y enumerates them), then the band boundaries
    hipLaunchKernelGGL(k_ccl_vmerge<0>, dim3(v3d_cdiv(W, 512), H - H / VM_BAND, frames), dim3(64), 0, st, img, W, H, newVal, maxDiff, lab);
    if (H / VM_BAND > 0) hipLaunchKernelGGL(k_ccl_vmerge<1>, dim3(v3d_cdiv(W, 512), H / VM_BAND, frames), dim3(64), 0, st, img, W, H, newVal, maxDiff, lab);
    hipLaunchKernelGGL(k_ccl_count, dim3(v3d_cdiv(H, 4), 1, frames), dim3(256), 0, st, W, H, maxSize, lab, runs, csz);
    hipLaunchKernelGGL(k_ccl_apply, dim3(v3d_cdiv(H, 4), 1, frames), dim3(256), 0, st, img, W, H, newVal, maxSize, lab, runs, csz);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

int sgbm_speckles(const v3d_sgbm* h, int16_t* out, int n, int W, int H, hipStream_t st)
{
    if (h->prm.speckleWindowSize <= 0) return V3D_OK;
    const int newVal = (h->prm.minDisparity - 1) * 16, maxDiff = 16 * h->prm.speckleRange, maxSize = h->prm.speckleWindowSize;
    return launch_speckles(out, W, H, n, newVal, maxSize, maxDiff, h->labels, st);
}

extern "C" int v3d_median3x3_i16(const int16_t* src, int W, int H, int16_t* dst, void* stream)
{
    if (!src || !dst || W < 1 || H < 1) { v3d_set_error("bad argument"); return V3D_ERR_ARG; }
    hipLaunchKernelGGL(k_median3x3, dim3(v3d_cdiv(W, 256), H, 1), dim3(256), 0, (hipStream_t)stream, src, W, H, dst);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_filter_speckles(int16_t* img, int W, int H, int newVal, int maxSize, int maxDiff, int32_t* ws, void* stream)
{
    if (!img || !ws || W < 1 || H < 1) { v3d_set_error("bad argument"); return V3D_ERR_ARG; }
    return launch_speckles(img, W, H, 1, newVal, maxSize, maxDiff, ws, (hipStream_t)stream);
}
