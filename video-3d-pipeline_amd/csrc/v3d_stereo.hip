// v3d_stereo.hip -- depth-image-based rendering (DIBR): 4K BGR frame + its u16 depth -> side-by-side stereo pair.
//
// The warp is purely horizontal, so every row is independent.  One workgroup of 256 threads marches a band of ST_BAND rows;
// the next row's depth and BGR bytes are in flight (16-byte loads into registers) while the current row is rendered in LDS:
//   1. stage: the row's aligned 16-byte chunks -> sD (depth), sF (BGR); both eyes' key rows sZ zeroed;
//   2. scatter: every source pixel x, per eye: t = x + floor((g (D - conv) + 2^23) / 2^24); ds_max_u32 of
//      (D << 16) | (x + 1) into sZ[eye][t] -- order-independent, so the result does not depend on scheduling;
//   3. scan: thread t owns PPT consecutive targets; "last key left of my run" is a max-scan of (index + 1) over the threads,
//      "first key right of my run" a max-scan of (WP - index) in the other direction (wave shuffles, then the four wave
//      totals through LDS);
//   4. fill + gather: holes take the farther neighbour (background extends into disocclusions), colours come from sF,
//      half SBS averages pairs in registers, and each thread writes its run with the widest aligned stores.
// Contract: tests/stereo_ref.py (bit-exact).  Resources and measured numbers: DESIGN.md §4, "DIBR stereo rendering".
//
// Sub-pixel DIBR (v3d_render_stereo_subpixel_batch, k_render_stereo<PPT, true, K>) is the same march with positions in 1/16 px:
// p(x) = 16 x + floor((g (D[x] - conv) + 2^19) / 2^20).  Source x owns the span [p(x), p(x) + L): L = p(x+1) - p(x) when that
// lies in (0, V3D_STEREO_TEAR16] (a connected span, colours interpolated between F[x] and F[x+1]), else 16 (a point: last
// column, fold or tear, colour F[x]).  It differs from the integer kernel in three places:
//   2. scatter: the span's integer targets (at most two, first (p + 15) >> 4) each take a ds_max_u32 of the same key;
//   4. gather: a hit target rebuilds p, L and w = 16 t - p from its key (D[x] is in the key, D[x+1] and the two colours in
//      LDS) and interpolates floor((2 ((L - w) F[x] + w F[x+1]) + L) / 2L) as a multiply by ceil(2^20 / 2L) and a shift;
//      holes carry the COLOUR of the neighbouring hit target, not its key;
//   ... and the nearest hit targets outside a thread's run are evaluated from their keys and the indices the scans yield.
// Contract: tests/stereo_sub_ref.py (bit-exact).  Resources and measured numbers: DESIGN.md §4, "Sub-pixel DIBR".
//
// Output packings (v3d_render_stereo_packed_batch): the march is written once, k_render_stereo<PPT, SUB, K>.  K = ST_K_SBS is the
// two side-by-side layouts above, stored from step 4; every other K adds a fifth step to either renderer, which packs the eyes
// top-bottom, row-interleaved or as a red-cyan anaglyph before the store; colours that must wait for the other eye or the next
// row wait in LDS words only their thread touches.
// Contract: tests/stereo_pack_ref.py (bit-exact).  Resources and measured numbers: DESIGN.md §4, "Output packings".
//
// Source fill (v3d_render_stereo_source_batch): the same march, entered with one more kernel argument (StSource).  A hole of an
// eye whose fill bit is set takes the bilinear sample of the film's own stored eye at its target instead of the background: four
// byte-wise global loads per channel, issued by the hole targets only (a few percent of a row); the eye plane is a few MB and
// stays in L2, so it costs neither LDS nor a 4K plane through HBM.  The row's j0, j1, fy are workgroup-uniform.
// Contract: tests/stereo_source_ref.py (bit-exact).  Resources and measured numbers: DESIGN.md §4, "Source-faithful 3D".
#include "v3d_common.h"
#include "v3d_wave.h"

#define ST_THREADS 256
#define ST_BAND 4                 // rows per workgroup: a 4K frame is 540 workgroups, one round of the resident slots
#define ST_MAX_W 8192

namespace {

// bytes of the aligned 16-byte chunks that cover `len` bytes starting at an address with (addr & 15) <= max_off
__host__ __device__ constexpr int st_chunks(int len, int max_off) { return (len + max_off + 15) / 16; }
__host__ __device__ constexpr int st_cdiv(int a, int b) { return (a + b - 1) / b; }

template <int NW>
__device__ __forceinline__ void st_store_run(uint8_t* p, const uint32_t (&w)[NW], int nbytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (nbytes == NW * 4) {
        if constexpr (NW % 4 == 0) {
            if ((a & 15) == 0) {
#pragma unroll
                for (int q = 0; q < NW / 4; ++q)
                    st_stream(reinterpret_cast<uint4*>(p) + q, make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]));
                return;
            }
        }
        if constexpr (NW % 2 == 0) {
            if ((a & 7) == 0) {
#pragma unroll
                for (int q = 0; q < NW / 2; ++q) st_stream(reinterpret_cast<uint2*>(p) + q, make_uint2(w[2 * q], w[2 * q + 1]));
                return;
            }
        }
        if ((a & 3) == 0) {
#pragma unroll
            for (int q = 0; q < NW; ++q) reinterpret_cast<uint32_t*>(p)[q] = w[q];
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < NW * 4; ++i)                           // the row's last run, or an unaligned row
        if (i < nbytes) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

__device__ __forceinline__ uint32_t st_fill(uint32_t a, uint32_t b)
{
    // a hole between keys a (left) and b (right): the farther one wins, ties go left; one side missing: the other (or 0)
    return (a && b) ? ((a >> 16) <= (b >> 16) ? a : b) : (a ? a : b);
}

__device__ __forceinline__ int st_shift(int g, int d, int conv)
{
    const int64_t num = (int64_t)g * (int64_t)(d - conv);      // |num| < 2^40
    return (int)((num + (1 << 23)) >> 24);                     // arithmetic shift = floor
}

__device__ __forceinline__ int st_shift16(int g, int d, int conv)
{
    // floor((g dd + 2^19) / 2^20), dd = d - conv, the shift in 1/16 px, without the 64-bit product: with g = 2^12 gh + gl it is
    // floor((dd gh + (dd gl + 2^19) / 2^12) / 2^8), and dd gh is an integer, so the inner quotient may be floored first.  |dd| < 2^16,
    // |gh| <= 2^12, gl < 2^12: 24-bit operands (full-rate v_mul_i32_i24), sums below 2^30.  tests/test_stereo_sub_ref.py repeats it.
    const int dd = d - conv;
    return (__mul24(dd, g >> 12) + ((__mul24(dd, g & 4095) + (1 << 19)) >> 12)) >> 8;
}

// sub-pixel: the colour of hit target t of the eye with gain g, from its key k != 0.  A point span (fold, tear) has w = 0; the last
// column reads itself as its right neighbour (L = 16, both colours equal): F[x] either way, without a branch.
__device__ __forceinline__ uint32_t st_sub_colour(uint32_t k, int t, int g, int conv, int W, const uint16_t* drow,
                                                  const unsigned char* frow, const uint32_t* sM)
{
    const int x = (int)(k & 0xFFFFu) - 1, x1 = min(x + 1, W - 1);
    const int s0 = st_shift16(g, (int)(k >> 16), conv);
    const int Lp = 16 + st_shift16(g, drow[x1], conv) - s0;
    const bool conn = (unsigned)(Lp - 1) < (unsigned)V3D_STEREO_TEAR16;
    // L <= 32 and w < L; the masks say so to the compiler, which then multiplies with the full-rate 24-bit instructions
    const uint32_t L = (conn ? (uint32_t)Lp : 16u) & 63u, w = (conn ? (uint32_t)(16 * t - (16 * x + s0)) : 0u) & 31u;
    const uint32_t m = sM[L] & 0xFFFFFu;
    const unsigned char *pa = frow + 3 * x, *pb = frow + 3 * x1;
    uint32_t c = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {                           // (L - w) a + w b = L a + w (b - a); numerator <= 511 L < 2^14, m <= 2^19
        const int fa = pa[ch], fb = pb[ch];
        const uint32_t num = (uint32_t)(2 * ((int)L * fa + (int)w * (fb - fa))) + L;
        c |= (((num & 0x3FFFu) * m) >> 20) << (8 * ch);
    }
    return c;
}

template <int PPT>
struct StGeom {
    static constexpr int WP = PPT * ST_THREADS;                // padded key row per eye (targets >= W stay 0)
    static constexpr int ND = st_cdiv(st_chunks(2 * WP, 14), ST_THREADS);   // depth chunks per thread
    static constexpr int NF = st_cdiv(st_chunks(3 * WP, 15), ST_THREADS);   // BGR chunks per thread
};

// what the march does with the eye colours: the two side-by-side layouts (the mode argument says which), full top-bottom,
// half top-bottom, row-interleaved, anaglyph (mode: Dubois)
enum { ST_K_SBS, ST_K_TB, ST_K_HTB, ST_K_ROWS, ST_K_ANA };

// LDS behind the BGR row in which a thread parks colours for itself, words [w][thread]: anaglyph the left eye's PPT colours until
// the right eye's are there, half top-bottom both eyes' packed even row (PPT * 3 / 4 words each) until the odd row's is there
template <int PPT>
__host__ __device__ constexpr int st_park_bytes(int kind)
{
    return kind == ST_K_ANA ? 4 * PPT * ST_THREADS : kind == ST_K_HTB ? 2 * (PPT * 3 / 4) * 4 * ST_THREADS : 0;
}

// static LDS of a packing's march (st_smem): both key rows, the widest depth and BGR rows at any phase, the parked words
template <int PPT>
__host__ __device__ constexpr int st_lds_bytes(int kind)
{
    return 8 * PPT * ST_THREADS + st_chunks(2 * PPT * ST_THREADS, 14) * 16 + st_chunks(3 * PPT * ST_THREADS, 15) * 16 + st_park_bytes<PPT>(kind);
}

// PPT colours (B | G << 8 | R << 16) -> the 3 PPT bytes of the run as words
template <int PPT>
__device__ __forceinline__ void st_pack3(const uint32_t (&col)[PPT], uint32_t (&wds)[PPT * 3 / 4])
{
#pragma unroll
    for (int w = 0; w < PPT * 3 / 4; ++w) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) v |= ((col[(4 * w + b) / 3] >> (8 * ((4 * w + b) % 3))) & 0xFFu) << (8 * b);
        wds[w] = v;
    }
}

// red-cyan anaglyph of one target from its left and right eye colours.  Colour: red from the left eye, green and blue from the
// right.  Dubois: his least-squares matrices in 1/65536 (every row sums to 65536: equal greys map to themselves), floor, clamp
__device__ __forceinline__ uint32_t st_anaglyph(uint32_t l, uint32_t r, int dubois)
{
    if (!dubois) return (r & 0x00FFFFu) | (l & 0xFF0000u);
    const int bl = (int)(l & 255u), gl = (int)((l >> 8) & 255u), rl = (int)((l >> 16) & 255u);
    const int br = (int)(r & 255u), gr = (int)((r >> 8) & 255u), rr = (int)((r >> 16) & 255u);
    const int R = (29891 * rl + 32800 * gl + 11559 * bl - 2849 * rr - 5763 * gr - 102 * br + 32768) >> 16;
    const int Gn = (-2627 * rl - 2479 * gl - 1033 * bl + 24804 * rr + 48080 * gr - 1209 * br + 32768) >> 16;
    const int B = (-997 * rl - 1350 * gl - 358 * bl - 4729 * rr - 7403 * gr + 80373 * br + 32768) >> 16;
    return (uint32_t)min(max(B, 0), 255) | ((uint32_t)min(max(Gn, 0), 255) << 8) | ((uint32_t)min(max(R, 0), 255) << 16);
}

// source fill: the SBS frames whose stored eyes the holes are sampled from, and the Q16 map from a target to eye coordinates
struct StSource {
    const uint8_t* sbs;
    size_t stride;                                             // bytes between frames
    int We, Hs, pitch, fill;                                   // eye width (Ws / 2), rows, row pitch, bit e: eye e's holes
    long long ax, bx, ay, by;
};

__device__ __forceinline__ const StSource& st_source(const StSource& s) { return s; }

// eye plane P at target t, from the eye's rows j0 and j1 (r0, r1: their first byte of this eye) and the row's fy; the taps
// stay inside the eye's We columns, 16-bit products and a sum below 2^24 + 2^15
__device__ __forceinline__ uint32_t st_source_colour(const uint8_t* r0, const uint8_t* r1, int fy, int t, const StSource& S)
{
    const long long um = (long long)(S.We - 1) << 16, ul = S.ax * t + S.bx;
    const int u = (int)(ul < 0 ? 0 : ul > um ? um : ul);
    const int i0 = u >> 16, i1 = min(i0 + 1, S.We - 1), fx = (u >> 8) & 255;
    uint32_t c = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const uint32_t top = (uint32_t)((256 - fx) * r0[3 * i0 + ch] + fx * r0[3 * i1 + ch]);
        const uint32_t bot = (uint32_t)((256 - fx) * r1[3 * i0 + ch] + fx * r1[3 * i1 + ch]);
        c |= (((256 - fy) * top + fy * bot + 32768u) >> 16) << (8 * ch);
    }
    return c;
}

// the march's LDS.  Side by side: dynamic, sized per launch for the row's W (launch_stereo), the file's one dynamic declaration,
// which the host emulator rewrites.  The packings: static, sized for the widest row of PPT pixels per thread plus what K parks
// (st_park_bytes); 8 WP of it do not depend on W anyway.
template <int PPT, int K>
__device__ __forceinline__ unsigned char* st_smem()
{
    if constexpr (K == ST_K_SBS) {
        extern __shared__ __attribute__((aligned(16))) unsigned char st_dyn[];
        return st_dyn;
    } else {
        __shared__ __attribute__((aligned(16))) unsigned char st_fix[st_lds_bytes<PPT>(K)];
        return st_fix;
    }
}

}  // namespace

// The march, once, for all four entries.  SUB selects the sub-pixel scatter and gather.  K says what becomes of the eye colours:
// ST_K_SBS stores them side by side (mode: half SBS) from step 4, the other K go through step 5 (mode: ST_K_ANA: Dubois), and the
// row-interleaved frame skips the eye a row does not show (eye_on; for every other K it folds away).  K selects by if constexpr,
// so an instantiation is compiled from its own statements alone, and its machine code is pinned (tools/kernel_digest.py;
// DESIGN.md §4, "Output packings", One march): a few declarations below stand where they do because moving them moves it.
// SRC is empty, or StSource: the source fill's one more kernel argument.  Its statements stand under if constexpr (sizeof...(SRC)),
// so the instantiations without it are compiled from what they had.
template <int PPT, bool SUB, int K, class... SRC>
__global__ __launch_bounds__(ST_THREADS) void k_render_stereo(const uint8_t* __restrict__ frame, size_t frame_stride,
                                                              const uint16_t* __restrict__ depth, size_t depth_stride, int W, int H,
                                                              int gl, int gr, int conv, int mode, uint8_t* __restrict__ out,
                                                              int sd_bytes, SRC... src)
{
    using G = StGeom<PPT>;
    constexpr int WP = G::WP, ND = G::ND, NF = G::NF;
    unsigned char* smem = st_smem<PPT, K>();
    uint32_t* sZ = reinterpret_cast<uint32_t*>(smem);          // [2][WP]
    unsigned char* sD = smem + 8 * WP;                         // depth row chunks (sd_bytes)
    unsigned char* sF = sD + sd_bytes;                         // BGR row chunks
    __shared__ uint32_t sTot[2][2][ST_THREADS / 64];           // [eye][prefix | suffix][wave]
    __shared__ uint32_t sM[SUB ? V3D_STEREO_TEAR16 + 1 : 1];   // sub-pixel: ceil(2^20 / 2L), read after the row's first barrier

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (SUB) {
        if (tid >= 1 && tid <= V3D_STEREO_TEAR16) sM[tid] = ((1u << 20) + 2u * tid - 1u) / (2u * tid);
    }
    const int f = blockIdx.y;
    const int y0 = blockIdx.x * ST_BAND, y1 = min(y0 + ST_BAND, H);
    const uint8_t* fr = frame + (size_t)f * frame_stride;
    const uint16_t* dp = depth + (size_t)f * depth_stride;
    // side by side: the output row's arithmetic, declared here and constant for every other K (either moves machine code otherwise)
    [[maybe_unused]] const int outW = K != ST_K_SBS ? 0 : mode ? W : 2 * W;
    [[maybe_unused]] const int eye_bytes = K != ST_K_SBS ? 0 : mode ? (W / 2) * 3 : W * 3;
    // this thread's parked words: st_park_bytes; nobody else reads or writes them, so they need no barrier
    uint32_t* sP = reinterpret_cast<uint32_t*>(sF + st_chunks(3 * W, 15) * 16) + tid;
    // row-interleaved keeps one eye per row (the left in even rows): the other is neither scattered, scanned nor filled
    auto eye_on = [&](int e, int y) { return K != ST_K_ROWS || e == (y & 1); };

    // a row's bytes as aligned 16-byte chunks: every load is unconditional (lanes past the last chunk re-read it), the
    // chunks never leave the 16-byte blocks the row touches
    uint4 rd[ND], rf[NF];
    auto load_row = [&](int y) {
        const uintptr_t ds = reinterpret_cast<uintptr_t>(dp + (size_t)y * W), fs = reinterpret_cast<uintptr_t>(fr + (size_t)y * W * 3);
        const uint4* da = reinterpret_cast<const uint4*>(ds & ~(uintptr_t)15);
        const uint4* fa = reinterpret_cast<const uint4*>(fs & ~(uintptr_t)15);
        const int nd = (int)((ds + 2 * (uintptr_t)W - (ds & ~(uintptr_t)15) + 15) >> 4);
        const int nf = (int)((fs + 3 * (uintptr_t)W - (fs & ~(uintptr_t)15) + 15) >> 4);
#pragma unroll
        for (int k = 0; k < ND; ++k) rd[k] = ld_stream(da + min(k * ST_THREADS + tid, nd - 1));
#pragma unroll
        for (int k = 0; k < NF; ++k) rf[k] = ld_stream(fa + min(k * ST_THREADS + tid, nf - 1));
    };

    load_row(y0);
    for (int y = y0; y < y1; ++y) {
        const uintptr_t ds = reinterpret_cast<uintptr_t>(dp + (size_t)y * W), fs = reinterpret_cast<uintptr_t>(fr + (size_t)y * W * 3);
        const int doff = (int)(ds & 15), foff = (int)(fs & 15);
        const int nd = (doff + 2 * W + 15) >> 4, nf = (foff + 3 * W + 15) >> 4;
        __syncthreads();                                       // the previous row's LDS reads are done
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const int c = k * ST_THREADS + tid;
            if (c < nd) reinterpret_cast<uint4*>(sD)[c] = rd[k];
        }
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const int c = k * ST_THREADS + tid;
            if (c < nf) reinterpret_cast<uint4*>(sF)[c] = rf[k];
        }
#pragma unroll
        for (int k = 0; k < 2 * WP / 4 / ST_THREADS; ++k) reinterpret_cast<uint4*>(sZ)[k * ST_THREADS + tid] = make_uint4(0, 0, 0, 0);
        if (y + 1 < y1) load_row(y + 1);                       // in flight while this row is rendered
        __syncthreads();

        // 2. scatter both eyes' keys
        const uint16_t* drow = reinterpret_cast<const uint16_t*>(sD + doff);
#pragma unroll 4
        for (int j = 0; j < PPT; ++j) {
            const int x = j * ST_THREADS + tid;
            if (x < W) {
                const int d = drow[x];
                const uint32_t key = ((uint32_t)d << 16) | (uint32_t)(x + 1);
                if constexpr (SUB) {
                    const int d1 = drow[min(x + 1, W - 1)];         // the last column: L' = 16, the point span's length
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        if (!eye_on(e, y)) continue;
                        const int g = e ? gr : gl, s0 = st_shift16(g, d, conv), Lp = 16 + st_shift16(g, d1, conv) - s0;
                        const int p = 16 * x + s0, end = p + ((unsigned)(Lp - 1) < (unsigned)V3D_STEREO_TEAR16 ? Lp : 16);
                        const int t0 = (p + 15) >> 4;              // arithmetic shift = floor; L <= 32: at most two targets
                        if (16 * t0 < end && (unsigned)t0 < (unsigned)W) atomicMax(sZ + e * WP + t0, key);
                        if (16 * t0 + 16 < end && (unsigned)(t0 + 1) < (unsigned)W) atomicMax(sZ + e * WP + t0 + 1, key);
                    }
                } else {
                    const int tl = x + st_shift(gl, d, conv), tr = x + st_shift(gr, d, conv);
                    if (eye_on(0, y) && (unsigned)tl < (unsigned)W) atomicMax(sZ + tl, key);
                    if (eye_on(1, y) && (unsigned)tr < (unsigned)W) atomicMax(sZ + WP + tr, key);
                }
            }
        }
        __syncthreads();

        // 3. nearest keys outside my run: (last key index + 1) from the left, (WP - first key index) from the right
        const int x0 = tid * PPT;
        uint32_t pre[2], suf[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!eye_on(e, y)) continue;
            const uint4* zr = reinterpret_cast<const uint4*>(sZ + e * WP + x0);
            uint32_t lastp = 0, firstp = 0;
#pragma unroll
            for (int q = PPT / 4 - 1; q >= 0; --q) {
                const uint4 v = zr[q];
                const uint32_t k4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (int i = 3; i >= 0; --i) {
                    if (k4[i]) {
                        if (!lastp) lastp = (uint32_t)(x0 + 4 * q + i + 1);
                        firstp = (uint32_t)(WP - (x0 + 4 * q + i));
                    }
                }
            }
            const near2 sc = near2_incl(lastp, firstp, lane);
            if (lane == 63) sTot[e][0][wave] = sc.pre;
            if (lane == 0) sTot[e][1][wave] = sc.suf;
            const near2 ex = near2_excl(sc, lane);
            pre[e] = ex.pre; suf[e] = ex.suf;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!eye_on(e, y)) continue;
#pragma unroll
            for (int w = 0; w < ST_THREADS / 64; ++w) {        // v3d_wave.h's near2_fold, kept here: its call costs half SBS 0.5 %
                if (w < wave) pre[e] = max(pre[e], sTot[e][0][w]);
                if (w > wave) suf[e] = max(suf[e], sTot[e][1][w]);
            }
        }

        // 4. fill, gather, store
        const int nvalid = min(PPT, W - x0);                   // <= 0: this thread's run lies beyond the row
        [[maybe_unused]] uint8_t* orow = K != ST_K_SBS ? nullptr : out + ((size_t)f * H + y) * (size_t)outW * 3;
        const unsigned char* frow = sF + foff;
        [[maybe_unused]] const uint8_t *er0 = nullptr, *er1 = nullptr;     // source fill: the SBS rows j0, j1 of this output row
        [[maybe_unused]] int efy = 0;
        if constexpr (sizeof...(SRC) > 0) {
            const StSource& S = st_source(src...);
            // v stays 64 bits wide: Hs has no bound but int's, so (Hs - 1) << 16 may pass 2^31 (u may not: We <= ST_MAX_W)
            const long long vm = (long long)(S.Hs - 1) << 16, vl = S.ay * y + S.by;
            const long long v = vl < 0 ? 0 : vl > vm ? vm : vl;
            const int j0 = (int)(v >> 16), j1 = min(j0 + 1, S.Hs - 1);
            const uint8_t* eb = S.sbs + (size_t)f * S.stride;
            er0 = eb + (size_t)j0 * S.pitch; er1 = eb + (size_t)j1 * S.pitch; efy = (int)(v >> 8) & 255;
        }
        for (int e = 0; e < 2; ++e) {
            if (!eye_on(e, y)) continue;
            uint32_t kk[PPT], col[PPT];
            [[maybe_unused]] uint32_t holes = 0;               // source fill: bit i: target x0 + i has no key
            const uint4* zr = reinterpret_cast<const uint4*>(sZ + e * WP + x0);
#pragma unroll
            for (int q = 0; q < PPT / 4; ++q) {
                const uint4 v = zr[q];
                kk[4 * q] = v.x; kk[4 * q + 1] = v.y; kk[4 * q + 2] = v.z; kk[4 * q + 3] = v.w;
            }
            uint32_t nb = suf[e] ? sZ[e * WP + WP - suf[e]] : 0u;
            uint32_t na = pre[e] ? sZ[e * WP + pre[e] - 1] : 0u;
            if constexpr (SUB) {
                // hit targets get their colour; holes then carry the (key, colour) of the nearest hit target on either side,
                // the key only for the depth comparison
                const int g = e ? gr : gl;
                uint32_t hit = 0, nbc = 0, nac = 0;
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    col[i] = 0;
                    if (kk[i]) { hit |= 1u << i; col[i] = st_sub_colour(kk[i], x0 + i, g, conv, W, drow, frow, sM); }
                }
                if (nb) nbc = st_sub_colour(nb, WP - (int)suf[e], g, conv, W, drow, frow, sM);
                if (na) nac = st_sub_colour(na, (int)pre[e] - 1, g, conv, W, drow, frow, sM);
#pragma unroll
                for (int i = PPT - 1; i >= 0; --i) {
                    if ((hit >> i) & 1u) { nb = kk[i]; nbc = col[i]; }
                    else { kk[i] = nb; col[i] = nbc; }
                }
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    if ((hit >> i) & 1u) { na = kk[i]; nac = col[i]; }
                    else if (na && (!kk[i] || (na >> 16) <= (kk[i] >> 16))) col[i] = nac;      // st_fill's choice
                }
                if constexpr (sizeof...(SRC) > 0) holes = ~hit;
            } else {
                uint32_t rb[PPT];
#pragma unroll
                for (int i = PPT - 1; i >= 0; --i) { rb[i] = nb; if (kk[i]) nb = kk[i]; }
#pragma unroll
                for (int i = 0; i < PPT; ++i) {
                    uint32_t k = kk[i];
                    if (k) na = k;
                    else k = st_fill(na, rb[i]);
                    const int s = k ? (int)(k & 0xFFFFu) - 1 : 0;
                    const unsigned char* px = frow + 3 * s;
                    col[i] = k ? ((uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16)) : 0u;
                    if constexpr (sizeof...(SRC) > 0) holes |= (kk[i] ? 0u : 1u) << i;
                }
            }
            if constexpr (sizeof...(SRC) > 0) {                // holes of a filled eye: the stored eye's colour at the target
                const StSource& S = st_source(src...);
                if ((S.fill >> e) & 1) {
                    // four targets per step of a loop that stays a loop: unrolled over the run, the loads of all PPT targets are
                    // scheduled together and the widest instantiations spill.  col[] is indexed by selects, not by q
                    const int eo = 3 * e * S.We;
                    holes &= nvalid >= PPT ? ~0u : nvalid > 0 ? (1u << nvalid) - 1u : 0u;
#pragma unroll 1
                    for (int q = 0; q < PPT / 4; ++q) {
                        const uint32_t h4 = (holes >> (4 * q)) & 15u;
                        if (!h4) continue;
                        uint32_t c4[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) c4[j] = st_source_colour(er0 + eo, er1 + eo, efy, x0 + 4 * q + j, S);
#pragma unroll
                        for (int i = 0; i < PPT; ++i)
                            if ((i >> 2) == q && ((h4 >> (i & 3)) & 1u)) col[i] = c4[i & 3];
                    }
                }
            }
            if constexpr (K == ST_K_SBS) {                     // side by side: store from here, statements kept as they were
                if (nvalid > 0 && !mode) {
                    constexpr int NW = PPT * 3 / 4;
                    uint32_t wds[NW];
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        uint32_t v = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) v |= ((col[(4 * w + b) / 3] >> (8 * ((4 * w + b) % 3))) & 0xFFu) << (8 * b);
                        wds[w] = v;
                    }
                    st_store_run(orow + e * eye_bytes + x0 * 3, wds, nvalid * 3);
                } else if (nvalid > 0) {
                    constexpr int NH = PPT / 2, NW = NH * 3 / 4;
                    uint32_t hc[NH];
#pragma unroll
                    for (int i = 0; i < NH; ++i) {             // per byte (a + b + 1) >> 1 = (a | b) - ((a ^ b) >> 1)
                        const uint32_t a = col[2 * i], b = col[2 * i + 1];
                        hc[i] = (a | b) - (((a ^ b) & 0xFEFEFEFEu) >> 1);
                    }
                    uint32_t wds[NW];
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        uint32_t v = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) v |= ((hc[(4 * w + b) / 3] >> (8 * ((4 * w + b) % 3))) & 0xFFu) << (8 * b);
                        wds[w] = v;
                    }
                    st_store_run(orow + e * eye_bytes + (x0 / 2) * 3, wds, (nvalid / 2) * 3);
                }
            } else {                                           // 5. pack and store
                constexpr int NW = PPT * 3 / 4;
                if constexpr (K == ST_K_ANA) {               // both eyes' colours of my targets: the left eye's wait in LDS
                    if (e == 0) {
#pragma unroll
                        for (int i = 0; i < PPT; ++i) sP[i * ST_THREADS] = col[i];
                        continue;
                    }
#pragma unroll
                    for (int i = 0; i < PPT; ++i) col[i] = st_anaglyph(sP[i * ST_THREADS], col[i], mode);
                }
                uint32_t wds[NW];
                st_pack3<PPT>(col, wds);
                if constexpr (K == ST_K_HTB) {                 // rows 2y' and 2y'+1 lie in one band: the even row's bytes wait in LDS
                    uint32_t* pk = sP + e * NW * ST_THREADS;
                    if (!(y & 1)) {
#pragma unroll
                        for (int w = 0; w < NW; ++w) pk[w * ST_THREADS] = wds[w];
                        continue;
                    }
#pragma unroll
                    for (int w = 0; w < NW; ++w) {             // per byte (a + b + 1) >> 1, as half SBS does
                        const uint32_t a = pk[w * ST_THREADS], b = wds[w];
                        wds[w] = (a | b) - (((a ^ b) & 0xFEFEFEFEu) >> 1);
                    }
                }
                // the output row: full top-bottom stacks the eyes (2H rows), half top-bottom their halved rows, the others have row y
                const size_t rows = K == ST_K_TB ? 2 * (size_t)H : (size_t)H;
                const int row = K == ST_K_TB ? e * H + y : K == ST_K_HTB ? e * (H / 2) + (y >> 1) : y;
                if (nvalid > 0) st_store_run(out + ((size_t)f * rows + row) * (size_t)W * 3 + x0 * 3, wds, nvalid * 3);
            }
        }
    }
}

template <int PPT, bool SUB, int K, class... SRC>
static int launch_stereo(const uint8_t* frame, size_t frame_stride, const uint16_t* depth, size_t depth_stride, int n, int W,
                         int H, int gl, int gr, int conv, int mode, uint8_t* out, hipStream_t stream, SRC... src)
{
    using G = StGeom<PPT>;
    const int sd = st_chunks(2 * W, 14) * 16, sf = st_chunks(3 * W, 15) * 16;
    auto* kernel = k_render_stereo<PPT, SUB, K, SRC...>;
    if constexpr (K == ST_K_SBS) {                             // dynamic LDS (st_smem); the packings' is static
        static bool attr_set = false;                          // per instantiation; the attribute is a property of the function
        if (!attr_set) {
            V3D_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              8 * G::WP + st_chunks(2 * G::WP, 14) * 16 + st_chunks(3 * G::WP, 15) * 16));
            attr_set = true;
        }
    }
    const int smem = K == ST_K_SBS ? 8 * G::WP + sd + sf : 0;
    hipLaunchKernelGGL(kernel, dim3(v3d_cdiv(H, ST_BAND), n), dim3(ST_THREADS), smem, stream, frame, frame_stride, depth,
                       depth_stride, W, H, gl, gr, conv, mode, out, sd, src...);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

template <int PPT, bool SUB, class... SRC>
static int launch_packing(int packing, const uint8_t* frame, size_t frame_stride, const uint16_t* depth, size_t depth_stride, int n,
                          int W, int H, int gl, int gr, int conv, uint8_t* out, hipStream_t s, SRC... src)
{
#define ST_LAUNCH(K, mode) launch_stereo<PPT, SUB, K>(frame, frame_stride, depth, depth_stride, n, W, H, gl, gr, conv, mode, out, s, src...)
    switch (packing) {
    case V3D_PACK_FULL_SBS: return ST_LAUNCH(ST_K_SBS, 0);
    case V3D_PACK_HALF_SBS: return ST_LAUNCH(ST_K_SBS, 1);
    case V3D_PACK_FULL_TB: return ST_LAUNCH(ST_K_TB, 0);
    case V3D_PACK_HALF_TB: return ST_LAUNCH(ST_K_HTB, 0);
    case V3D_PACK_ROWS: return ST_LAUNCH(ST_K_ROWS, 0);
    case V3D_PACK_ANAGLYPH_COLOUR: return ST_LAUNCH(ST_K_ANA, 0);
    default: return ST_LAUNCH(ST_K_ANA, 1);                    // V3D_PACK_ANAGLYPH_DUBOIS
    }
#undef ST_LAUNCH
}

// every refusal the render entries share: V3D_ERR_ARG first, then V3D_ERR_UNSUPPORTED.  max_packing: the entry's last packing code
// (the layouts of the two older entries are codes 0, 1)
static int stereo_refusal(const char* who, const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth, size_t depth_stride,
                          int n, int W, int H, int gain_left, int gain_right, int convergence, int packing, int max_packing,
                          uint8_t* out_bgr)
{
    if (!frame_bgr || !depth || !out_bgr) { v3d_set_error("%s: null pointer", who); return V3D_ERR_ARG; }
    if (n < 1 || n > 65535 || W < 1 || H < 1) { v3d_set_error("%s: bad geometry n=%d W=%d H=%d", who, n, W, H); return V3D_ERR_ARG; }
    if (n > 1 && (frame_stride < (size_t)W * H * 3 || depth_stride < (size_t)W * H)) {
        v3d_set_error("%s: frame stride %zu B / depth stride %zu elements smaller than a frame", who, frame_stride, depth_stride);
        return V3D_ERR_ARG;
    }
    if (packing < 0 || packing > max_packing) { v3d_set_error("%s: layout %d", who, packing); return V3D_ERR_ARG; }
    if (packing == V3D_PACK_HALF_SBS && (W & 1)) { v3d_set_error("%s: half SBS needs an even width (W=%d)", who, W); return V3D_ERR_ARG; }
    if (packing == V3D_PACK_HALF_TB && (H & 1)) { v3d_set_error("%s: half top-bottom needs an even height (H=%d)", who, H); return V3D_ERR_ARG; }
    const int gmax = 1 << 24;
    if (gain_left <= -gmax || gain_left >= gmax || gain_right <= -gmax || gain_right >= gmax) {
        v3d_set_error("%s: |gain| must be < 2^24 (%d, %d)", who, gain_left, gain_right);
        return V3D_ERR_ARG;
    }
    if (convergence < 0 || convergence > 65535) { v3d_set_error("%s: convergence %d outside [0, 65535]", who, convergence); return V3D_ERR_ARG; }
    if (W > ST_MAX_W) { v3d_set_error("%s: W=%d > %d", who, W, ST_MAX_W); return V3D_ERR_UNSUPPORTED; }
    return V3D_OK;
}

// every refusal, then the launch
template <bool SUB, class... SRC>
static int render_stereo(const char* who, const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth, size_t depth_stride,
                         int n, int W, int H, int gain_left, int gain_right, int convergence, int packing, int max_packing,
                         uint8_t* out_bgr, void* stream, SRC... src)
{
    const int rc = stereo_refusal(who, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right, convergence, packing,
                                  max_packing, out_bgr);
    if (rc != V3D_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (W <= 8 * ST_THREADS) return launch_packing<8, SUB>(packing, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right, convergence, out_bgr, s, src...);
    if (W <= 16 * ST_THREADS) return launch_packing<16, SUB>(packing, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right, convergence, out_bgr, s, src...);
    return launch_packing<32, SUB>(packing, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right, convergence, out_bgr, s, src...);
}

extern "C" int v3d_render_stereo_batch(const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth, size_t depth_stride,
                                       int n, int W, int H, int gain_left, int gain_right, int convergence, int layout,
                                       uint8_t* out_bgr, void* stream)
{
    return render_stereo<false>("v3d_render_stereo_batch", frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right,
                                convergence, layout, V3D_STEREO_HALF_SBS, out_bgr, stream);
}

extern "C" int v3d_render_stereo_subpixel_batch(const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth,
                                                size_t depth_stride, int n, int W, int H, int gain_left, int gain_right,
                                                int convergence, int layout, uint8_t* out_bgr, void* stream)
{
    return render_stereo<true>("v3d_render_stereo_subpixel_batch", frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left,
                               gain_right, convergence, layout, V3D_STEREO_HALF_SBS, out_bgr, stream);
}

extern "C" int v3d_render_stereo_packed_batch(const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth, size_t depth_stride,
                                              int n, int W, int H, int gain_left, int gain_right, int convergence, int subpixel,
                                              int packing, uint8_t* out_bgr, void* stream)
{
    const char* who = "v3d_render_stereo_packed_batch";
    if (subpixel != 0 && subpixel != 1) { v3d_set_error("%s: subpixel %d is neither 0 nor 1", who, subpixel); return V3D_ERR_ARG; }
    return (subpixel ? render_stereo<true> : render_stereo<false>)(who, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left,
                                                                   gain_right, convergence, packing, V3D_PACK_ANAGLYPH_DUBOIS, out_bgr,
                                                                   stream);
}

extern "C" int v3d_render_stereo_source_batch(const uint8_t* frame_bgr, size_t frame_stride, const uint16_t* depth, size_t depth_stride,
                                              int n, int W, int H, int gain_left, int gain_right, int convergence, int subpixel,
                                              int packing, const uint8_t* sbs_bgr, size_t sbs_stride, int Ws, int Hs, int pitch,
                                              int fill_eyes, int64_t ax, int64_t bx, int64_t ay, int64_t by, uint8_t* out_bgr,
                                              void* stream)
{
    const char* who = "v3d_render_stereo_source_batch";
    if (subpixel != 0 && subpixel != 1) { v3d_set_error("%s: subpixel %d is neither 0 nor 1", who, subpixel); return V3D_ERR_ARG; }
    if (fill_eyes < 0 || fill_eyes > 3) { v3d_set_error("%s: fill_eyes %d outside 0 .. 3", who, fill_eyes); return V3D_ERR_ARG; }
    if (fill_eyes && !sbs_bgr) { v3d_set_error("%s: null SBS pointer with fill_eyes %d", who, fill_eyes); return V3D_ERR_ARG; }
    if (Ws < 2 || (Ws & 1) || Hs < 1) { v3d_set_error("%s: bad SBS geometry Ws=%d (even, >= 2) Hs=%d", who, Ws, Hs); return V3D_ERR_ARG; }
    if ((int64_t)pitch < 3 * (int64_t)Ws) { v3d_set_error("%s: pitch %d < 3 Ws = %lld", who, pitch, 3LL * Ws); return V3D_ERR_ARG; }
    if (n > 1 && sbs_stride < (size_t)Hs * (size_t)pitch) {
        v3d_set_error("%s: SBS stride %zu B smaller than a frame", who, sbs_stride);
        return V3D_ERR_ARG;
    }
    const int64_t amin = 1 << 12, amax = 1 << 20, bmax = (int64_t)1 << 40;
    if (ax < amin || ax > amax || ay < amin || ay > amax || bx < -bmax || bx > bmax || by < -bmax || by > bmax) {
        v3d_set_error("%s: map (%lld, %lld, %lld, %lld) outside scale [2^12, 2^20], |offset| <= 2^40", who, (long long)ax,
                      (long long)bx, (long long)ay, (long long)by);
        return V3D_ERR_ARG;
    }
    // every V3D_ERR_ARG of the packed entry comes before either V3D_ERR_UNSUPPORTED (W, then the eye width)
    const int last = V3D_PACK_ANAGLYPH_DUBOIS;
    const int rc = stereo_refusal(who, frame_bgr, frame_stride, depth, depth_stride, n, W, H, gain_left, gain_right, convergence, packing,
                                  last, out_bgr);
    if (rc != V3D_OK) return rc;
    if (Ws / 2 > ST_MAX_W) { v3d_set_error("%s: eye width %d > %d", who, Ws / 2, ST_MAX_W); return V3D_ERR_UNSUPPORTED; }
    if (!fill_eyes)                                            // no eye to fill: the packed entry's kernels, and so its bits and its time
        return (subpixel ? render_stereo<true> : render_stereo<false>)(who, frame_bgr, frame_stride, depth, depth_stride, n, W, H,
                                                                       gain_left, gain_right, convergence, packing, last, out_bgr, stream);
    const StSource src = { sbs_bgr, sbs_stride, Ws / 2, Hs, pitch, fill_eyes, ax, bx, ay, by };
    return (subpixel ? render_stereo<true, StSource> : render_stereo<false, StSource>)(who, frame_bgr, frame_stride, depth, depth_stride,
                                                                                       n, W, H, gain_left, gain_right, convergence,
                                                                                       packing, last, out_bgr, stream, src);
}
