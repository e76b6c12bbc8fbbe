// v3d_sgbm_paths.hip -- the SGBM's path aggregation and winner-take-all (a-5, a-6): C -> S -> one WTA record per pixel.
// Default route: k_vdd (the three top-down paths in one lock-step pass) + k_hfused (both horizontal paths and the WTA tail in
// one launch).  k_chain (one launch per path direction, WTA tail on the last) is the route behind the options "lockstep" = 0 /
// "hfused" = 0 and is parity-tested like the default.
#include "v3d_sgbm_internal.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------
// a-5 / a-6: one SGM path direction per launch.  A "chain" is one scanline of the direction
// (a row, a column or a diagonal); a wave runs DPL adjacent chains in lock-step:
// LPP = 64/DPL lanes per pixel, each lane holding DPL consecutive disparities as DPL/2 packed
// int16 pairs.  d+-1 neighbours come from v_alignbit + one DPP row shift each way, the min over
// d from packed mins + a DPP butterfly inside the pixel's lane group: no LDS in the recurrence.
//   MODE 0: S  = L          (first direction)
//   MODE 1: S += L (sat)    (middle directions)
//   MODE 2: S + L -> LDS -> winner-take-all / uniqueness / sub-pixel / right-view keys (last direction)
// ------------------------------------------------------------------------------------------------
struct ChainArgs {
    const unsigned char* C; int16_t* S;
    int W1, H, W, nframes;
    int P1, P2;
    int uniq;                 // uniquenessRatio
    uint32_t t1_mul; int t1_shift;      // v3d_t1_magic(100 - uniq): the uniqueness threshold without a division (unused when uniq >= 100)
    uint32_t* wta;            // MODE 2: [nframes][H][W] WTA records (wta_word); columns < 64 are never written
    int xcd;                  // k_hfused: XCD-contiguous row-group order (V3D_HF_XCD=1).  Measured 4 % slower: off
    int persist;              // k_hfused: 0 = one wave per row group; 1 = the resident number of waves draws row groups from `ticket`
    int* ticket;
};

// minimum of both halves of `mn` over the LPP lanes of a pixel, returned in BOTH halves.  One v_pk_min_u16 with op_sel
// swaps the halves against each other (lo = min(lo, hi), hi = min(hi, lo)); a word with equal halves orders like its
// half as an unsigned 32-bit number, so each butterfly step is ONE v_min_u32 with a DPP operand (packed VOP3P ops cannot
// take DPP) and the result needs no re-broadcast.  Costs are non-negative 15-bit values.
template <int LPP>
__device__ __forceinline__ uint32_t pk_hmin_lanes(uint32_t mn)
{
    uint32_t m1;
    asm("v_pk_min_u16 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(m1) : "v"(mn));
    m1 = min(m1, dpp_xchg<V3D_DPP_QUAD(1, 0, 3, 2)>(m1));
    m1 = min(m1, dpp_xchg<V3D_DPP_QUAD(2, 3, 0, 1)>(m1));
    if (LPP >= 8) m1 = min(m1, dpp_xchg<V3D_DPP_ROW_HALF_MIRROR>(m1));
    if (LPP >= 16) m1 = min(m1, dpp_xchg<V3D_DPP_ROW_MIRROR>(m1));
    return m1;
}

// L[d] = C[d] + min(Lp[d], Lp[d-1]+P1, Lp[d+1]+P1, delta) - delta ; returns delta' = min_d L[d] + P2 (both halves)
template <int NP, int LPP>
__device__ __forceinline__ uint32_t chain_step(const uint32_t (&p)[NP], uint32_t delta, const uint32_t (&c)[NP],
                                               uint32_t (&L)[NP], uint32_t P1pk, uint32_t P2pk, bool first_lane, bool last_lane)
{
    const uint32_t MAXPK = 0x7FFF7FFFu;
    // d-1 / d+1 across the lanes of a pixel: one v_or_b32 with a DPP operand each.  The pixel's edge lanes OR the
    // out-of-range fill in (costs are 15-bit, so x | 0x7FFF7FFF is the fill whatever the shift delivered: the neighbour
    // pixel's lane, or 0 from bound_ctrl where the DPP row ends); the masks are loop-invariant registers.
    const uint32_t fill_prev = first_lane ? MAXPK : 0u, fill_next = last_lane ? MAXPK : 0u;
    const uint32_t prev = dpp_xchg<V3D_DPP_ROW_SHR(1)>(p[NP - 1]) | fill_prev;
    const uint32_t next = dpp_xchg<V3D_DPP_ROW_SHL(1)>(p[0]) | fill_next;
    uint32_t m[NP + 1];
    m[0] = alignbit(p[0], prev, 16);
#pragma unroll
    for (int i = 1; i < NP; i++) m[i] = alignbit(p[i], p[i - 1], 16);
    m[NP] = alignbit(next, p[NP - 1], 16);
    uint32_t mn = MAXPK;
#pragma unroll
    for (int i = 0; i < NP; i++) {
        // C - delta + min(p, n, delta) = C - max(delta - min(p, n), 0): the clamp is the unsigned saturating subtract's
        // (5 packed ops per pair instead of 6; delta - min(p, n) <= P2 <= C, all operands in [0, 32767))
        uint32_t n = pk_add(pk_min(m[i], m[i + 1]), P1pk);
        L[i] = pk_sub(c[i], pk_subu_sat(delta, pk_min(p[i], n)));
        mn = pk_min(mn, L[i]);
    }
    return pk_add(pk_hmin_lanes<LPP>(mn), P2pk);
}

// delta = min_d L[d] + P2 (both halves) recomputed from a path-state vector: lets checkpoints drop the delta word
template <int NP, int LPP>
__device__ __forceinline__ uint32_t chain_delta(const uint32_t (&p)[NP], uint32_t P2pk)
{
    uint32_t mn = p[0];
#pragma unroll
    for (int i = 1; i < NP; i++) mn = pk_min(mn, p[i]);
    return pk_add(pk_hmin_lanes<LPP>(mn), P2pk);
}

#define WTA_ROWB 144   // bytes per pixel row in LDS (128 + 16 pad, keeps 16-B alignment)

// winner-take-all for one pixel whose 64 aggregated costs sit in LDS (stereosgbm.cpp per-row tail)
__device__ __forceinline__ void wta_pixel(const unsigned char* srow, bool valid, int x, int y, int frame,
                                          const ChainArgs& a)
{
    uint32_t v[32];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint4 t = *reinterpret_cast<const uint4*>(srow + q * 16);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
    // argmin with the lowest d winning ties, in packed 16-bit arithmetic: (1) min S over the 64 halves; (2) keys
    // (S - minS) * 64 + d with saturation (only keys < 64, i.e. S == minS, can win) and their packed minimum.
    // 4 packed ops per two disparities instead of 6 scalar ones.
    uint32_t mpk = v[0];
#pragma unroll
    for (int i = 1; i < 32; i++) mpk = pk_minu(mpk, v[i]);
    const int minS = (int)min(mpk & 0xFFFFu, mpk >> 16);
    const uint32_t minpk = pk_bcast(minS), k64 = 0x00400040u;
    // (three passes, not one loop: the compiler assumes a forwarding hazard around every inline-asm result and would put an
    //  s_nop on each side of the v_pk_mad_u16 if its producer and consumer stood next to it -- 57 per pixel)
    uint32_t kacc = 0xFFFFFFFFu, key[32];
#pragma unroll
    for (int i = 0; i < 32; i++) key[i] = pk_subu_sat(v[i], minpk);
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const uint32_t dc = (uint32_t)(2 * i) | ((uint32_t)(2 * i + 1) << 16);
        asm("v_pk_mad_u16 %0, %1, %2, %3 clamp" : "=v"(key[i]) : "v"(key[i]), "v"(k64), "s"(dc));
    }
#pragma unroll
    for (int i = 0; i < 32; i++) kacc = pk_minu(kacc, key[i]);
    const int best = (int)(min(kacc & 0xFFFFu, kacc >> 16) & 63u);
    // uniqueness: reject iff exists d, |d-best| > 1, S[d]*(100-uniq) < minS*100  <=>  S[d] < T1
    // Everything below is computed on every lane and only SELECTED by uq, ok and valid, so that the tail is one basic block;
    // the empty asm statements pin a value to this place (the compiler otherwise moves its computation behind a branch again).
    const int uq = 100 - a.uniq;
    int t1q = v3d_t1_ceil(minS, uq, a.t1_mul, a.t1_shift);
    asm volatile("" : "+v"(t1q));
    const int T1 = min(uq > 0 ? t1q : min(minS, 1) << 15, 32768);                // uq == 0: minS * 100 > 0 ? 32768 : 0
    // count of S[d] < T1: S in [0, 32767] and T1 in [0, 32768], so S - T1 fits int16 and its sign bit IS the comparison.
    // Per pair of words 2 subtracts + 2 shifts + one three-operand add (a half counts to 32 at most: no carry between them).
    const uint32_t T1pk = pk_bcast(T1);
    uint32_t cntpk = 0;
#pragma unroll
    for (int i = 0; i < 32; i += 2) cntpk += pk_shr_u(pk_subu(v[i], T1pk), 15) + pk_shr_u(pk_subu(v[i + 1], T1pk), 15);
    const int cnt = (int)(cntpk & 0xFFFFu) + (int)(cntpk >> 16);
    const unsigned short* s16 = reinterpret_cast<const unsigned short*>(srow);
    const bool inner = best > 0 && best < V3D_D - 1;
    const int sm = best > 0 ? (int)s16[best - 1] : 0, sp = best < V3D_D - 1 ? (int)s16[best + 1] : 0;
    int cw = (minS < T1) ? 1 : 0;
    if (best > 0 && sm < T1) cw++;
    if (best < V3D_D - 1 && sp < T1) cw++;
    const bool ok = (minS < V3D_MAX_COST) && (cnt <= cw);
    int subpix = v3d_subpix_q(sm - minS, sp - minS);            // meaningful only where `inner`
    asm volatile("" : "+v"(subpix));
    uint32_t word = wta_word(minS, best * 16 + (inner ? subpix : 0), best);
    asm volatile("" : "+v"(word));
    word = ok ? word : 0u;                                     // 0 = invalid
    if (valid) a.wta[((size_t)frame * a.H + y) * a.W + x + V3D_D] = word;
}

template <bool HORIZ, int XS, bool YREV, int MODE, int DPL>
__global__ __launch_bounds__(256) void k_chain(ChainArgs a)
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, PPW = DPL;     // chains (pixels) per wave = 64 / LPP
    constexpr int PF = 4;                                     // prefetch depth (steps)
    constexpr int BS = 64 / PPW;                              // MODE 2: steps per WTA batch
    typedef typename VecT<DPL>::type Vec;
    static_assert(MODE != 2 || HORIZ, "the WTA tail rides on a horizontal direction");

    __shared__ __attribute__((aligned(16))) unsigned char sS[MODE == 2 ? 4 * 64 * WTA_ROWB : 16];

    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W1 = a.W1, H = a.H;
    const int NC = HORIZ ? H : (XS == 0 ? W1 : W1 + H - 1);
    const int groups = (NC + PPW - 1) / PPW;
    const int gw = blockIdx.x * 4 + wib;
    const int frame = gw / groups, grp = gw - frame * groups;
    if (frame >= a.nframes) return;                           // wave-uniform; no block-wide barriers below

    const int sub = lane / LPP, dl = lane % LPP;
    const int c0 = grp * PPW, c1 = min(c0 + PPW, NC) - 1;
    const int c = c0 + sub;
    const bool cvalid = c <= c1;
    const int cc = min(c, c1);

    int tlo = 0, thi;
    if (HORIZ) thi = W1;
    else if (XS == 0) thi = H;
    else if (XS > 0) { tlo = max(0, H - 1 - c1); thi = min(H, W1 + H - 1 - c0); }
    else { tlo = max(0, c0 - (W1 - 1)); thi = min(H, c1 + 1); }

    const unsigned char* Cf = a.C + (size_t)frame * c_frame(H, W1) + c_lane_off<DPL>(dl);
    int16_t* Sf = a.S + (size_t)frame * vol_frame(H, W1) + dl * DPL;
    const int x0 = HORIZ ? 0 : (XS == 0 ? cc : (XS > 0 ? cc - (H - 1) : cc));

    auto pos = [&](int t, int& x, int& y) {
        if (HORIZ) { x = XS > 0 ? t : W1 - 1 - t; y = cc; }
        else { y = YREV ? H - 1 - t : t; x = x0 + XS * t; }
    };
    auto pix_off = [&](int t) -> int {                         // pixel index of step t inside the frame
        int x, y; pos(t, x, y);
        x = min(max(x, 0), W1 - 1);
        return y * W1 + x;
    };

    const uint32_t P1pk = pk_bcast(a.P1), P2pk = pk_bcast(a.P2);
    const bool first_lane = dl == 0, last_lane = dl == LPP - 1;

    uint32_t p[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) p[i] = 0;
    uint32_t delta = P2pk;                                    // out-of-image predecessor: L = 0, min = 0

    typename CRaw<DPL>::type cq[PF]; Vec sq[PF];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const size_t o = (size_t)pix_off(min(tlo + j, thi - 1));
        cq[j] = *reinterpret_cast<const typename CRaw<DPL>::type*>(Cf + o * C_PXB);
        if (MODE != 0) sq[j] = *reinterpret_cast<const Vec*>(Sf + o * VOL_PX);
    }

    unsigned char* myS = sS + (MODE == 2 ? wib * 64 * WTA_ROWB : 0);

    for (int tb = tlo; tb < thi; tb += (MODE == 2 ? BS : PF)) {
#pragma unroll
        for (int jj = 0; jj < (MODE == 2 ? BS : PF); jj++) {
            const int j = jj % PF;
            const int t = tb + jj;
            if (t < thi) {
                uint32_t cv[NP], sv[NP], L[NP];
                vec_unpack<NP>(c_unpack(cq[j], dl, P2pk), cv);
                if (MODE != 0) vec_unpack<NP>(sq[j], sv);
                const size_t o = (size_t)pix_off(t) * VOL_PX;
                {   // refill this queue slot with step t + PF
                    const size_t on = (size_t)pix_off(min(t + PF, thi - 1));
                    cq[j] = *reinterpret_cast<const typename CRaw<DPL>::type*>(Cf + on * C_PXB);
                    if (MODE != 0) sq[j] = *reinterpret_cast<const Vec*>(Sf + on * VOL_PX);
                }
                uint32_t nd = chain_step<NP, LPP>(p, delta, cv, L, P1pk, P2pk, first_lane, last_lane);
                bool active = cvalid;
                if (!HORIZ && XS != 0) {
                    int x, y; pos(t, x, y);
                    active = cvalid && ((unsigned)x < (unsigned)W1);
#pragma unroll
                    for (int i = 0; i < NP; i++) L[i] = active ? L[i] : 0u;
                    nd = active ? nd : P2pk;
                }
#pragma unroll
                for (int i = 0; i < NP; i++) p[i] = L[i];
                delta = nd;
                if (MODE == 0) {
                    if (active) *reinterpret_cast<Vec*>(Sf + o) = Packer<NP>::go(L);
                } else {
#pragma unroll
                    for (int i = 0; i < NP; i++) sv[i] = pk_add_sat(sv[i], L[i]);
                    if (MODE == 1) {
                        if (active) *reinterpret_cast<Vec*>(Sf + o) = Packer<NP>::go(sv);
                    } else {
                        *reinterpret_cast<Vec*>(myS + (sub * BS + jj) * WTA_ROWB + dl * DPL * 2) = Packer<NP>::go(sv);
                    }
                }
            }
        }
        if (MODE == 2) {
            // lane = (chain, step-in-batch): one pixel per lane, all 64 costs read back from LDS
            const int wsub = lane / BS, wj = lane % BS;
            const int t = tb + wj;
            const int y = c0 + wsub;
            const int x = XS > 0 ? t : W1 - 1 - t;
            const bool valid = (y <= c1) && (t < thi);
            wta_pixel(myS + lane * WTA_ROWB, valid, x, y, frame, a);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// a-5/a-6, both horizontal paths + WTA in ONE launch (saves an S write, an S read and a C read per
// frame versus k_chain<H0, mode 1> + k_chain<H4, mode 2>).  The final S needs L_left(x) and L_right(x)
// of the same pixel, but the two recurrences run in opposite directions and a row of L (237 KB) fits
// nowhere on chip.  So: phase 1 sweeps left->right reading only C and drops a CHECKPOINT of the path
// state (DPL/2 + 1 registers per lane) every K pixels into a small global buffer; phase 2 walks the
// K-pixel blocks right->left: restore the checkpoint, recompute L_left for the block into registers,
// run L_right backwards over it, form S + L_left + L_right on chip and do the WTA tail.
// Cost: L_left is computed twice (+1 path of VALU), C is read twice, S once, never written.
// ------------------------------------------------------------------------------------------------
template <int DPL> struct HfC {
    typedef typename CRaw<DPL>::type Raw;
    // pointer to the lane's field of pixel (row, x = 0) and the load of pixel x
    static __device__ __forceinline__ const unsigned char* base(const unsigned char* C, int frame, int H, int W1, int row, int dl)
    {
        return C + (size_t)frame * c_frame(H, W1) + c_row(row, W1) + c_lane_off<DPL>(dl);
    }
    static __device__ __forceinline__ Raw load(const unsigned char* b, int x) { return c_load<DPL, false>(b + (size_t)x * C_PXB); }
};

// ---------------- phase 1: left -> right over blocks 0 .. nblk-2, checkpoint at every block start ----------------
// The checkpoints are written / read with streaming hints: they are re-read ~1 ms later, long after L2 has turned over, and as
// plain accesses they evict the C lines consecutive 96-byte pixels share (4.41 -> 4.22 ms per 34 frames)
template <int DPL>
__device__ __forceinline__ void hf_phase1(const unsigned char* Crow, uint32_t* ck, int nblk, int dl, uint32_t P1pk, uint32_t P2pk)
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, K = 64 / DPL;
    const bool first_lane = dl == 0, last_lane = dl == LPP - 1;
    uint32_t p[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) p[i] = 0;
    uint32_t delta = P2pk;
#pragma unroll
    for (int i = 0; i < NP; i++) __builtin_nontemporal_store(p[i], ck + i * 64);     // block 0: the zero state
    const int xend = (nblk - 1) * K;                       // the last block is recomputed in phase 2 anyway
    for (int xb = 0; xb < xend; xb += K) {
        // a block's K loads go out back to back: per row stream the DRAM sees one 2-KB burst, not 16 scattered lines
        typename HfC<DPL>::Raw cb[K];
#pragma unroll
        for (int jj = 0; jj < K; jj++) cb[jj] = HfC<DPL>::load(Crow, xb + jj);
#pragma unroll
        for (int jj = 0; jj < K; jj++) {
            uint32_t cv[NP], L[NP];
            vec_unpack<NP>(c_unpack(cb[jj], dl, P2pk), cv);
            delta = chain_step<NP, LPP>(p, delta, cv, L, P1pk, P2pk, first_lane, last_lane);
#pragma unroll
            for (int i = 0; i < NP; i++) p[i] = L[i];
        }
        uint32_t* c = ck + (size_t)(xb / K + 1) * NP * 64;
#pragma unroll
        for (int i = 0; i < NP; i++) __builtin_nontemporal_store(p[i], c + i * 64);
    }
}

// ---------------- phase 2, one K-pixel block: restore -> left path forwards, right path backwards -> S + both -> LDS ----------------
// Cb / Sb: the lane's field of the block's first pixel in C and S; p, delta: the left path's state at the block start
// (checkpoint); q, qdelta: the right path's state, carried from block to block; Sl: the lane's slot of the block's LAST
// pixel in the wave's WTA rows (pixel j of the block sits K - 1 - j rows further on).
// FULL (the block lies inside the row; nvalid == K): every load is base + a compile-time offset (j * C_PXB <= 1440 and
// j * VOL_PX * 2 <= 1920 fit the instruction's immediate) and the block is ONE basic block.  !FULL is the row's last block
// when W1 is not a multiple of K: pixels j >= nvalid re-read the row's last pixel (their left-path steps are never used)
// and the right path starts at pixel nvalid - 1.
template <int DPL, bool FULL>
__device__ __forceinline__ void hf_block(const unsigned char* Cb, const int16_t* Sb, int nvalid, uint32_t (&p)[DPL / 2], uint32_t delta,
                                         uint32_t (&q)[DPL / 2], uint32_t& qdelta, unsigned char* Sl, int dl, uint32_t P1pk, uint32_t P2pk)
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, K = 64 / DPL;
    typedef typename VecT<DPL>::type Vec;
    const bool first_lane = dl == 0, last_lane = dl == LPP - 1;
    typename HfC<DPL>::Raw craw[K]; Vec cvv[K], svv[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int xj = FULL ? j : min(j, nvalid - 1);
        craw[j] = HfC<DPL>::load(Cb, xj);
        svv[j] = ld_stream(reinterpret_cast<const Vec*>(Sb + (size_t)xj * VOL_PX));
    }
    uint32_t L0[K][NP];
#pragma unroll
    for (int j = 0; j < K; j++) {                          // forward recompute of the left path inside the block
        uint32_t cv[NP];
        cvv[j] = c_unpack(craw[j], dl, P2pk);              // unpacked once, as it arrives; the backward pass re-uses the int16 form
        vec_unpack<NP>(cvv[j], cv);
        delta = chain_step<NP, LPP>(p, delta, cv, L0[j], P1pk, P2pk, first_lane, last_lane);
#pragma unroll
        for (int i = 0; i < NP; i++) p[i] = L0[j][i];
    }
#pragma unroll
    for (int jj = 0; jj < K; jj++) {                       // right path, backwards
        const int j = K - 1 - jj;
        if (FULL || j < nvalid) {                          // uniform
            uint32_t cv[NP], sv[NP], L[NP];
            vec_unpack<NP>(cvv[j], cv);
            vec_unpack<NP>(svv[j], sv);
            qdelta = chain_step<NP, LPP>(q, qdelta, cv, L, P1pk, P2pk, first_lane, last_lane);
#pragma unroll
            for (int i = 0; i < NP; i++) { q[i] = L[i]; sv[i] = pk_add_sat(pk_add_sat(sv[i], L0[j][i]), L[i]); }
            *reinterpret_cast<Vec*>(Sl + jj * WTA_ROWB) = Packer<NP>::go(sv);
        }
    }
}

// PH: 3 = both phases in one launch; 2 = phase 2 only (k_hscan has dropped the checkpoints before)
template <int DPL, int PH>
__global__ __launch_bounds__(256, 4) void k_hfused(ChainArgs a, uint32_t* __restrict__ ckpt)      // four waves per SIMD: the 128-VGPR budget
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, PPW = DPL, K = 64 / PPW;
    __shared__ __attribute__((aligned(16))) unsigned char sS[4 * 64 * WTA_ROWB];

    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W1 = a.W1, H = a.H;
    const int groups = (H + PPW - 1) / PPW, total = groups * a.nframes;
    const int sub = lane / LPP, dl = lane % LPP;
    const int nblk = (W1 + K - 1) / K;
    const uint32_t P1pk = pk_bcast(a.P1), P2pk = pk_bcast(a.P2);
    unsigned char* myS = sS + wib * 64 * WTA_ROWB;
    // Ticketed form (a.persist): exactly the resident number of waves is launched and each draws (frame, row group) tickets
    // until none is left, instead of one wave per row group: no partly filled last "round" of the 4096 wave slots (34 frames
    // are 2.24 rounds).  Measured per 34 / 68 frames: 4.76 -> 4.56 ms / 9.46 -> 8.98 ms; 30 frames (1.98 rounds): unchanged.
    // (Also measured, round 3: letting the odd waves run their left-to-right scan one group AHEAD, so that both phases are on
    //  the chip at all times instead of all waves streaming, then all waves computing -- 4-7 % SLOWER at every batch size: the
    //  kernel does not suffer from its waves marching in step.)
    auto draw = [&]() -> int {
        int g = 0;
        if (lane == 0) g = atomicAdd(a.ticket, 1);
        return __builtin_amdgcn_readfirstlane(g);
    };
    int work = a.persist ? draw() : (a.xcd ? (int)xcd_linear(blockIdx.x, gridDim.x) : (int)blockIdx.x) * 4 + wib;
    for (;;) {
    if (work >= total) break;                                  // wave-uniform; no block-wide barriers anywhere
    {
    const int frame = work / groups, grp = work - frame * groups;
    const int c0 = grp * PPW, c1 = min(c0 + PPW, H) - 1;
    const int cc = min(c0 + sub, c1);
    const unsigned char* Crow = HfC<DPL>::base(a.C, frame, H, W1, cc, dl);
    const int16_t* Srow = a.S + (size_t)frame * vol_frame(H, W1) + vol_row(cc, W1) + dl * DPL;
    uint32_t* ck = ckpt + ((size_t)frame * groups + grp) * nblk * NP * 64 + lane;         // [blk][reg][lane]; delta is recomputed
    if (PH & 1) hf_phase1<DPL>(Crow, ck, nblk, dl, P1pk, P2pk);

    // ---------------- phase 2: right -> left, block by block ----------------
    uint32_t q[NP];
#pragma unroll
    for (int i = 0; i < NP; i++) q[i] = 0;
    uint32_t qdelta = P2pk;
    const unsigned char* Cb = Crow + (size_t)(nblk - 1) * K * C_PXB;                     // the block's first pixel in both row streams
    const int16_t* Sb = Srow + (size_t)(nblk - 1) * K * VOL_PX;
    unsigned char* Sl = myS + sub * K * WTA_ROWB + dl * DPL * 2;
    // WTA: lane = (row, pixel of the block).  The lanes of rows beyond the image's last repeat row c1 (as the chains above do):
    // same record to the same address, so the store needs no row predicate
    const int wsub = min(lane / K, c1 - c0), wj = lane % K, y = c0 + wsub;
    const unsigned char* Wl = myS + (wsub * K + wj) * WTA_ROWB;
    // (Round 2, 30 frames, same-box A/B, when the kernel waited on memory with its VALU 56 % busy: prefetching the next
    //  block's C/S into a second register set (182 VGPRs: half the occupancy, 1.84 -> 2.07 ms per 8 frames), issuing the next
    //  block's loads before this block's WTA tail, prefetching C one further block ahead (153 VGPRs), double- and
    //  triple-buffering phase 1's C blocks (119-122 VGPRs) -- all on the same 4.91-4.95 ms or slower; forced to 128 VGPRs the
    //  prefetching forms spill and take 6.6-7.1 ms.  Today's budget of the block, instruction by instruction: DESIGN.md section 4.)
    auto block = [&](int blk, auto full) {
        constexpr bool FULL = decltype(full)::value;
        const int x0 = blk * K;
        uint32_t p[NP];
        const uint32_t* c = ck + (size_t)blk * NP * 64;         // block 0 restores the zero state phase 1 has put there: no branch
#pragma unroll
        for (int i = 0; i < NP; i++) p[i] = __builtin_nontemporal_load(c + i * 64);
        const uint32_t delta = chain_delta<NP, LPP>(p, P2pk);
        hf_block<DPL, FULL>(Cb, Sb, FULL ? K : W1 - x0, p, delta, q, qdelta, Sl, dl, P1pk, P2pk);
        const int x = x0 + K - 1 - wj;
        wta_pixel(Wl, FULL || x < W1, x, y, frame, a);
        Cb -= K * C_PXB; Sb -= K * VOL_PX;
    };
    // the row's last block is the only one that can cross W1: peeled off, so that the loop runs the branch-free form alone
    int blk = nblk - 1;
    if (W1 % K) block(blk--, std::false_type());
    for (; blk >= 0; blk--) block(blk, std::true_type());
    }
    if (!a.persist) break;
    work = draw();
    }
}

// phase 1 of k_hfused as its own launch: it needs a dozen registers where phase 2 needs 119, so on its own it runs at twice
// the occupancy and keeps twice the bytes in flight per CU
template <int DPL>
__global__ __launch_bounds__(256, 8) void k_hscan(ChainArgs a, uint32_t* __restrict__ ckpt)
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, PPW = DPL, K = 64 / PPW;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W1 = a.W1, H = a.H;
    const int groups = (H + PPW - 1) / PPW;
    const int gw = (int)blockIdx.x * 4 + wib;
    const int frame = gw / groups, grp = gw - frame * groups;
    if (frame >= a.nframes) return;
    const int sub = lane / LPP, dl = lane % LPP;
    const int c0 = grp * PPW, c1 = min(c0 + PPW, H) - 1;
    const int cc = min(c0 + sub, c1);
    const int nblk = (W1 + K - 1) / K;
    uint32_t* ck = ckpt + ((size_t)frame * groups + grp) * nblk * NP * 64 + lane;
    hf_phase1<DPL>(HfC<DPL>::base(a.C, frame, H, W1, cc, dl), ck, nblk, dl, pk_bcast(a.P1), pk_bcast(a.P2));
}

// ------------------------------------------------------------------------------------------------
// a-5, the three top-down paths r1 = (x-1, y-1), r2 = (x, y-1), r3 = (x+1, y-1) in ONE pass over C
// (SURVEY 8a-5's K_v): reads C once, writes S = L1 + L2 + L3 once -- 2 volumes instead of the
// 7 that three k_chain launches move.
//
// The diagonals couple neighbouring columns row by row, so a column strip cannot run alone.  Here a
// workgroup (1024 threads = 16 waves, 16 lanes x 4 disparities per pixel) owns a strip of 64 columns of
// one frame and marches down the rows in LOCK-STEP with its two neighbour strips:
//   * inside the strip the previous row's (L1, L3) state is exchanged through LDS (one barrier per row);
//   * across strips the state of the column NEXT TO each edge column travels through global memory as 8-byte
//     {data, tag} granules (relaxed agent-scope atomic stores / loads: sc1, served by L2, no fences --
//     MI355X_MICROARCH "handoff-1to1"), tag = (call sequence << 12) | (row + 1), 8-row ring per strip edge
//     (VDD_RING; stays in L2).
// Row cycle.  Strip A's first pixel (column xs) needs L1(xs-1, y-1), a column of its left neighbour B.  If B published
// that column, A's row y would wait for B's row y-1 and B's row y for A's row y-1: one 2.7-us hop in every row's
// dependency cycle.  Instead B publishes the column before it, L1 and delta of (xs-2, y), and A's edge lanes form
//   L1(xs-1, y-1) = chain_step(L1(xs-2, y-2), delta1(xs-2, y-2), C(xs-1, y-1))
// themselves: B's own inputs, so B's bits.  Mirrored for L3 at the right edge (B's pixel 1, after the ragged rule: a
// last strip of one in-image column publishes (0, P2), the out-of-image state).  A's row y now waits for B's row y-2
// and B's row y for A's row y-2: one hop per TWO rows, a strip may run two rows ahead of a neighbour, and the granule
// an edge wave wants is a whole row period old.  That is what pays: the wave fetches it during the row BEFORE, one
// granule per lane, right after its own publish, so the L2 round trip runs behind the vertical step and the barrier
// and the row starts with a tag compare, not with a poll (measured: the rebuilt column with the poll still at the
// start of the row is 3 % SLOWER than the one-row hand-off, 3.27 -> 3.37 ms per 34 frames; with the early fetch
// 3.27-3.38 -> 3.16-3.21 ms.  Merging the rebuilt column into p1 / p3 in registers instead of through the LDS halo
// slot: 64 VGPRs and back to 3.24-3.32 ms).  Rows 0 and 1 start from the out-of-image state and poll nothing; a
// row is published only if a row y+2 exists.  Price: one more chain step per row on wave 0 / wave 15 and a 12-byte
// (8 at 4 disparities per lane) C fetch per edge lane, queued one row ahead.
// The coupling is bidirectional (strip k waits for k-1 AND k+1), so the strips of ONE FRAME must be co-resident;
// frames are independent.  Workgroups are dispatched in blockIdx order (per XCD, each XCD taking every 8th), so the
// resident set is always a prefix of the grid = whole frames plus at most one partial frame per XCD skew, and a
// partial frame merely waits (bounded spin) until finished frames free slots for its remaining strips: a launch
// larger than the chip -- or a chip that has lost slots to another tenant -- slows down instead of dead-locking
// (tests: a 768-workgroup launch on 512 slots).  The host still sizes launches to the occupancy query because a
// waiting partial frame costs a whole extra pass.  Every spin is bounded and trips an error flag instead of hanging.
// (Round 3, measured: drawing (frame, strip) from a ticket at workgroup start -- residency order by construction --
//  scatters neighbour strips over the XCDs and costs 3.38 -> 4.56 ms per 30 frames, like the XCD-contiguous order below;
//  the hardware's own blockIdx -> XCD round-robin, neighbours on adjacent XCDs, is the fast placement.)
// ------------------------------------------------------------------------------------------------
// poll budget of an edge wave over the whole pass (every poll round is one L2 round trip, ~1 us): a healthy pass spends
// none to three rounds per row, so 64 per row + slack is two orders of magnitude of headroom and still bounds a pass whose
// neighbours never become resident to ~0.1 s at 1080 rows (it was 2^20 rounds, i.e. seconds)
#define VDD_SPIN_PER_ROW 64
#define VDD_SPIN_SLACK 4096

struct VddArgs {
    const unsigned char* C; int16_t* S;
    int W1, H, nframes, nstrips;
    int P1, P2;
    uint32_t seq;
    int spin_limit;                     // poll rounds a lane may spend waiting over the whole pass
    unsigned long long* gran;           // [frame][strip][2 dirs][VDD_RING][VDD_GRAN]
    int* err;
    int xcd;                            // 1: XCD-contiguous strip order, co-resident launches only (launch_vdd).  Measured slower (3.48 -> 4.58 ms per 30 frames): off
};

// one {data, tag} granule.  An edge wave fetches a row's 33 granules one per lane: a single load instruction per poll
// round (one L2 round trip), two registers to hold the row
__device__ __forceinline__ unsigned long long vdd_get(const unsigned long long* g)
{
    return __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void vdd_put(unsigned long long* g, uint32_t v, uint32_t tag)
{
    __hip_atomic_store(g, ((unsigned long long)tag << 32) | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// YREV: the same pass bottom-up (MODE_HH's second half: predecessors (x-1,y+1), (x,y+1), (x+1,y+1)), accumulating
// into the S the top-down pass left behind (S += L1 + L2 + L3, saturating).
template <int DPL, bool YREV>
__global__ __launch_bounds__(1024, 8) void k_vdd(VddArgs a)      // 8 waves/SIMD = two workgroups per CU: the second hides the hand-off latency
{
    constexpr int NP = DPL / 2, LPP = 64 / DPL, PPW = DPL, PXS = 16 * PPW;   // PXS = columns per strip (64 / 128)
#ifndef V3D_VDD_PF8
#define V3D_VDD_PF8 2
#endif
    // C prefetch depth in rows.  The 64-VGPR budget of two workgroups per CU binds at DPL = 8: two rows of the 12-bit C (3 registers
    // per row; measured 3.34 -> 3.23 ms per 34 frames against one row); the bottom-up pass also queues S and has room for one
    constexpr int PF = DPL == 8 ? (YREV ? 1 : V3D_VDD_PF8) : 4;
    typedef typename VecT<DPL>::type Vec;
    // per-pixel exchanged state: LPP lanes x {L1 (NP dwords), L3 (NP dwords)} + per pixel {delta1, delta3}
    __shared__ Vec sL1[2][PXS + 2][LPP];
    __shared__ Vec sL3[2][PXS + 2][LPP];
    __shared__ uint2 sDl[2][PXS + 2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);    // wave index as an SGPR: edge-wave branches stay scalar
    const int px = wv * PPW + lane / LPP, dl = lane % LPP;      // pixel inside the strip, disparity group
    const int vb = a.xcd ? (int)xcd_linear(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int frame = vb / a.nstrips, strip = vb - frame * a.nstrips;
    const int W1 = a.W1, H = a.H;
    const int x = strip * PXS + px;
    const bool colok = x < W1;
    const bool ragged = __builtin_amdgcn_readfirstlane((strip + 1) * PXS > W1);   // this strip sticks out of the image
    const int xc = min(x, W1 - 1);
    const size_t fbase = (size_t)frame * vol_frame(H, W1);
    const unsigned char* Cp = a.C + (size_t)frame * c_frame(H, W1) + (size_t)xc * C_PXB + c_lane_off<DPL>(dl);
    int16_t* Sp = a.S + fbase + (size_t)xc * VOL_PX + dl * DPL;

    const uint32_t P1pk = pk_bcast(a.P1), P2pk = pk_bcast(a.P2);
    const bool first_lane = dl == 0, last_lane = dl == LPP - 1;
    const bool has_left = strip > 0, has_right = strip + 1 < a.nstrips;
    unsigned long long* gme = a.gran + ((size_t)(frame * a.nstrips + strip) * 2) * VDD_RING * VDD_GRAN;
    const unsigned long long* gleft = a.gran + ((size_t)(frame * a.nstrips + strip - 1) * 2 + 1) * VDD_RING * VDD_GRAN;   // left neighbour, right-going
    const unsigned long long* gright = a.gran + ((size_t)(frame * a.nstrips + strip + 1) * 2 + 0) * VDD_RING * VDD_GRAN;  // right neighbour, left-going
    const bool edge_l = has_left && wv == 0;                      // wave-uniform: this wave talks to the left strip
    const bool edge_r = has_right && wv == 15;                     //               ... to the right strip
    const bool lane_l = lane < LPP, lane_r = lane >= 64 - LPP;     // lanes of the strip's first / last pixel
    int budget = a.spin_limit;
    bool failed = a.spin_limit < 0 && tid == 0;                    // spin_limit -1: test hook, every workgroup reports a time-out

    // row -1: every path starts from the out-of-image state (L = 0, delta = P2)
    {
        uint32_t z[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) z[i] = 0u;
        for (int i = tid; i < 2 * (PXS + 2) * LPP; i += 1024) { (&sL1[0][0][0])[i] = Packer<NP>::go(z); (&sL3[0][0][0])[i] = Packer<NP>::go(z); }
        for (int i = tid; i < 2 * (PXS + 2); i += 1024) (&sDl[0][0])[i] = make_uint2(P2pk, P2pk);
    }
    uint32_t p2[NP], d2 = P2pk;
#pragma unroll
    for (int i = 0; i < NP; i++) p2[i] = 0u;

    typename CRaw<DPL>::type cq[PF];
    auto rowy = [&](int y) -> int { const int yc = min(y, H - 1); return YREV ? H - 1 - yc : yc; };
    auto rowof = [&](int y) -> size_t { return vol_row(rowy(y), W1); };
    auto ld_c = [&](int y) { return c_load<DPL, true>(Cp + c_row(rowy(y), W1)); };
    Vec sq[PF];
#pragma unroll
    for (int j = 0; j < PF; j++) { cq[j] = ld_c(j); if (YREV) sq[j] = ld_stream(reinterpret_cast<const Vec*>(Sp + rowof(j))); }
    __syncthreads();

    // The row loop exists twice: waves that own a strip-edge pixel (wave 0 / wave 15 of an inner strip) carry the
    // poll and publish code, the other 14 run a copy without it -- no merge copies of the polled registers, no
    // branch tests.  Every wave still executes one barrier per row.
    auto rows = [&](auto edge_tag) {
    constexpr bool EDGE = decltype(edge_tag)::value;
    // an edge wave is wave 0 or wave 15, never both, so one halo step per row serves either side
    const bool halo_lane = edge_l ? lane_l : lane_r;               // the lanes that rebuild the neighbour's edge column
    const bool pub_l = lane / LPP == 1, pub_r = lane / LPP == PPW - 2;   // pixel 1's L3 goes left, pixel PXS - 2's L1 goes right
    const unsigned long long* gin = edge_l ? gleft : gright;
    const ptrdiff_t halo_off = edge_l ? -(ptrdiff_t)C_PXB : (ptrdiff_t)C_PXB;   // column x0 - 1 / x0 + PXS, seen from the edge pixel
    const bool gran_lane = lane <= 32;                             // a row's 32 data granules + delta, one per lane
    typename CRaw<DPL>::type hq = {};                              // the halo column's C of the row before the current one
    unsigned long long gq = 0;                                     // the neighbour's granule of the row before that
    if constexpr (EDGE) if (halo_lane) hq = c_load<DPL, true>(Cp + c_row(rowy(0), W1) + halo_off);
    for (int y0 = 0; y0 < H; y0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            const int y = y0 + j;
            if (y < H) {                                           // uniform
                const int prev = (y + 1) & 1, cur = y & 1;         // buffer holding row y-1 / receiving row y
                __syncthreads();                                   // row y-1 of the whole strip is in buffer `prev`
                // ---- 0. edge waves: the neighbour's edge column of row y-1, rebuilt here from what the neighbour published of
                //         row y-2 -- a whole row period old, so it was fetched during row y-1 -- and the halo column's C of
                //         row y-1: one chain step, same inputs and so same bits as the neighbour's own.  After the barrier, so
                //         the other 14 waves compute meanwhile.  The result goes into the strip's LDS halo slot (slot 0 / PXS + 1
                //         of `prev`, which no other wave touches) and is read back below like any other predecessor: nothing
                //         of this step is live when the three regular steps start ----
                if constexpr (EDGE) if (y > 0) {
                    uint32_t hp[NP], hd = P2pk, hv[NP], hL[NP];
#pragma unroll
                    for (int i = 0; i < NP; i++) hp[i] = 0u;       // rows 0 and -1 of every column: the out-of-image state
                    if (y > 1) {
                        // the row's 33 granules sit one per lane in `gq`, fetched during row y-1: only a wave that runs ahead
                        // of its neighbour finds a stale tag and polls
                        const uint32_t tag = (a.seq << 12) | (uint32_t)(y - 1);        // row y-2 carries tag (y-2)+1
                        const unsigned long long* g = gin + ((y - 2) & (VDD_RING - 1)) * VDD_GRAN + lane;
                        while (__builtin_amdgcn_ballot_w64(gran_lane && (uint32_t)(gq >> 32) != tag)) {      // wave-uniform
                            if (--budget < 0) { failed = failed || lane == 0; budget = 0; break; }
                            __builtin_amdgcn_s_sleep(1);
                            if (gran_lane) gq = vdd_get(g);
                        }
#pragma unroll
                        for (int i = 0; i < NP; i++) hp[i] = (uint32_t)__builtin_amdgcn_ds_bpermute((NP * dl + i) * 4, (int)(uint32_t)gq);
                        hd = (uint32_t)__builtin_amdgcn_ds_bpermute(32 * 4, (int)(uint32_t)gq);
                    }
                    vec_unpack<NP>(c_unpack(hq, dl, P2pk), hv);
                    if (halo_lane) hq = c_load<DPL, true>(Cp + c_row(rowy(y), W1) + halo_off);    // for row y+1
                    const uint32_t hnd = chain_step<NP, LPP>(hp, hd, hv, hL, P1pk, P2pk, first_lane, last_lane);
                    if (halo_lane) {
                        if (edge_l) { sL1[prev][0][dl] = Packer<NP>::go(hL); if (dl == 0) sDl[prev][0].x = hnd; }
                        else { sL3[prev][PXS + 1][dl] = Packer<NP>::go(hL); if (dl == 0) sDl[prev][PXS + 1].y = hnd; }
                    }
                }
                // ---- 1. predecessors: row y-1 of the columns x-1 and x+1 from LDS ----
                uint32_t cv[NP], p1[NP], p3[NP];
                uint32_t sold[NP];
                // (12-bit C: unpacking the NEXT row at the end of this one, off the path between the barrier and the recurrences
                //  the neighbour strips wait for, was measured: 3.32 -> 3.49 ms per 34 frames -- one more row of raw fields and
                //  an unpacked row live across the barrier cost more than the ~18 ops they move)
                vec_unpack<NP>(c_unpack(cq[j], dl, P2pk), cv);
                if (YREV) vec_unpack<NP>(sq[j], sold);
                cq[j] = ld_c(y + PF);
                if (YREV) sq[j] = ld_stream(reinterpret_cast<const Vec*>(Sp + rowof(y + PF)));
                vec_unpack<NP>(sL1[prev][px][dl], p1);             // column x-1 (slot px holds pixel px-1)
                vec_unpack<NP>(sL3[prev][px + 2][dl], p3);         // column x+1
                uint32_t d1 = sDl[prev][px].x, d3 = sDl[prev][px + 2].y;
                // ---- 2. the two diagonal recurrences first: their edge values are what the neighbour strips wait for ----
                uint32_t L1[NP], L2[NP], L3[NP];
                uint32_t nd1 = chain_step<NP, LPP>(p1, d1, cv, L1, P1pk, P2pk, first_lane, last_lane);
                uint32_t nd3 = chain_step<NP, LPP>(p3, d3, cv, L3, P1pk, P2pk, first_lane, last_lane);
                if (ragged) if (!colok) {                           // columns beyond the image (last strip only; `ragged`
#pragma unroll                                                      //  is uniform, so full strips skip the block): out-of-image state
                    for (int i = 0; i < NP; i++) L1[i] = L3[i] = 0u;
                    nd1 = nd3 = P2pk;
                }
                // ---- 3. publish row y as early as possible: granules for the neighbours, LDS for the strip ----
                if constexpr (EDGE) if (y + 2 < H) {               // row y is read by the neighbours' row y + 2
                    const uint32_t tag = (a.seq << 12) | (uint32_t)(y + 1);
                    const int slot = y & (VDD_RING - 1);
                    if (edge_r) if (pub_r) {                        // L1 of the column before my last goes right
                        unsigned long long* g = gme + (size_t)(1 * VDD_RING + slot) * VDD_GRAN;
#pragma unroll
                        for (int i = 0; i < NP; i++) vdd_put(g + NP * dl + i, L1[i], tag);
                        if (dl == 0) vdd_put(g + 32, nd1, tag);
                    }
                    if (edge_l) if (pub_l) {                        // L3 of the column after my first goes left
                        unsigned long long* g = gme + (size_t)(0 * VDD_RING + slot) * VDD_GRAN;
#pragma unroll
                        for (int i = 0; i < NP; i++) vdd_put(g + NP * dl + i, L3[i], tag);
                        if (dl == 0) vdd_put(g + 32, nd3, tag);
                    }
                }
                sL1[cur][px + 1][dl] = Packer<NP>::go(L1);
                sL3[cur][px + 1][dl] = Packer<NP>::go(L3);
                if (dl == 0) sDl[cur][px + 1] = make_uint2(nd1, nd3);
                // the neighbour's row y-1, which row y+1 will want: published about one row period ago, fetched behind the
                // vertical step and the barrier instead of after it
                if constexpr (EDGE) if (y > 0 && y + 1 < H) if (gran_lane) gq = vdd_get(gin + ((y - 1) & (VDD_RING - 1)) * VDD_GRAN + lane);
                // ---- 4. the vertical recurrence and the sum ----
                const uint32_t nd2 = chain_step<NP, LPP>(p2, d2, cv, L2, P1pk, P2pk, first_lane, last_lane);
#pragma unroll
                for (int i = 0; i < NP; i++) p2[i] = L2[i];
                d2 = nd2;
                if (colok) {
                    uint32_t o[NP];
#pragma unroll
                    for (int i = 0; i < NP; i++) { o[i] = pk_add_sat(pk_add_sat(L1[i], L2[i]), L3[i]); if (YREV) o[i] = pk_add_sat(o[i], sold[i]); }
                    st_stream(reinterpret_cast<Vec*>(Sp + rowof(y)), Packer<NP>::go(o));
                }

            }
        }
    }
    };
    if (edge_l || edge_r) rows(std::true_type{}); else rows(std::false_type{});
    if (failed) atomicAdd(a.err, 1);
}

// ------------------------------------------------------------------------------------------------
// Lock-step guard: the last launch of a compute call that used k_vdd.  If any strip of this handle has timed out
// since the counter was last cleared, the caller must never consume the disparities: every output pixel becomes
// INVALID and a flag lands in host-visible memory (the next API call on the handle then returns V3D_ERR_LOCKSTEP).
// Healthy path: one dword load per workgroup.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vdd_guard(const int* __restrict__ err, volatile int* err_host, int16_t* __restrict__ out, size_t n, int invalid)
{
    const int e = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (e == 0) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *err_host = e; __threadfence_system(); }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = (int16_t)invalid;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// resident k_vdd workgroups per CU of each mapping (the bottom-up form needs the most registers)
void sgbm_vdd_occupancy(int* wg_per_cu_dpl4, int* wg_per_cu_dpl8)
{
    *wg_per_cu_dpl4 = *wg_per_cu_dpl8 = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(wg_per_cu_dpl4, k_vdd<4, true>, 1024, 0);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(wg_per_cu_dpl8, k_vdd<8, true>, 1024, 0);
}

// frames one lock-step launch should hold at cost-region width W1: the workgroup slots the occupancy query reports
// (minus the CUs the host says other streams keep busy, two slots each) over the strips of one frame.  No safety
// margin: an over-sized launch is slow, not wrong (k_vdd: in-order dispatch keeps whole frames resident).
int sgbm_vdd_frames_per_launch(const v3d_sgbm* h, int dpl, int W1)
{
    const int cus = h->ncu - h->reserve_cus > 0 ? h->ncu - h->reserve_cus : 0;
    return ((dpl == 8 ? h->vdd_occ8 : h->vdd_occ4) * cus) / v3d_cdiv(W1, 16 * dpl);
}

template <bool HORIZ, int XS, bool YREV, int MODE>
static void launch_chain(const v3d_sgbm* h, const ChainArgs& a, hipStream_t st)
{
    const int NC = HORIZ ? a.H : (XS == 0 ? a.W1 : a.W1 + a.H - 1);
    if (h->dpl == 4) {
        const int groups = v3d_cdiv(NC, 4), waves = groups * a.nframes;
        hipLaunchKernelGGL((k_chain<HORIZ, XS, YREV, MODE, 4>), dim3(v3d_cdiv(waves, 4)), dim3(256), 0, st, a);
    } else {
        const int groups = v3d_cdiv(NC, 8), waves = groups * a.nframes;
        hipLaunchKernelGGL((k_chain<HORIZ, XS, YREV, MODE, 8>), dim3(v3d_cdiv(waves, 4)), dim3(256), 0, st, a);
    }
}

// one lock-step pass over the three top-down (or, rev, bottom-up) paths; frames per launch bounded by co-residency.
// mapping: 4 disparities per lane (64-column strips) while the whole batch fits one co-resident launch, else
// 8 per lane (128-column strips: ~30 % fewer instructions per element, twice the frames per launch)
static void launch_vdd(v3d_sgbm* h, int n, int W1, int H, bool rev, hipStream_t st)
{
    // sized from THIS call's width (a handle made for 4K frames holds more 1080p frames per launch)
    const int mf4 = sgbm_vdd_frames_per_launch(h, 4, W1), mf8 = sgbm_vdd_frames_per_launch(h, 8, W1);
    const int dpl = h->vdd_dpl ? h->vdd_dpl : (n <= mf4 ? 4 : 8);
    const int mf = h->vdd_launch_frames > 0 ? h->vdd_launch_frames : dpl == 8 ? (mf8 > 0 ? mf8 : 1) : (mf4 > 0 ? mf4 : 1);
    const int nl = v3d_cdiv(n, mf), per = v3d_cdiv(n, nl);           // equal shares: two launches of 20, not 34 + 6
    for (int f0 = 0; f0 < n; f0 += per) {
        VddArgs v;
        const int nf = n - f0 < per ? n - f0 : per;
        v.C = h->C + (size_t)f0 * c_frame(H, W1); v.S = h->S + (size_t)f0 * vol_frame(H, W1);
        v.W1 = W1; v.H = H; v.nframes = nf; v.nstrips = v3d_cdiv(W1, 16 * dpl); v.P1 = h->P1; v.P2 = h->P2;
        v.seq = (h->vdd_seq++) & 0xFFFFFu;
        if (v.seq == 0) {                                   // the 20-bit launch sequence wrapped: sweep the stale tags (once per 2^20 launches)
            (void)hipMemsetAsync(h->gran, 0, h->gran_bytes, st);
            v.seq = (h->vdd_seq++) & 0xFFFFFu;
        }
        v.gran = h->gran; v.err = h->vdd_err;
        // the XCD order is a speed switch and must never cost forward progress: a launch beyond the co-residency bound relies on
        // dispatch order = strip order (k_vdd), which the permutation breaks -- a frame across two XCDs' ranges would have some
        // strips resident first and the others last, and the first would spin their budget away
        v.xcd = h->vdd_xcd && nf <= (dpl == 8 ? mf8 : mf4);
        v.spin_limit = h->vdd_spin_limit != 0 ? h->vdd_spin_limit : VDD_SPIN_PER_ROW * H + VDD_SPIN_SLACK;
        const dim3 grid(v.nstrips * nf), block(1024);
        if (dpl == 8) { if (rev) hipLaunchKernelGGL((k_vdd<8, true>), grid, block, 0, st, v); else hipLaunchKernelGGL((k_vdd<8, false>), grid, block, 0, st, v); }
        else { if (rev) hipLaunchKernelGGL((k_vdd<4, true>), grid, block, 0, st, v); else hipLaunchKernelGGL((k_vdd<4, false>), grid, block, 0, st, v); }
    }
}

// C -> S (every path but the last) -> WTA records, between the events ST_V2 and ST_LRCHECK that run_sgbm records.
// *lockstep_ran: the top-down paths went through k_vdd, so the call must end with sgbm_lockstep_guard
int sgbm_aggregate_wta(v3d_sgbm* h, int n, int W, int H, hipStream_t st, bool* lockstep_ran)
{
    const int W1 = W - V3D_D;
    ChainArgs a;
    a.C = h->C; a.S = h->S; a.W1 = W1; a.H = H; a.W = W; a.nframes = n; a.P1 = h->P1; a.P2 = h->P2; a.uniq = h->uniq;
    a.t1_mul = h->t1_mul; a.t1_shift = h->t1_shift;
    a.wta = h->wta; a.xcd = h->hf_xcd; a.persist = 0; a.ticket = h->hf_ticket;
    // direction order is free (sums commute; saturation of non-negative addends is order-independent)
    const bool use_vdd = vdd_usable(h) && H < 4095;         // k_vdd's tag holds row + 1 in 12 bits
    *lockstep_ran = use_vdd;
    if (use_vdd) {
        launch_vdd(h, n, W1, H, false, st);                 // r1 + r2 + r3 in one lock-step pass
        prof_mark(h, ST_D1, st);
        prof_mark(h, ST_D3, st);
        V3D_HIP_CHECK(hipEventRecord(h->vdd_done_ev, st));       // v3d_sgbm_stream_wait_lockstep: other streams may order behind the pass
        h->vdd_ev_recorded = true;
    } else {
        launch_chain<false, 0, false, 0>(h, a, st);         // r2: (x, y-1)
        prof_mark(h, ST_D1, st);
        launch_chain<false, 1, false, 1>(h, a, st);         // r1: (x-1, y-1)
        prof_mark(h, ST_D3, st);
        launch_chain<false, -1, false, 1>(h, a, st);        // r3: (x+1, y-1)
    }
    prof_mark(h, ST_H0, st);
    if (!h->hfused) launch_chain<true, 1, false, 1>(h, a, st);          // r0: (x-1, y)
    prof_mark(h, ST_V2R, st);
    if (h->prm.mode == V3D_MODE_HH) {
        if (use_vdd) {
            launch_vdd(h, n, W1, H, true, st);              // (x-1,y+1), (x,y+1), (x+1,y+1) in one bottom-up lock-step pass
            prof_mark(h, ST_D1R, st); prof_mark(h, ST_D3R, st);
            V3D_HIP_CHECK(hipEventRecord(h->vdd_done_ev, st));
        } else {
            launch_chain<false, 0, true, 1>(h, a, st);      // (x, y+1)
            prof_mark(h, ST_D1R, st);
            launch_chain<false, -1, true, 1>(h, a, st);     // (x+1, y+1)
            prof_mark(h, ST_D3R, st);
            launch_chain<false, 1, true, 1>(h, a, st);      // (x-1, y+1)
        }
    } else { prof_mark(h, ST_D1R, st); prof_mark(h, ST_D3R, st); }
    prof_mark(h, ST_H4_WTA, st);
    if (h->hfused) {                                    // r0 + r4 + WTA tail in one launch
        const dim3 g4(v3d_cdiv(v3d_cdiv(H, 4) * n, 4)), g8(v3d_cdiv(v3d_cdiv(H, 8) * n, 4));
        if (h->hsplit) {
            if (h->dpl == 4) { hipLaunchKernelGGL(k_hscan<4>, g4, dim3(256), 0, st, a, h->ckpt); hipLaunchKernelGGL((k_hfused<4, 2>), g4, dim3(256), 0, st, a, h->ckpt); }
            else { hipLaunchKernelGGL(k_hscan<8>, g8, dim3(256), 0, st, a, h->ckpt); hipLaunchKernelGGL((k_hfused<8, 2>), g8, dim3(256), 0, st, a, h->ckpt); }
        } else {
            dim3 l4 = g4, l8 = g8;
            if (h->hf_persist) {                            // resident waves only: 4 workgroups of 4 waves per CU (LDS / 119 VGPRs)
                a.persist = h->hf_persist;
                V3D_HIP_CHECK(hipMemsetAsync(h->hf_ticket, 0, sizeof(int), st));
                const unsigned res = (unsigned)h->ncu * 4u;
                if (l4.x > res) l4.x = res;
                if (l8.x > res) l8.x = res;
            }
            if (h->dpl == 4) hipLaunchKernelGGL((k_hfused<4, 3>), l4, dim3(256), 0, st, a, h->ckpt);
            else hipLaunchKernelGGL((k_hfused<8, 3>), l8, dim3(256), 0, st, a, h->ckpt);
        }
    } else
        launch_chain<true, -1, false, 2>(h, a, st);     // r4: (x+1, y), + WTA tail
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// time-outs of this call's (or an earlier, uncleared) lock-step pass: poison `out`, raise the host flag
int sgbm_lockstep_guard(v3d_sgbm* h, int16_t* out, size_t npx, hipStream_t st)
{
    hipLaunchKernelGGL(k_vdd_guard, dim3(256), dim3(256), 0, st, h->vdd_err, h->err_host, out, npx, 16 * (h->prm.minDisparity - 1));
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
