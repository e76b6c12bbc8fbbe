// v3d_sgbm_internal.h -- what more than one stage of the SGBM needs: the layout of its volumes, the codecs of the cost
// volume and of the WTA record, the handle, and the stage entry points.  The stages:
//   v3d_sgbm_cost.hip   a-4      k_prefilter + k_cost -> C
//   v3d_sgbm_paths.hip  a-5/a-6  k_vdd (the three top-down paths in one lock-step pass) + k_hfused (both horizontal paths +
//                                WTA tail), k_chain (one launch per path direction) behind the options "lockstep" / "hfused"
//   v3d_sgbm_post.hip   a-7/a-8  k_lrcheck_median + k_ccl_*
//   v3d_sgbm.hip                 the handle and the C-ABI: run_sgbm is the sequence of the stage calls below
//
// HBM layout (per frame, W1 = W - 64):
//   rec        : uint4 [H][W]        pre-filter records, left then right image: {grad, grad_lo, grad_hi, 0 | raw, raw_lo, raw_hi, 0}
//   C          : 12-bit [H][W1][64]  d fastest: one pixel = 96 bytes
//   S          : int16 [H][W1][64]   d fastest: one pixel = one 128-B line
//   wta        : u32 [H][W]          WTA record per pixel (min S, sub-pixel disparity, winning d); the right-view map is
//                                    formed from it inside k_lrcheck_median (LDS min-scatter), never in HBM
#pragma once
#include "v3d_common.h"
#include <vector>

// S (aggregated costs): int16 [H][W1][64] -- offsets in ELEMENTS
#define VOL_PX V3D_D                                               // elements between pixel x and x + 1 of a row
__host__ __device__ static inline size_t vol_row(int y, int W1) { return (size_t)y * W1 * V3D_D; }
__host__ __device__ static inline size_t vol_frame(int H, int W1) { return (size_t)H * W1 * V3D_D; }
// C (matching costs): [H][W1] pixels of C_PXB bytes -- offsets in BYTES.  A pixel is 64 x 12 bits, disparity d at bit 12 d,
// holding C - P2 (the 5x5 box sum alone: <= 25 * 93 = 2325 < 4096); every reader adds P2 back as it unpacks, so the recurrences
// see C as int16.  A quarter fewer bytes than int16 on each of C's four touches (one write, three reads).
#define C_PXB 96
__host__ __device__ static inline size_t c_row(int y, int W1) { return (size_t)y * W1 * C_PXB; }
__host__ __device__ static inline size_t c_frame(int H, int W1) { return (size_t)H * W1 * C_PXB; }

template <int DPL> struct VecT;
template <> struct VecT<8> { typedef uint4 type; };
template <> struct VecT<4> { typedef uint2 type; };
template <int NP> __device__ __forceinline__ void vec_unpack(const uint4& v, uint32_t (&r)[NP]) { r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
template <int NP> __device__ __forceinline__ void vec_unpack(const uint2& v, uint32_t (&r)[NP]) { r[0] = v.x; r[1] = v.y; }
template <int NP> struct Packer;
template <> struct Packer<4> { static __device__ __forceinline__ uint4 go(const uint32_t (&r)[4]) { return make_uint4(r[0], r[1], r[2], r[3]); } };
template <> struct Packer<2> { static __device__ __forceinline__ uint2 go(const uint32_t (&r)[2]) { return make_uint2(r[0], r[1]); } };

// ---- a lane's view of C: DPL disparities of one pixel.  CRaw is what it fetches, c_unpack turns it into DPL/2 packed int16 pairs ----
typedef uint32_t v3d_u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t v3d_u32x3_a4 __attribute__((ext_vector_type(3), aligned(4)));
template <int DPL> struct CRaw;
template <> struct CRaw<8> { typedef v3d_u32x3_a4 type; };      // the lane's 8 x 12 bits: 12 bytes at byte 12 dl of the pixel
template <> struct CRaw<4> { typedef v3d_u32x2_a4 type; };      // 8 bytes from the dword boundary at or below byte 6 dl: the lane's 48 bits start at bit (dl & 1) * 16
template <int DPL> __device__ __forceinline__ int c_lane_off(int dl) { return DPL == 8 ? 12 * dl : (6 * dl) & ~3; }
__device__ __forceinline__ uint32_t unpack12_pair(uint32_t t) { return (t & 0xFFFu) | ((t << 4) & 0x0FFF0000u); }     // bits 0-11 | 12-23 -> two halves
__device__ __forceinline__ uint4 c_unpack(const v3d_u32x3_a4& v, int, uint32_t P2pk)
{
    return make_uint4(pk_add(unpack12_pair(v.x), P2pk), pk_add(unpack12_pair(alignbit(v.y, v.x, 24)), P2pk),
                      pk_add(unpack12_pair(alignbit(v.z, v.y, 16)), P2pk), pk_add(unpack12_pair(v.z >> 8), P2pk));
}
__device__ __forceinline__ uint2 c_unpack(const v3d_u32x2_a4& v, int dl, uint32_t P2pk)
{
    const uint32_t sh = (uint32_t)(dl & 1) * 16u;
    const uint32_t lo = alignbit(v.y, v.x, sh), hi = v.y >> sh;                 // the lane's 48 bits: lo, hi[15:0]
    return make_uint2(pk_add(unpack12_pair(lo), P2pk), pk_add(unpack12_pair(alignbit(hi, lo, 24)), P2pk));
}
// load of a lane's field; p = pixel base + c_lane_off.  STREAM: non-temporal (k_vdd: every line is touched by one load).  With
// 96-byte pixels k_hfused's consecutive pixel loads share cache lines (pixel k starts at 96 k): there the plain load keeps the
// line in L1 for the next pixel (measured: 4.52 -> 4.30 ms per 34 frames; the same switch costs k_vdd 1.5 %)
template <int DPL, bool STREAM> __device__ __forceinline__ typename CRaw<DPL>::type c_load(const unsigned char* p)
{
    if (STREAM) return __builtin_nontemporal_load(reinterpret_cast<const typename CRaw<DPL>::type*>(p));
    return *reinterpret_cast<const typename CRaw<DPL>::type*>(p);
}

// WTA record of one cost-region pixel: [31:17] min S (< 32767), [16:6] d16 + 16 (0 = invalid pixel), [5:0] winning d.
// One plain store per pixel; the right-view map is formed from these records in k_lrcheck_median.
__device__ __forceinline__ uint32_t wta_word(int minS, int d16, int best) { return ((uint32_t)minS << 17) | ((uint32_t)(d16 + 16) << 6) | (uint32_t)best; }
__device__ __forceinline__ int wta_d16(uint32_t w) { return (int)((w >> 6) & 0x7FFu) - 16; }

// k_vdd's edge granules: [frame][strip][2 directions][VDD_RING rows][VDD_GRAN] of 8 bytes
// Ring depth.  A strip reads its neighbour's row r - 2 in its own row r (k_vdd, "row cycle").  Strip B writes row r only
// after its poll of A's row r - 2 has returned; A published that row in its own iteration r - 2, after that iteration's poll
// of B's row r - 4 had returned (poll and publish are the same wave's, in program order).  So when B overwrites a slot with
// row r, A has finished with B's rows <= r - 4 and rows r - 3 .. r are live: 4 slots suffice.  8 is twice that.
#define VDD_RING 8
#define VDD_GRAN 34                      // granules per edge per row: 32 data dwords + delta (+1 pad)

// ------------------------------------------------------------------------------------------------
// the handle; every default is the measured best (v3d_sgbm_set_option changes the tuning fields)
// ------------------------------------------------------------------------------------------------
struct v3d_sgbm {
    v3d_sgbm_params prm;
    int device, maxW, maxH, maxB;
    int P1, P2, ftzero, uniq, d12;
    uint32_t t1_mul = 0; int t1_shift = 0;       // v3d_t1_magic(100 - uniq)
    int dpl = 4;                                // disparities per lane in k_chain and k_hfused (4 or 8)
    uint4* rec = nullptr;
    unsigned char* C = nullptr;                 // cost volume, C_PXB bytes per pixel
    int16_t* S = nullptr;
    uint32_t* wta = nullptr;                    // WTA records, one per pixel
    uint32_t* ckpt = nullptr;                   // k_hfused checkpoints
    unsigned long long* gran = nullptr;         // k_vdd edge granules
    size_t gran_bytes = 0;
    int* vdd_err = nullptr;
    uint32_t vdd_seq = 1;                       // running count of lock-step launches; a launch carries its low 20 bits, never 0 (launch_vdd)
    int vdd_mode = 1;                           // 1: lock-step pass (k_vdd), 0: three k_chain launches
    int vdd_dpl = 0;                            // forced k_vdd mapping (4 / 8), 0 = choose per call
    int cost_band = 90;                         // rows per k_cost workgroup
    int vdd_xcd = 0, cost_xcd = 1, hf_xcd = 0;  // measured: XCD-contiguous order pays for k_cost only
    int lrm_tiles = 0;                          // 1: L-R check + median as 128 x 16 tiles instead of the row march
    int hf_persist = 1;                         // k_hfused: 0 one wave per row group, 1 resident waves draw row groups from a ticket counter
                                                // (measured: -4 % at 34 / 68 frames, neutral at 30)
    int* hf_ticket = nullptr;
    int vdd_mf4 = 0, vdd_mf8 = 0;               // frames per launch of each mapping at maxW (reported by get_option)
    int vdd_occ4 = 0, vdd_occ8 = 0, ncu = 0;    // occupancy query results the bounds are derived from
    int reserve_cus = 0;                        // CUs left to other streams' kernels (e.g. an RCCL collective) when sizing a lock-step launch
    int vdd_launch_frames = 0;                  // 0 = size launches from the occupancy query; > 0: frames per launch (tests: over-sized launches)
    int vdd_spin_limit = 0;                     // 0 = derive from the row count
    int* err_host = nullptr;                    // pinned, device-visible: lock-step time-outs seen by k_vdd_guard
    hipEvent_t vdd_done_ev = nullptr;           // recorded behind the last lock-step launch of a compute call
    bool vdd_ev_recorded = false;
    int hfused = 1;                             // 1: both horizontal paths + WTA in one launch (k_hfused), 0: two k_chain launches
    int hsplit = 0;                             // 1: left->right scan of the horizontal pass as its own launch (k_hscan)
    int32_t* labels = nullptr;
    size_t bytes = 0;
    // optional per-stage HIP-event timing (v3d_sgbm_profile): events live on the caller's stream
    bool prof_on = false;
    int prof_calls = 0;
    std::vector<hipEvent_t> prof_ev;            // [call][V3D_NSTAGE + 1]
};

enum { ST_PREFILTER = 0, ST_COST, ST_V2, ST_D1, ST_D3, ST_H0, ST_V2R, ST_D1R, ST_D3R, ST_H4_WTA, ST_LRCHECK, ST_MEDIAN, ST_SPECKLE, V3D_NSTAGE };
#define V3D_PROF_MAX_CALLS 512

// record the event that closes stage `slot` - 1 and opens `slot`; stages that are skipped record nothing
static inline void prof_mark(v3d_sgbm* h, int slot, hipStream_t stm)
{
    if (!h->prof_on || h->prof_calls >= V3D_PROF_MAX_CALLS) return;
    (void)hipEventRecord(h->prof_ev[(size_t)h->prof_calls * (V3D_NSTAGE + 1) + slot], stm);
}

// ---- the stages, for n frames of W x H on stream st.  Each returns V3D_OK or an error code with v3d_set_error's text set,
// and records the events that open its own stages; run_sgbm records the one that follows each call ----
// v3d_sgbm_cost.hip
int sgbm_cost_volume(v3d_sgbm* h, const uint8_t* left, const uint8_t* right, int n, int W, int H, int pitch, size_t frame_stride, hipStream_t st);
int sgbm_export_cost(const v3d_sgbm* h, int W, int H, int16_t* C_out, hipStream_t st);     // C of one frame as int16 [H][W - 64][64], P2 folded in
// v3d_sgbm_paths.hip
void sgbm_vdd_occupancy(int* wg_per_cu_dpl4, int* wg_per_cu_dpl8);                         // resident k_vdd workgroups per CU
int sgbm_vdd_frames_per_launch(const v3d_sgbm* h, int dpl, int W1);
static inline bool vdd_usable(const v3d_sgbm* h) { return h->vdd_mode && h->vdd_mf4 >= 1 && h->vdd_mf8 >= 1; }
int sgbm_aggregate_wta(v3d_sgbm* h, int n, int W, int H, hipStream_t st, bool* lockstep_ran);   // C -> S -> WTA records
int sgbm_lockstep_guard(v3d_sgbm* h, int16_t* out, size_t npx, hipStream_t st);             // after a lock-step pass: time-outs poison `out`
// v3d_sgbm_post.hip
int sgbm_lrcheck_median(const v3d_sgbm* h, int n, int W, int H, int16_t* out, bool med, hipStream_t st);   // WTA records -> disparities
int sgbm_speckles(const v3d_sgbm* h, int16_t* out, int n, int W, int H, hipStream_t st);
