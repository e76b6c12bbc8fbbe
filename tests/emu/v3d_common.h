// Host stand-in for csrc/v3d_common.h, for the emulated tests (tests/test_*_emulated.py) only: a kernel source of csrc/ is compiled
// as plain C++ against it.  The threads of a workgroup (at most 1024, in one or two dimensions; a wave = 64 consecutive linear ids)
// are fibers that a scheduler runs, in ascending or descending id order, until each waits at a rendezvous:
// __syncthreads() / __syncthreads_or() for the workgroup; a wave shuffle, ballot, readlane or DPP move for the lanes of its wave.  Workgroups run one after
// another, in ascending or descending order; dynamic LDS is a fresh poisoned heap block of exactly the launch's byte count per
// workgroup, static __shared__ arrays are plain statics; atomics are plain read-modify-writes (one fiber runs at a time).
// It covers what the emulated sources use and nothing more.  Nothing here is used by the product.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>
#include <ucontext.h>
#include <algorithm>
#include <vector>
#include <functional>
#include "v3d_hip.h"
#include "v3d_depth_math.h"
using std::min; using std::max;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(8) uint2 { uint32_t x, y; };
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(8) int2 { int x, y; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
static inline int4 make_int4(int a, int b, int c, int d) { return int4{a, b, c, d}; }
typedef void* hipStream_t;
typedef int hipError_t;
typedef void* hipEvent_t;                                      // v3d_sgbm_internal.h names it in the handle; nothing is ever recorded
static inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return 0; }
#define hipSuccess 0
#define hipFuncAttributeMaxDynamicSharedMemorySize 8
static inline hipError_t hipFuncSetAttribute(const void*, int, int) { return hipSuccess; }
#define V3D_HIP_CHECK(expr) do { (void)(expr); } while (0)
#define V3D_LAUNCH_CHECK() do {} while (0)
#define V3D_D 64
#define V3D_MAX_COST 32767
#define V3D_INVALID16 (-16)

struct Fiber { ucontext_t ctx; void* sp; dim3 tid; int lin; bool done; char* stack; size_t stack_size; char* stale; };
extern Fiber* g_cur; extern dim3 blockIdx, gridDim, blockDim;
#define threadIdx (g_cur->tid)
void fiber_yield();
extern int g_nthreads;
extern long g_progress;                                        // counts released rendezvous and finished fibers: the deadlock watch
extern unsigned char* g_lds;                                   // the launch's dynamic LDS: what `extern __shared__ ... smem[]` becomes
static inline int emu_wave_lanes(int w) { return min(64, g_nthreads - 64 * w); }

// rendezvous number ph of this thread.  Nobody reaches rendezvous ph + 1's wait before all have arrived at ph, so at most two
// slots of a ring are live; a slot is cleared again half a ring later
#define EMU_MAX_THREADS 1024                                   // a CDNA workgroup: 16 waves
#define EMU_RING 8
static inline int __syncthreads_or(int pred)
{
    extern long g_bar_count[]; extern long g_bar_phase[]; extern int g_bar_or[];
    const int t = g_cur->lin; const long ph = ++g_bar_phase[t]; const int s = ph & (EMU_RING - 1);
    g_bar_count[s]++; g_bar_or[s] |= pred != 0;
    while (g_bar_count[s] < g_nthreads) fiber_yield();
    ++g_progress;
    g_bar_count[(s + EMU_RING / 2) & (EMU_RING - 1)] = 0; g_bar_or[(s + EMU_RING / 2) & (EMU_RING - 1)] = 0;
    return g_bar_or[s];
}
static inline void __syncthreads() { (void)__syncthreads_or(0); }
// the rendezvous of a wave: every lane of it hands in v -> what the lanes handed in, by lane (to be read before the next rendezvous)
static inline const uint32_t* emu_wave_exchange(uint32_t v)
{
    extern long g_sh_phase[]; extern long g_sh_count[EMU_MAX_THREADS / 64][EMU_RING]; extern uint32_t g_sh_val[EMU_MAX_THREADS / 64][EMU_RING][64];
    const int t = g_cur->lin, w = t >> 6, l = t & 63; const long ph = ++g_sh_phase[t]; const int s = ph & (EMU_RING - 1);
    g_sh_val[w][s][l] = v; g_sh_count[w][s]++;
    while (g_sh_count[w][s] < emu_wave_lanes(w)) fiber_yield();
    ++g_progress;
    g_sh_count[w][(s + EMU_RING / 2) & (EMU_RING - 1)] = 0;
    return g_sh_val[w][s];
}
static inline uint32_t shfl_any(uint32_t v, int src_lane_of_me)
{
    const uint32_t* all = emu_wave_exchange(v);
    return (src_lane_of_me >= 0 && src_lane_of_me < emu_wave_lanes(g_cur->lin >> 6)) ? all[src_lane_of_me] : v;
}
template <class T> static inline T __shfl_up(T v, int o) { int l = g_cur->lin & 63; return (T)shfl_any((uint32_t)v, l - o >= 0 ? l - o : l); }
template <class T> static inline T __shfl_down(T v, int o) { int l = g_cur->lin & 63; return (T)shfl_any((uint32_t)v, l + o < 64 ? l + o : l); }
template <class T> static inline T __shfl_xor(T v, int o) { int l = g_cur->lin & 63; return (T)shfl_any((uint32_t)v, l ^ o); }

// ballot / readfirstlane / readlane: the lanes of a wave that exist (a partial last wave has fewer than 64) all take part, like the
// shuffles; a lane that does not exist votes 0, and reading one is an emulator error
[[noreturn]] void emu_fail(const char* fmt, ...);
static inline unsigned long long emu_ballot(bool pred)
{
    const uint32_t* all = emu_wave_exchange(pred ? 1u : 0u);
    unsigned long long m = 0;
    for (int l = 0, n = emu_wave_lanes(g_cur->lin >> 6); l < n; l++) m |= (unsigned long long)(all[l] & 1u) << l;
    return m;
}
static inline int emu_readlane(int v, int lane)
{
    const uint32_t* all = emu_wave_exchange((uint32_t)v);
    if (lane < 0 || lane >= emu_wave_lanes(g_cur->lin >> 6)) emu_fail("readlane of lane %d, which the wave does not have", lane);
    return (int)all[lane];
}
#define __builtin_amdgcn_ballot_w64 emu_ballot
#define __builtin_amdgcn_readlane emu_readlane
#define __builtin_amdgcn_readfirstlane(v) emu_readlane((v), 0)
// v_mov_b32_dpp as the gfx9 ISA states it, for the controls the emulated sources use: row_shr:1..15 (0x111..0x11F), row_bcast:15
// (0x142: lane 15 of each 16-lane row to all lanes of the next row) and row_bcast:31 (0x143: lane 31 to rows 2 and 3).  A lane
// whose row (row_mask bit lane / 16) or bank (bank_mask bit lane % 16 / 4) is masked off receives `old`; a lane whose source lies
// outside its row, or does not exist, receives `old`, or 0 with bound_ctrl.  Any other control is an emulator error
static inline int emu_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl)
{
    const uint32_t* all = emu_wave_exchange((uint32_t)src);
    const int l = g_cur->lin & 63, row = l >> 4, n = emu_wave_lanes(g_cur->lin >> 6);
    int from;
    if (ctrl >= 0x111 && ctrl <= 0x11F) from = (l & 15) - (ctrl - 0x110) >= 0 ? l - (ctrl - 0x110) : -1;
    else if (ctrl == 0x142) from = row >= 1 ? 16 * row - 1 : -1;
    else if (ctrl == 0x143) from = row >= 2 ? 31 : -1;
    else emu_fail("DPP control 0x%x is not emulated", ctrl);
    if (!((row_mask >> row) & 1) || !((bank_mask >> ((l & 15) >> 2)) & 1)) return old;
    if (from < 0 || from >= n) return bound_ctrl ? 0 : old;
    return (int)all[from];
}
#define __builtin_amdgcn_update_dpp emu_update_dpp
#define V3D_DPP_ROW_SHR(n) (0x110 + (n))   // lane i reads lane i-n of its row
template <int CTRL> static inline uint32_t dpp_mov(uint32_t old, uint32_t src) { return (uint32_t)emu_update_dpp((int)old, (int)src, CTRL, 0xF, 0xF, false); }

// atomics on LDS and global memory alike: uint32_t / unsigned and unsigned long long (uint64_t is unsigned long here)
template <class T, class V> static inline T atomicAdd(T* p, V v) { T o = *p; *p = (T)(o + (T)v); return o; }
template <class T, class V> static inline T atomicOr(T* p, V v) { T o = *p; *p = (T)(o | (T)v); return o; }
template <class T, class V> static inline T atomicMax(T* p, V v) { T o = *p; if ((T)v > o) *p = (T)v; return o; }
template <class T, class V> static inline T atomicMin(T* p, V v) { T o = *p; if ((T)v < o) *p = (T)v; return o; }

// relaxed agent-scope loads and stores: plain accesses (one fiber runs at a time)
#define __HIP_MEMORY_SCOPE_AGENT 4
template <class T> static inline T __hip_atomic_load(const T* p, int, int) { return *p; }
template <class T, class V> static inline void __hip_atomic_store(T* p, V v, int, int) { *p = (T)v; }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }

static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
// the low 24 bits of each operand, sign-extended; the low 32 bits of the product
static inline int __mul24(int a, int b)
{
    const int64_t x = (int64_t)((uint64_t)(uint32_t)a << 40) >> 40, y = (int64_t)((uint64_t)(uint32_t)b << 40) >> 40;
    return (int)(uint32_t)(uint64_t)(x * y);
}
// v_sad_u8: the four byte-wise absolute differences of a and b, added to c
static inline unsigned emu_sad_u8(unsigned a, unsigned b, unsigned c)
{
    for (int i = 0; i < 4; i++) { const int x = (a >> (8 * i)) & 255, y = (b >> (8 * i)) & 255; c += (unsigned)(x > y ? x - y : y - x); }
    return c;
}
#define __builtin_amdgcn_sad_u8 emu_sad_u8
static inline uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31)); }
// two int16 in one word, element-wise: signed min / max, wrapping add, one value in both halves
static inline uint32_t emu_pk(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
static inline int emu_lo16(uint32_t a) { return (int16_t)(uint16_t)(a & 0xFFFFu); }
static inline int emu_hi16(uint32_t a) { return (int16_t)(uint16_t)(a >> 16); }
static inline uint32_t pk_min(uint32_t a, uint32_t b) { return emu_pk(min(emu_lo16(a), emu_lo16(b)), min(emu_hi16(a), emu_hi16(b))); }
static inline uint32_t pk_max(uint32_t a, uint32_t b) { return emu_pk(max(emu_lo16(a), emu_lo16(b)), max(emu_hi16(a), emu_hi16(b))); }
static inline uint32_t pk_add(uint32_t a, uint32_t b) { return emu_pk(emu_lo16(a) + emu_lo16(b), emu_hi16(a) + emu_hi16(b)); }
static inline uint32_t pk_bcast(int v) { return emu_pk(v, v); }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
// single roundings (the build passes -ffp-contract=off, and x86-64 evaluates float expressions in float)
static inline float __fmul_rn(float a, float b) { volatile float r = a * b; return r; }
static inline float __fadd_rn(float a, float b) { volatile float r = a + b; return r; }
static inline float __fsub_rn(float a, float b) { volatile float r = a - b; return r; }
static inline float __fdiv_rn(float a, float b) { volatile float r = a / b; return r; }

// per-frame float min / max in a {min, max} slot of two ordered uints, as in csrc/v3d_common.h
static inline void mm_reset(unsigned* slot) { slot[0] = 0xFFFFFFFFu; slot[1] = 0u; }
static inline void mm_wave_fold(unsigned* slot, unsigned lo, unsigned hi, bool skip_empty = false)
{
    for (int s = 32; s >= 1; s >>= 1) { lo = min(lo, (unsigned)__shfl_xor((int)lo, s)); hi = max(hi, (unsigned)__shfl_xor((int)hi, s)); }
    if ((threadIdx.x & 63) == 0 && !(skip_empty && lo > hi)) { atomicMin(slot, lo); atomicMax(slot + 1, hi); }
}

// 16-byte and 8-byte streaming accesses: counted when off their alignment (then done byte-wise, so that the run goes on), and a
// load is counted when its block lies in a registered input but holds none of its payload (emu_register_payload)
extern int g_misaligned, g_nopayload;
void emu_check_block(const void* p, size_t bytes);
template <class T> static inline T emu_ld(const T* p)
{
    emu_check_block(p, sizeof(T));
    if ((uintptr_t)p % sizeof(T)) { ++g_misaligned; T v; memcpy(&v, (const void*)p, sizeof(T)); return v; }
    return *p;
}
template <class T> static inline void emu_st(T* p, T v)
{
    if ((uintptr_t)p % sizeof(T)) { ++g_misaligned; memcpy((void*)p, &v, sizeof(T)); return; }
    *p = v;
}
static inline uint4 ld_stream(const uint4* p) { return emu_ld(p); }
static inline uint2 ld_stream(const uint2* p) { return emu_ld(p); }
static inline void st_stream(uint4* p, uint4 v) { emu_st(p, v); }
static inline void st_stream(uint2* p, uint2 v) { emu_st(p, v); }

void v3d_set_error(const char* fmt, ...);
static inline int v3d_cdiv(int a, int b) { return (a + b - 1) / b; }
void run_grid(dim3 grid, dim3 block, size_t lds, std::function<void()> body);
#define hipLaunchKernelGGL(k, grid, block, lds, st, ...) run_grid(grid, block, lds, [&]() { k(__VA_ARGS__); })

// what a driver sets before it calls an entry (harness.cpp)
extern "C" {
void emu_configure(int wg_descending, int threads_descending, int lds_poison);
void emu_register_payload(const void* alloc, size_t alloc_bytes, const void* payload, size_t payload_bytes);
int emu_misaligned_loads();
int emu_nopayload_loads();
}
