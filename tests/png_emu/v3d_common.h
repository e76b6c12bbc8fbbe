// Host stand-in for csrc/v3d_common.h, for tests/test_png_emulated.py only: csrc/v3d_png.hip is compiled as plain C++ against it.
// The 256 threads of a workgroup are fibers (ucontext) that a round-robin scheduler runs until each waits at a rendezvous:
// __syncthreads() for the workgroup, a wave shuffle for its 64 lanes.  Workgroups run one after another; LDS is one poisoned
// static buffer; atomics are plain read-modify-writes (one fiber runs at a time).  Nothing here is used by the product.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <ucontext.h>
#include <algorithm>
#include <vector>
#include <functional>
#include "v3d_hip.h"
using std::min; using std::max;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
struct uint2 { uint32_t x, y; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static inline uint4 make_uint4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return uint4{a, b, c, d}; }
static inline uint2 make_uint2(uint32_t a, uint32_t b) { return uint2{a, b}; }
typedef void* hipStream_t;
struct Fiber { ucontext_t ctx; dim3 tid; bool done; std::vector<char> stack; };
extern Fiber* g_cur; extern ucontext_t g_sched; extern dim3 blockIdx, gridDim;
#define threadIdx (g_cur->tid)
void fiber_yield();
extern int g_nthreads;
static inline void __syncthreads()
{
    extern long g_bar_count[]; extern long g_bar_phase[];
    // rendezvous number ph of this thread; its counter slot is cleared again half a ring later
    int t = g_cur->tid.x; long ph = ++g_bar_phase[t];
    g_bar_count[ph & 1023]++;
    while (g_bar_count[ph & 1023] < g_nthreads) fiber_yield();
    g_bar_count[(ph + 512) & 1023] = 0;
}
static inline uint32_t shfl_any(uint32_t v, int src_lane_of_me)
{
    extern long g_sh_phase[]; extern long g_sh_count[4][1024]; extern uint32_t g_sh_val[4][1024][64];
    int t = g_cur->tid.x, w = t >> 6, l = t & 63; long ph = ++g_sh_phase[t]; int s = ph & 1023;
    g_sh_val[w][s][l] = v; g_sh_count[w][s]++;
    while (g_sh_count[w][s] < 64) fiber_yield();
    g_sh_count[w][(s + 512) & 1023] = 0;
    return (src_lane_of_me >= 0 && src_lane_of_me < 64) ? g_sh_val[w][s][src_lane_of_me] : v;
}
template <class T> static inline T __shfl_up(T v, int o) { int l = g_cur->tid.x & 63; return (T)shfl_any((uint32_t)v, l - o >= 0 ? l - o : l); }
template <class T> static inline T __shfl_down(T v, int o) { int l = g_cur->tid.x & 63; return (T)shfl_any((uint32_t)v, l + o < 64 ? l + o : l); }
template <class T> static inline T __shfl_xor(T v, int o) { int l = g_cur->tid.x & 63; return (T)shfl_any((uint32_t)v, l ^ o); }
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { uint32_t o = *p; *p += v; return o; }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { uint32_t o = *p; *p |= v; return o; }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
extern int g_misaligned;
static inline uint4 ld_stream(const uint4* p) { if ((uintptr_t)p & 15) ++g_misaligned; return *p; }
static inline uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31)); }
void v3d_set_error(const char* fmt, ...);
#define V3D_LAUNCH_CHECK() do {} while (0)
static inline int v3d_cdiv(int a, int b) { return (a + b - 1) / b; }
void run_grid(dim3 grid, dim3 block, size_t lds, std::function<void()> body);
#define hipLaunchKernelGGL(k, grid, block, lds, st, ...) run_grid(grid, block, lds, [&]() { k(__VA_ARGS__); })
