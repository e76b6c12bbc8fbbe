// Toy kernels of tests/test_emu_selftest.py, written like the product's (against tests/emu/v3d_common.h).  One workgroup of 256
// threads (toy_workgroup_order: four); in holds 256 words (toy_global_overread: 256 bytes, toy_misaligned_load: 4096 + 16 bytes),
// out 256 words (toy_workgroup_order: 4).  bad = 0 is the correct twin.
#include "v3d_common.h"
#include "toys.h"

// writes one element past its dynamic LDS (and reads it back: the output is right)
__global__ void k_lds_overrun(const uint32_t* in, uint32_t* out, int bad)
{
    uint32_t* s = reinterpret_cast<uint32_t*>(g_lds);
    const int t = threadIdx.x;
    s[t + bad] = in[t];
    __syncthreads();
    out[t] = s[t + bad];
}
// reads one byte past its input and does not use it
__global__ void k_global_overread(const uint8_t* in, uint32_t* out, int bad)
{
    const int t = threadIdx.x;
    (void)*reinterpret_cast<const volatile uint8_t*>(in + t + bad);
    out[t] = in[t];
}
// a 16-byte load one byte off its alignment: bad = 1 through ld_stream, bad = 2 as a plain dereference
__global__ void k_misaligned_load(const uint8_t* in, uint32_t* out, int bad)
{
    const int t = threadIdx.x;
    const uint4* p = reinterpret_cast<const uint4*>(in + 16 * t + (bad ? 1 : 0));
    const uint4 v = bad == 2 ? *p : ld_stream(p);
    out[t] = v.x ^ v.y ^ v.z ^ v.w;
}
// reads LDS that no thread wrote
__global__ void k_lds_unwritten(const uint32_t* in, uint32_t* out, int bad)
{
    uint32_t* s = reinterpret_cast<uint32_t*>(g_lds);
    const int t = threadIdx.x;
    if (!bad) s[t] = 0;
    __syncthreads();
    out[t] = in[t] + s[255 - t];
}
// lacks the barrier between a write and the read by another wave
__global__ void k_missing_barrier(const uint32_t* in, uint32_t* out, int bad)
{
    uint32_t* s = reinterpret_cast<uint32_t*>(g_lds);
    const int t = threadIdx.x;
    s[t] = in[t];
    if (!bad) __syncthreads();
    out[t] = s[(t + 64) & 255];
}
// a result that depends on the order in which the workgroups ran
__global__ void k_workgroup_order(uint32_t* counter, uint32_t* out, int bad)
{
    if (threadIdx.x == 0) {
        const uint32_t ticket = atomicAdd(counter, 1u);
        out[blockIdx.x] = bad ? ticket : blockIdx.x;
    }
}

extern "C" int toy_lds_overrun(const uint32_t* in, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_lds_overrun, dim3(1), dim3(256), 1024, (hipStream_t)stream, in, out, bad);
    return 0;
}
extern "C" int toy_global_overread(const uint8_t* in, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_global_overread, dim3(1), dim3(256), 0, (hipStream_t)stream, in, out, bad);
    return 0;
}
extern "C" int toy_misaligned_load(const uint8_t* in, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_misaligned_load, dim3(1), dim3(256), 0, (hipStream_t)stream, in, out, bad);
    return 0;
}
extern "C" int toy_lds_unwritten(const uint32_t* in, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_lds_unwritten, dim3(1), dim3(256), 1024, (hipStream_t)stream, in, out, bad);
    return 0;
}
extern "C" int toy_missing_barrier(const uint32_t* in, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_missing_barrier, dim3(1), dim3(256), 1024, (hipStream_t)stream, in, out, bad);
    return 0;
}
extern "C" int toy_workgroup_order(uint32_t* counter, uint32_t* out, int bad, void* stream)
{
    hipLaunchKernelGGL(k_workgroup_order, dim3(4), dim3(256), 0, (hipStream_t)stream, counter, out, bad);
    return 0;
}
// every thread counts itself: out[0] = the number of threads that ran
__global__ void k_count(uint32_t* out) { atomicAdd(out, 1u); }
extern "C" int toy_launch(uint32_t* out, int lds_bytes, int threads, void* stream)
{
    hipLaunchKernelGGL(k_count, dim3(1), dim3(threads), lds_bytes, (hipStream_t)stream, out);
    return 0;
}

// ---- the cross-lane shims, each with a known answer (test_emu_selftest.py restates them in NumPy) ----
// row_shr:n of in, `old` = ~in: lanes whose source lies left of their 16-lane row keep old
template <int N> static inline uint32_t shr_of(uint32_t v) { return dpp_mov<V3D_DPP_ROW_SHR(N)>(~v, v); }
__global__ void k_row_shr(const uint32_t* in, uint32_t* out, int n)
{
    const int t = threadIdx.x; const uint32_t v = in[t];
    out[t] = n == 1 ? shr_of<1>(v) : n == 2 ? shr_of<2>(v) : n == 4 ? shr_of<4>(v) : shr_of<8>(v);
}
// which = 15: row_bcast:15 with row_mask 0xA; 31: row_bcast:31 with row_mask 0xC; 150 / 310: the same with row_mask 0xF (row 0, and
// rows 0 and 1, have no source); anything else goes to the builtin as the control (an emulator error)
__global__ void k_row_bcast(const uint32_t* in, uint32_t* out, int which)
{
    const int t = threadIdx.x; const int v = (int)in[t];
    out[t] = which == 15 ? (uint32_t)__builtin_amdgcn_update_dpp(~v, v, 0x142, 0xA, 0xF, false)
           : which == 31 ? (uint32_t)__builtin_amdgcn_update_dpp(~v, v, 0x143, 0xC, 0xF, false)
           : which == 150 ? (uint32_t)__builtin_amdgcn_update_dpp(~v, v, 0x142, 0xF, 0xF, false)
           : which == 310 ? (uint32_t)__builtin_amdgcn_update_dpp(~v, v, 0x143, 0xF, 0xF, false)
           : (uint32_t)__builtin_amdgcn_update_dpp(~v, v, which, 0xF, 0xF, false);
}
// the inclusive max-scan over a wave's 64 lanes, built like the product's from four shifts and two broadcasts; bad = 1 leaves out the
// row_bcast:31 step: rows 2 and 3 then miss what rows 0 and 1 hold
__global__ void k_wave_scan(const uint32_t* in, uint32_t* out, int bad)
{
    uint32_t v = in[threadIdx.x];
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(1)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(2)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(4)>(0u, v));
    v = max(v, dpp_mov<V3D_DPP_ROW_SHR(8)>(0u, v));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));
    if (!bad) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false));
    out[threadIdx.x] = v;
}
// the ballot of bit 0 of in, as two words per thread; launched with `threads` threads (a partial last wave)
__global__ void k_ballot(const uint32_t* in, uint32_t* out)
{
    const int t = threadIdx.x;
    const unsigned long long m = __builtin_amdgcn_ballot_w64((in[t] & 1u) != 0u);
    out[2 * t] = (uint32_t)m; out[2 * t + 1] = (uint32_t)(m >> 32);
}
// lane 63's and the first lane's value; lane = 64 reads a lane no wave has
__global__ void k_readlane(const uint32_t* in, uint32_t* out, int lane)
{
    const int t = threadIdx.x;
    out[2 * t] = (uint32_t)__builtin_amdgcn_readlane((int)in[t], lane); out[2 * t + 1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)in[t]);
}
// waves `live` .. 3 return as a whole before any rendezvous; the others go on through every kind of it
__global__ void k_wave_exit(const uint32_t* in, uint32_t* out, int live)
{
    const int t = threadIdx.x;
    if ((t >> 6) >= live) return;                              // wave-uniform
    const uint32_t a = (uint32_t)__shfl_up((int)in[t], 1);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)in[t], 63);
    const unsigned long long m = __builtin_amdgcn_ballot_w64((in[t] & 1u) != 0u);
    out[t] = a ^ b ^ (uint32_t)__popcll(m) ^ dpp_mov<V3D_DPP_ROW_SHR(1)>(0u, in[t]);
}
#define TOY(name, kernel, threads) \
    extern "C" int name(const uint32_t* in, uint32_t* out, int arg, void* stream) \
    { hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), 0, (hipStream_t)stream, in, out, arg); return 0; }
TOY(toy_row_shr, k_row_shr, 256)
TOY(toy_row_bcast, k_row_bcast, 256)
TOY(toy_wave_scan, k_wave_scan, 256)
TOY(toy_readlane, k_readlane, 256)
TOY(toy_wave_exit, k_wave_exit, 256)
extern "C" int toy_ballot(const uint32_t* in, uint32_t* out, int threads, void* stream)
{
    hipLaunchKernelGGL(k_ballot, dim3(1), dim3(threads), 0, (hipStream_t)stream, in, out);
    return 0;
}
