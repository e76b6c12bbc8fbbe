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
