// v3d_range.hip -- float depth -> per-frame (min, max) -> u16 samples: every entry that reduces a depth range or normalises
// against one (contracts in include/v3d_hip.h; the arithmetic itself is v3d_depth_math.h).
//   v3d_depth_to_u16[_batch]        depth.py:397-406 save_depth_map: a frame against its own min and max
//   v3d_depth_minmax_batch          the same reduction, handed out as floats (the temporal stage's window range starts here)
//   v3d_depth_to_u16_range_batch    the same samples against a (lo, hi) the device supplies per frame
//   v3d_depth_robust_minmax_batch   ("Robust range"; NumPy restatement in tests/range_ref.py): per frame, one
//     read of the depth gives the float min and max and a histogram of the fixed-point disparities d16 = rint(16 D), valid iff >= 1:
//       hist[b] = #{d16 == b} for 1 <= b <= 2046, hist[2047] = #{d16 >= 2047}, n_valid = sum hist
//       k = max(1, ceil(q n_valid / 10000)), hi16 = the smallest b whose cumulative count reaches k
//       hi = mx if n_valid == 0 or hi16 == 2047, else max(hi16 / 16, mn)                 -> (mn, hi) per frame
// Min and max are exact, every sum is an integer and the normalisation is per element, so neither the order of the atomics nor
// the batch or block count can change a bit.  No entry synchronises or allocates.
#include "v3d_common.h"
#include "v3d_wave.h"

#define RR_NB 2048
#define RR_WAVES 4             // waves of a 256-lane workgroup

static int check_frames(int n, size_t elems, size_t stride, size_t min_elems = 1)
{
    if (n < 1 || n > 65535 || elems < min_elems) { v3d_set_error("bad batch %d x %zu", n, elems); return V3D_ERR_ARG; }
    if (n > 1 && stride < elems) { v3d_set_error("frame stride %zu below the frame size %zu", stride, elems); return V3D_ERR_ARG; }
    return V3D_OK;
}
// blocks per frame of a (blocks, n) grid whose block covers px elements per step: about 1024 blocks per launch whatever n is, at
// least `floor` per frame, never more than the frame fills (a 1080p frame is 8100 blocks of 256)
static int frame_blocks(size_t elems, int n, int floor, size_t px = 256)
{
    const size_t want = (elems + px - 1) / px, per = (size_t)(1024 / n > floor ? 1024 / n : floor);
    return (int)(want < per ? want : per);
}

// ---- per-frame min / max: blockIdx.y is the frame, frame f's {min, max} slot is mm[2f], mm[2f + 1] (ordered uints) ----
__global__ void k_mm_init(unsigned* mm, int n)
{
    for (int f = blockIdx.x * 256 + threadIdx.x; f < n; f += gridDim.x * 256) mm_reset(mm + 2 * f);
}
__global__ __launch_bounds__(256) void k_minmax(const float* __restrict__ d, size_t n, size_t stride, unsigned* mm)
{
    d += blockIdx.y * stride; mm += 2 * blockIdx.y;
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned o = v3d_f2ord(d[i]);
        lo = min(lo, o); hi = max(hi, o);
    }
    mm_wave_fold(mm, lo, hi);
}
// a reduced {min, max} slot as floats.  The codec sorts a NaN with the sign bit set below -inf and one with it clear above +inf,
// so a frame that holds any NaN shows it in the slot's min or in its max: then both are NaN, as numpy's min() and max() give
struct mm_pair { float lo, hi; };
__device__ __forceinline__ mm_pair mm_decode(const unsigned* mm)
{
    const float lo = v3d_ord2f(mm[0]), hi = v3d_ord2f(mm[1]);
    const bool nan = lo != lo || hi != hi;
    return { nan ? __builtin_nanf("") : lo, nan ? __builtin_nanf("") : hi };
}
__global__ void k_mm_decode(unsigned* mm, int n)
{
    for (int f = blockIdx.x * 256 + threadIdx.x; f < n; f += gridDim.x * 256) {
        const mm_pair p = mm_decode(mm + 2 * f);
        mm[2 * f] = __float_as_uint(p.lo); mm[2 * f + 1] = __float_as_uint(p.hi);
    }
}
// ENCODED: the frame's (lo, hi) is a {min, max} slot as k_minmax leaves it; else two floats
template <bool ENCODED>
__global__ __launch_bounds__(256) void k_norm_u16(const float* __restrict__ d, size_t n, size_t stride, const unsigned* __restrict__ lohi,
                                                  uint16_t* __restrict__ out)
{
    d += blockIdx.y * stride; lohi += 2 * blockIdx.y; out += blockIdx.y * n;
    const float lo = ENCODED ? v3d_ord2f(lohi[0]) : __uint_as_float(lohi[0]), hi = ENCODED ? v3d_ord2f(lohi[1]) : __uint_as_float(lohi[1]);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = v3d_norm_u16(d[i], lo, hi);
}

static int depth_to_u16(const float* depth, int n, size_t elems, size_t stride, uint16_t* out, float* ws, hipStream_t st)
{
    if (!depth || !out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (check_frames(n, elems, stride, 0) != V3D_OK) return V3D_ERR_ARG;
    if (elems == 0) return V3D_OK;
    unsigned* mm = reinterpret_cast<unsigned*>(ws);
    const int bx = frame_blocks(elems, n, 64);
    hipLaunchKernelGGL(k_mm_init, dim3(v3d_cdiv(n, 256)), dim3(256), 0, st, mm, n);
    hipLaunchKernelGGL(k_minmax, dim3(bx, n), dim3(256), 0, st, depth, elems, stride, mm);
    hipLaunchKernelGGL(k_norm_u16<true>, dim3(bx, n), dim3(256), 0, st, depth, elems, stride, mm, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
extern "C" int v3d_depth_to_u16(const float* depth, size_t n, uint16_t* out, float* ws, void* stream)
{
    return depth_to_u16(depth, 1, n, n, out, ws, (hipStream_t)stream);
}
extern "C" int v3d_depth_to_u16_batch(const float* depth, int n, size_t frame_elems, size_t frame_stride, uint16_t* out,
                                      float* minmax_ws, void* stream)
{
    return depth_to_u16(depth, n, frame_elems, frame_stride, out, minmax_ws, (hipStream_t)stream);
}

extern "C" int v3d_depth_minmax_batch(const float* depth, int T, size_t frame_elems, size_t frame_stride, float* minmax_out,
                                      void* stream)
{
    if (!depth || !minmax_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (check_frames(T, frame_elems, frame_stride) != V3D_OK) return V3D_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    unsigned* mm = reinterpret_cast<unsigned*>(minmax_out);
    hipLaunchKernelGGL(k_mm_init, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, mm, T);
    hipLaunchKernelGGL(k_minmax, dim3(frame_blocks(frame_elems, T, 64), T), dim3(256), 0, st, depth, frame_elems, frame_stride, mm);
    hipLaunchKernelGGL(k_mm_decode, dim3(v3d_cdiv(T, 256)), dim3(256), 0, st, mm, T);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_depth_to_u16_range_batch(const float* depth, int n, size_t frame_elems, size_t frame_stride, const float* lohi,
                                            uint16_t* out, void* stream)
{
    if (!depth || !lohi || !out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (check_frames(n, frame_elems, frame_stride) != V3D_OK) return V3D_ERR_ARG;
    hipLaunchKernelGGL(k_norm_u16<false>, dim3(frame_blocks(frame_elems, n, 64), n), dim3(256), 0, (hipStream_t)stream, depth, frame_elems,
                       frame_stride, reinterpret_cast<const unsigned*>(lohi), out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// ---- the robust range: its own fused kernels (min/max and histogram off one read), one init launch ----
// the histogram bin: 0 = invalid (not counted; NaN and -inf are invalid), the last bin saturates (+inf lands there)
__device__ __forceinline__ int rr_bin(float d)
{
    const int v = v3d_d16_tap(d);
    return v >= RR_NB - 1 ? RR_NB - 1 : v;
}

__global__ void k_rr_init(unsigned* hist, unsigned* mm, int T)
{
    const size_t n = (size_t)T * RR_NB;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) hist[i] = 0u;
    for (int f = blockIdx.x * 256 + threadIdx.x; f < T; f += gridDim.x * 256) mm_reset(mm + 2 * f);
}

// A depth map is piecewise smooth, so the lanes of a wave, and the 4 pixels of a lane, mostly hit the same few bins: same-
// address LDS atomics.  The remedy that won its A/B: a lane merges equal bins among its 4 pixels before it issues,
// at most one atomic per distinct bin.  One sub-histogram per wave on top of it gained nothing and was removed.  Invalid
// pixels (a fifth of a matcher's frame, one single value) issue nothing: they are not in the histogram, n_valid is its sum.
__device__ __forceinline__ void rr_count4(unsigned* h, const float4 v)
{
    const int b0 = rr_bin(v.x), b1 = rr_bin(v.y), b2 = rr_bin(v.z), b3 = rr_bin(v.w);
    if (b0) atomicAdd(h + b0, 1u + (b1 == b0) + (b2 == b0) + (b3 == b0));
    if (b1 && b1 != b0) atomicAdd(h + b1, 1u + (b2 == b1) + (b3 == b1));
    if (b2 && b2 != b0 && b2 != b1) atomicAdd(h + b2, 1u + (b3 == b2));
    if (b3 && b3 != b0 && b3 != b1 && b3 != b2) atomicAdd(h + b3, 1u);
}
__device__ __forceinline__ void rr_minmax4(unsigned& lo, unsigned& hi, const float4 v)
{
    const unsigned a = v3d_f2ord(v.x), b = v3d_f2ord(v.y), c = v3d_f2ord(v.z), d = v3d_f2ord(v.w);
    lo = min(min(lo, a), min(b, min(c, d)));
    hi = max(max(hi, a), max(b, max(c, d)));
}

// grid (blocks, T).  VEC: the frame's base address and stride allow 16-byte loads, a lane owns 4 adjacent pixels and four loads
// are in flight per step; the n & 3 last pixels, and everything in the other instantiation (unaligned views, odd strides), go
// element by element.
template <bool VEC>
__global__ __launch_bounds__(256) void k_rr_hist(const float* __restrict__ d, size_t n, size_t stride, unsigned* __restrict__ hist,
                                                 unsigned* __restrict__ mm)
{
    __shared__ unsigned h[RR_NB];
    d += blockIdx.y * stride; hist += (size_t)blockIdx.y * RR_NB; mm += 2 * blockIdx.y;
    for (int i = threadIdx.x; i < RR_NB; i += 256) h[i] = 0u;
    __syncthreads();
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    const size_t step = (size_t)gridDim.x * 256;
    const size_t nvec = VEC ? n / 4 : 0;
    if (VEC) {
        const float4* d4 = reinterpret_cast<const float4*>(d);
        size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        for (; i + 3 * step < nvec; i += 4 * step) {                       // four 16-byte loads in flight per lane
            const float4 a = d4[i], b = d4[i + step], c = d4[i + 2 * step], e = d4[i + 3 * step];
            rr_minmax4(lo, hi, a); rr_minmax4(lo, hi, b); rr_minmax4(lo, hi, c); rr_minmax4(lo, hi, e);
            rr_count4(h, a); rr_count4(h, b); rr_count4(h, c); rr_count4(h, e);
        }
        for (; i < nvec; i += step) {
            const float4 a = d4[i];
            rr_minmax4(lo, hi, a);
            rr_count4(h, a);
        }
    }
    for (size_t i = nvec * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        const float v = d[i];
        const unsigned o = v3d_f2ord(v);
        lo = min(lo, o); hi = max(hi, o);
        const int b = rr_bin(v);
        if (b) atomicAdd(h + b, 1u);
    }
    mm_wave_fold(mm, lo, hi);
    __syncthreads();
    for (int b = threadIdx.x; b < RR_NB; b += 256) {
        const unsigned c = h[b];
        if (c) atomicAdd(hist + b, c);
    }
}

// one workgroup per frame: a lane owns 8 adjacent bins, block scan of the lanes' sums, the lane whose run crosses k walks its 8
__global__ __launch_bounds__(256) void k_rr_select(const unsigned* __restrict__ hist, const unsigned* __restrict__ mm, int q,
                                                   float* __restrict__ out)
{
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint4* h4 = reinterpret_cast<const uint4*>(hist + (size_t)t * RR_NB) + 2 * tid;
    const uint4 a = h4[0], b = h4[1];
    const unsigned c[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    const unsigned own = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
    __shared__ unsigned part[RR_WAVES];
    const excl_total sc = block_excl_add_u32<RR_WAVES>(own, lane, wave, part);
    const unsigned before = sc.excl, n_valid = sc.total;
    const mm_pair p = mm_decode(mm + 2 * t);                               // a frame with a NaN: (NaN, NaN), whatever the histogram holds
    const float mn = p.lo, mx = p.hi;
    if (tid == 0) { out[2 * t] = mn; if (n_valid == 0) out[2 * t + 1] = mx; }
    if (n_valid == 0) return;
    const unsigned long long kq = ((unsigned long long)q * n_valid + 9999ull) / 10000ull;
    const unsigned k = kq < 1ull ? 1u : (unsigned)kq;                      // q <= 10000: k <= n_valid
    if (before < k && k <= before + own) {                                 // exactly one lane
        unsigned run = before;
        int hi16 = -1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            run += c[j];
            if (hi16 < 0 && run >= k) hi16 = 8 * tid + j;
        }
        const float v = (float)hi16 * 0.0625f;
        out[2 * t + 1] = hi16 == RR_NB - 1 ? mx : (v > mn ? v : mn);
    }
}

extern "C" size_t v3d_depth_robust_minmax_ws_bytes(int T)
{
    return T < 1 ? 0 : (size_t)T * (RR_NB + 2) * sizeof(unsigned);
}

extern "C" int v3d_depth_robust_minmax_batch(const float* depth, int T, size_t frame_elems, size_t frame_stride, int q, void* ws,
                                             float* minmax_out, void* stream)
{
    if (!depth || !ws || !minmax_out) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (check_frames(T, frame_elems, frame_stride) != V3D_OK) return V3D_ERR_ARG;
    if (q < 5000 || q > 10000) { v3d_set_error("range quantile %d outside [5000, 10000]", q); return V3D_ERR_ARG; }
    if (((uintptr_t)ws & 15) != 0) { v3d_set_error("workspace must be 16-byte aligned"); return V3D_ERR_ARG; }
    if (frame_elems > 0xFFFFFFFFull) { v3d_set_error("frame of %zu elements: the bins are 32-bit counters", frame_elems); return V3D_ERR_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream;
    unsigned* hist = reinterpret_cast<unsigned*>(ws);
    unsigned* mm = hist + (size_t)T * RR_NB;
    const bool vec = ((uintptr_t)depth & 15) == 0 && (T == 1 || (frame_stride & 3) == 0);
    // one step of a block covers 4096 px.  All workgroups of a 34-frame pass are resident at once (4 per CU): a grid a little
    // larger than the chip holds runs a second, nearly empty round that costs as much as the first
    const int bx = frame_blocks(frame_elems, T, 8, 4096);
    hipLaunchKernelGGL(k_rr_init, dim3(T < 128 ? 8 * T : 1024), dim3(256), 0, st, hist, mm, T);
    if (vec) hipLaunchKernelGGL(k_rr_hist<true>, dim3(bx, T), dim3(256), 0, st, depth, frame_elems, frame_stride, hist, mm);
    else hipLaunchKernelGGL(k_rr_hist<false>, dim3(bx, T), dim3(256), 0, st, depth, frame_elems, frame_stride, hist, mm);
    hipLaunchKernelGGL(k_rr_select, dim3(T), dim3(256), 0, st, hist, mm, q, minmax_out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
