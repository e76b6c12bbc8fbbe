// v3d_align.hip -- audio alignment (utils.py:137-165 of the reference: find_audio_offset): normalise both tracks,
// cross-correlate them with a complex float32 FFT, and pick the peak lag by direct f64 sums.
//
//   1. f64 reductions: mean, population std, then an = (a - mean) / (std + 1e-10) rounded to float32, E = sum an^2.
//   2. pack z[n] = s1 a1n[n] + i s2 a2n[n], zero-padded to N = 2^m (N >= n1 + n2 - 1, N >= 2^10, m <= 26).  s1, s2 are
//      powers of two that bring both tracks to a norm near 1: the float32 error of the two-for-one FFT is of the order
//      eps |z|^2, so unequal norms would put the larger track's error onto the smaller one's correlation.  The norm of
//      an is sqrt(n) std / (std + 1e-10): a track with std far below 1e-10 is as far below sqrt(n).
//   3. forward FFT of z in 1 to 3 in-place passes through HBM (see FftPlan): each pass runs LDS-resident radix-4/2
//      sub-FFTs of R = 2^d points over a tile whose global rows hold 16 consecutive complex values (128 bytes), with the
//      inter-pass twiddle fused into the pass.  The spectrum ends in digit-reversed order (storage position perm(k)).
//   4. one kernel separates the two real spectra, A = (Z[k] + conj Z[N-k]) / 2, B = (Z[k] - conj Z[N-k]) / 2i, and
//      writes conj(A) B / (s1 s2 N) in place (a thread owns the pair k, N-k).
//   5. inverse FFT (the forward passes transposed, in reverse order: digit-reversed in, natural order out).  The real
//      part is the circular correlation c[L mod N] = sum_n a2n[n + L] a1n[n].
//   6. peak: per-block maxima of |c| over the valid lags, the TOPK largest, each with its +-NB neighbours, are
//      re-evaluated by direct f64 sums over their overlap; the largest |c| wins.  A maximum that is unique among the
//      valid lags is found; of exactly tied lags the smallest NOMINATED one is returned, and which of them a block
//      nominates (one lag per block, by the float32 value) depends on rounding.
// Twiddles are computed in f64 (sincospi) and rounded to float32 into the caller's workspace by every call.  Every
// reduction has a fixed order: a call's result does not depend on scheduling.
#include "v3d_common.h"
#include <math.h>

namespace {

constexpr int XC_MIN_LOG = 10, XC_MAX_LOG = 26;
constexpr int TW_LOG = 12;                        // in-LDS twiddles: table of W_4096^j
constexpr int RED_BLOCKS = 512, RED_THREADS = 256;
constexpr int PEAK_SPAN = 4096;                   // lag indices per block maximum
constexpr int TOPK = 16, NB = 2, GROUP = 2 * NB + 1, NCAND = TOPK * GROUP;
constexpr int DIRECT_CHUNK = 32768;               // samples of a1n per block of the direct sums

// N = 2^m as 1 to 3 passes of 2^d[i] points (pass 0 has the largest stride).  m <= 12: one launch of a 2^m-point FFT.
// Otherwise ceil(m / 9) passes of near-equal digits (6..9 bits): 2^24 = 256 x 256 x 256, 2^26 = 512 x 512 x 256.
struct FftPlan {
    int m, passes, d[3];
};

FftPlan make_plan(int m)
{
    FftPlan p{};
    p.m = m;
    if (m <= 12) { p.passes = 1; p.d[0] = m; return p; }
    p.passes = (m + 8) / 9;
    for (int i = 0; i < p.passes; ++i) p.d[i] = m / p.passes + (i < m % p.passes ? 1 : 0);
    return p;
}

struct Layout {
    FftPlan plan;
    size_t N, nbm, nchunk;
    size_t z, an1, an2, tw, twlo, twhi, part, stats, bmax, bidx, cand, dpart, total;
};

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// false: sizes out of range (the caller reports which)
bool make_layout(int n1, int n2, Layout& L)
{
    if (n1 < 1 || n2 < 1) return false;
    const long long need = (long long)n1 + n2 - 1;
    int m = XC_MIN_LOG;
    while (m <= XC_MAX_LOG && (1ll << m) < need) ++m;
    if (m > XC_MAX_LOG) return false;
    L.plan = make_plan(m);
    L.N = (size_t)1 << m;
    L.nbm = (L.N + PEAK_SPAN - 1) / PEAK_SPAN;
    L.nchunk = ((size_t)n1 + DIRECT_CHUNK - 1) / DIRECT_CHUNK;
    const int s = (m + 1) / 2;
    size_t o = 0;
    L.z = o;     o = align_up(o + L.N * 8);
    L.an1 = o;   o = align_up(o + (size_t)n1 * 4);
    L.an2 = o;   o = align_up(o + (size_t)n2 * 4);
    L.tw = o;    o = align_up(o + ((size_t)1 << TW_LOG) * 8);
    L.twlo = o;  o = align_up(o + ((size_t)1 << s) * 8);
    L.twhi = o;  o = align_up(o + ((size_t)1 << (m - s)) * 8);
    L.part = o;  o = align_up(o + 2 * RED_BLOCKS * 8);
    L.stats = o; o = align_up(o + 8 * 8);
    L.bmax = o;  o = align_up(o + L.nbm * 4);
    L.bidx = o;  o = align_up(o + L.nbm * 4);
    L.cand = o;  o = align_up(o + TOPK * 4);
    L.dpart = o; o = align_up(o + (size_t)NCAND * L.nchunk * 8);
    L.total = o;
    return true;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }

// W_N^e = lo[e mod 2^s] * hi[e >> s]
__device__ __forceinline__ float2 tw_n(const float2* __restrict__ lo, const float2* __restrict__ hi, uint32_t e, int s)
{
    return cmul(lo[e & ((1u << s) - 1)], hi[e >> s]);
}

// tables: W_4096^j (j < 4096), W_N^j (j < 2^s), W_N^(j 2^s) (j < 2^(m-s)); W_M^j = exp(-2 pi i j / M) in f64, then float32
__global__ __launch_bounds__(256) void k_xc_twiddles(float2* __restrict__ tw, float2* __restrict__ lo, float2* __restrict__ hi, int m, int s)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n0 = 1 << TW_LOG, n1 = 1 << s, n2 = 1 << (m - s);
    double x;                                   // the angle as a multiple of pi: exact (j / M is a dyadic fraction)
    float2* dst;
    if (i < n0) { x = -2.0 * i / n0; dst = tw + i; }
    else if (i < n0 + n1) { x = -2.0 * (i - n0) / (double)(1ll << m); dst = lo + (i - n0); }
    else if (i < n0 + n1 + n2) { x = -2.0 * ((double)(i - n0 - n1) * n1) / (double)(1ll << m); dst = hi + (i - n0 - n1); }
    else return;
    double sn, cs;
    sincospi(x, &sn, &cs);
    *dst = make_float2((float)cs, (float)sn);
}

__device__ double block_sum(double v, double* sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int k = RED_THREADS / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// stats[t*4 + 0..3] = mean, std, E, norm of the packed track t (before its power-of-two scale)
enum { RED_SUM = 0, RED_VAR = 1, RED_NORM = 2, RED_RAW = 3, RED_SQ = 4 };

// 2^-ilogb(norm): exact in float32, brings the track's norm into [1, 2)
__device__ __forceinline__ double pack_scale(double norm) { return norm > 0.0 ? ldexp(1.0, -ilogb(norm)) : 1.0; }

// RED_SUM / RED_VAR / RED_SQ: partial sums of a, (a - mean)^2, a^2 of track blockIdx.y.  RED_NORM: an = (a - mean) /
// (std + 1e-10) -> an1 / an2 and z = s1 an1 + i s2 an2 over [0, N), partial sums of an^2 of both tracks.  RED_RAW:
// z = s1 a1 + i s2 a2, no sums.
template <int MODE>
__global__ __launch_bounds__(RED_THREADS) void k_xc_reduce(const float* __restrict__ a1, int n1, const float* __restrict__ a2, int n2,
                                                           float* __restrict__ an1, float* __restrict__ an2, float2* __restrict__ z,
                                                           size_t N, const double* __restrict__ stats, double* __restrict__ part)
{
    __shared__ double sh[RED_THREADS];
    const size_t stride = (size_t)RED_BLOCKS * RED_THREADS;
    const size_t i0 = (size_t)blockIdx.x * RED_THREADS + threadIdx.x;
    if (MODE == RED_SUM || MODE == RED_VAR || MODE == RED_SQ) {
        const int t = blockIdx.y;
        const float* a = t ? a2 : a1;
        const size_t n = (size_t)(t ? n2 : n1);
        const double mean = MODE == RED_VAR ? stats[t * 4] : 0.0;
        double acc = 0.0;
        for (size_t i = i0; i < n; i += stride) {
            const double v = (double)a[i] - mean;
            acc += MODE == RED_SUM ? v : v * v;
        }
        acc = block_sum(acc, sh);
        if (threadIdx.x == 0) part[t * RED_BLOCKS + blockIdx.x] = acc;
    } else {
        const double m1 = MODE == RED_NORM ? stats[0] : 0.0, d1 = MODE == RED_NORM ? stats[1] + 1e-10 : 1.0;
        const double m2 = MODE == RED_NORM ? stats[4] : 0.0, d2 = MODE == RED_NORM ? stats[5] + 1e-10 : 1.0;
        const float s1 = (float)pack_scale(stats[3]), s2 = (float)pack_scale(stats[7]);
        double e1 = 0.0, e2 = 0.0;
        for (size_t i = i0; i < N; i += stride) {
            float v1 = 0.f, v2 = 0.f;
            if (i < (size_t)n1) {
                v1 = MODE == RED_NORM ? (float)(((double)a1[i] - m1) / d1) : a1[i];
                if (MODE == RED_NORM) { an1[i] = v1; e1 += (double)v1 * v1; }
            }
            if (i < (size_t)n2) {
                v2 = MODE == RED_NORM ? (float)(((double)a2[i] - m2) / d2) : a2[i];
                if (MODE == RED_NORM) { an2[i] = v2; e2 += (double)v2 * v2; }
            }
            z[i] = make_float2(v1 * s1, v2 * s2);
        }
        if (MODE == RED_NORM) {
            e1 = block_sum(e1, sh);
            e2 = block_sum(e2, sh);
            if (threadIdx.x == 0) { part[blockIdx.x] = e1; part[RED_BLOCKS + blockIdx.x] = e2; }
        }
    }
}

// one workgroup folds the RED_BLOCKS partials of both tracks in a fixed order into stats
template <int MODE>
__global__ __launch_bounds__(RED_THREADS) void k_xc_finish(const double* __restrict__ part, int n1, int n2, double* __restrict__ stats)
{
    __shared__ double sh[RED_THREADS];
    for (int t = 0; t < 2; ++t) {
        double v = 0.0;
        for (int i = threadIdx.x; i < RED_BLOCKS; i += RED_THREADS) v += part[t * RED_BLOCKS + i];
        const double s = block_sum(v, sh);
        if (threadIdx.x == 0) {
            const double n = t ? n2 : n1;
            if (MODE == RED_SUM) stats[t * 4] = s / n;
            else if (MODE == RED_VAR) {
                // |an| = sqrt(n) std / (std + 1e-10): sqrt(n) for ordinary audio, far below it for a track quieter than 1e-10
                const double sd = sqrt(s / n);
                stats[t * 4 + 1] = sd;
                stats[t * 4 + 3] = sqrt(n) * (sd / (sd + 1e-10));
            }
            else if (MODE == RED_SQ) stats[t * 4 + 3] = sqrt(s);
            else stats[t * 4 + 2] = s;
        }
    }
}

// One pass of the FFT over z viewed as [A][R][B] (R = 2^LOG_R), in place.  Forward: y[a][k][b] = W_N^(k b P) sum_r
// x[a][r][b] W_R^(r k), with P = N / (R B) (the four-step twiddle of this digit, fused into the store).  Inverse (the
// transposed pass): conj twiddle on the load, then the conjugate DFT.  COLS (B >= 16): a workgroup takes C = 16
// neighbouring columns b of one a, so each global row it touches is 128 contiguous bytes.  !COLS (B = 1, the last
// digit): a workgroup takes C contiguous transforms.  LDS holds the tile as [r][c] with a row stride of C + 1 complex
// values; the sub-FFT is in-place decimation in frequency (radix-4 steps, one radix-2 step for an odd LOG_R), so
// frequency k sits in LDS row bitrev(k).
template <int LOG_R, int C, bool COLS, bool INV>
__global__ __launch_bounds__(256) void k_xc_fft(float2* __restrict__ z, int logB, int logP, const float2* __restrict__ tw,
                                               const float2* __restrict__ twlo, const float2* __restrict__ twhi, int s)
{
    constexpr int R = 1 << LOG_R, S = C == 1 ? 1 : C + 1;
    constexpr int NPAIR = R * C / 512;               // float4 (two complex values) per thread
    constexpr int NBF = R * C / 1024;                // radix-4 butterflies per thread and step
    static_assert(R * C >= 1024 && (R * C) % 1024 == 0, "tile");
    static_assert(!COLS || C == 16, "column tile");
    __shared__ float2 lds[R * S];
    const int tid = threadIdx.x;
    size_t base;
    int b0 = 0;
    if (COLS) {
        const size_t nbc = ((size_t)1 << logB) / C;
        const size_t a = blockIdx.x / nbc;
        b0 = (int)(blockIdx.x % nbc) * C;
        base = ((a * R) << logB) + b0;
    } else {
        base = (size_t)blockIdx.x * R * C;
    }

    float4 v[NPAIR];
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        const int pi = tid + 256 * i;
        size_t g;
        if (COLS) g = base + ((size_t)(pi / (C / 2)) << logB) + 2 * (pi % (C / 2));
        else g = base + (size_t)(pi / (R / 2)) * R + 2 * (pi % (R / 2));
        v[i] = *reinterpret_cast<const float4*>(z + g);
    }
#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        const int pi = tid + 256 * i;
        float2 x0 = make_float2(v[i].x, v[i].y), x1 = make_float2(v[i].z, v[i].w);
        if (COLS) {
            const int r = pi / (C / 2), c = 2 * (pi % (C / 2));
            if (INV) {
                const uint32_t e = ((uint32_t)r * (uint32_t)(b0 + c)) << logP;
                x0 = cmul(x0, cconj(tw_n(twlo, twhi, e, s)));
                x1 = cmul(x1, cconj(tw_n(twlo, twhi, e + ((uint32_t)r << logP), s)));
            }
            lds[r * S + c] = x0;
            lds[r * S + c + 1] = x1;
        } else {
            const int c = pi / (R / 2), r = 2 * (pi % (R / 2));
            lds[r * S + c] = x0;
            lds[(r + 1) * S + c] = x1;
        }
    }
    __syncthreads();

    // radix-4 DIF steps: block 4q, elements j + {0,1,2,3} q; == the radix-2 steps of spans 2q and q
#pragma unroll
    for (int lq = LOG_R - 2; lq >= 0; lq -= 2) {
        const int q = 1 << lq;
#pragma unroll
        for (int i = 0; i < NBF; ++i) {
            const int beta = tid + 256 * i;
            const int c = beta % C, rest = beta / C;
            const int j = rest & (q - 1), r0 = ((rest >> lq) << (lq + 2)) + j;
            const float2 x0 = lds[r0 * S + c], x1 = lds[(r0 + q) * S + c];
            const float2 x2 = lds[(r0 + 2 * q) * S + c], x3 = lds[(r0 + 3 * q) * S + c];
            const int t1 = j << (TW_LOG - lq - 2);
            float2 w1 = tw[t1], w2 = tw[2 * t1];
            if (INV) { w1 = cconj(w1); w2 = cconj(w2); }
            const float2 a0 = cadd(x0, x2), a1 = cadd(x1, x3);
            const float2 a2 = cmul(csub(x0, x2), w1);
            float2 d3 = csub(x1, x3);
            d3 = INV ? make_float2(-d3.y, d3.x) : make_float2(d3.y, -d3.x);        // * W_4^(-+1) = +-i
            const float2 a3 = cmul(d3, w1);
            lds[r0 * S + c] = cadd(a0, a1);
            lds[(r0 + q) * S + c] = cmul(csub(a0, a1), w2);
            lds[(r0 + 2 * q) * S + c] = cadd(a2, a3);
            lds[(r0 + 3 * q) * S + c] = cmul(csub(a2, a3), w2);
        }
        __syncthreads();
    }
    if (LOG_R & 1) {                                 // last radix-2 step, span 1 (twiddle 1)
#pragma unroll
        for (int i = 0; i < 2 * NBF; ++i) {
            const int beta = tid + 256 * i;
            const int c = beta % C, r0 = 2 * (beta / C);
            const float2 x0 = lds[r0 * S + c], x1 = lds[(r0 + 1) * S + c];
            lds[r0 * S + c] = cadd(x0, x1);
            lds[(r0 + 1) * S + c] = csub(x0, x1);
        }
        __syncthreads();
    }

#pragma unroll
    for (int i = 0; i < NPAIR; ++i) {
        const int pi = tid + 256 * i;
        size_t g;
        float2 y0, y1;
        if (COLS) {
            const int k = pi / (C / 2), c = 2 * (pi % (C / 2));
            const int kr = (int)(__builtin_bitreverse32((uint32_t)k) >> (32 - LOG_R));
            y0 = lds[kr * S + c];
            y1 = lds[kr * S + c + 1];
            if (!INV) {
                const uint32_t e = ((uint32_t)k * (uint32_t)(b0 + c)) << logP;
                y0 = cmul(y0, tw_n(twlo, twhi, e, s));
                y1 = cmul(y1, tw_n(twlo, twhi, e + ((uint32_t)k << logP), s));
            }
            g = base + ((size_t)k << logB) + c;
        } else {
            const int c = pi / (R / 2), k = 2 * (pi % (R / 2));
            const int kr0 = (int)(__builtin_bitreverse32((uint32_t)k) >> (32 - LOG_R));
            const int kr1 = (int)(__builtin_bitreverse32((uint32_t)(k + 1)) >> (32 - LOG_R));
            y0 = lds[kr0 * S + c];
            y1 = lds[kr1 * S + c];
            g = base + (size_t)c * R + k;
        }
        *reinterpret_cast<float4*>(z + g) = make_float4(y0.x, y0.y, y1.x, y1.y);
    }
}

// storage position <-> frequency: pass i's output digit k_i (bits [sum d_<i, + d_i) of k) sits at the high end of p
__device__ __forceinline__ uint32_t xc_freq_of(uint32_t p, FftPlan pl)
{
    uint32_t k = 0;
    int rem = pl.m, sh = 0;
    for (int i = 0; i < pl.passes; ++i) {
        rem -= pl.d[i];
        k |= ((p >> rem) & ((1u << pl.d[i]) - 1)) << sh;
        sh += pl.d[i];
    }
    return k;
}

__device__ __forceinline__ uint32_t xc_pos_of(uint32_t k, FftPlan pl)
{
    uint32_t p = 0;
    int rem = pl.m, sh = 0;
    for (int i = 0; i < pl.passes; ++i) {
        rem -= pl.d[i];
        p |= ((k >> sh) & ((1u << pl.d[i]) - 1)) << rem;
        sh += pl.d[i];
    }
    return p;
}

// Z = A + iB (A, B the spectra of the two scaled real tracks) -> conj(A) B / (s1 s2 N), in place; the thread with
// k <= N - k owns the pair and writes P[N - k] = conj(P[k]) (real correlation: Hermitian spectrum)
__global__ __launch_bounds__(256) void k_xc_product(float2* __restrict__ z, FftPlan pl, const double* __restrict__ stats)
{
    const uint32_t N = 1u << pl.m, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const uint32_t k = xc_freq_of(p, pl), kn = (N - k) & (N - 1);
    if (k > kn) return;
    const uint32_t q = xc_pos_of(kn, pl);
    const float2 zk = z[p], zn = cconj(z[q]);
    const float2 A = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y + zn.y));
    const float2 d = csub(zk, zn);
    const float2 B = make_float2(0.5f * d.y, -0.5f * d.x);              // d / 2i
    const double inv = 1.0 / (pack_scale(stats[3]) * pack_scale(stats[7]) * (double)N);   // a power of two: exact
    float2 P = cmul(cconj(A), B);
    P = make_float2((float)(P.x * inv), (float)(P.y * inv));
    z[p] = P;
    if (q != p) z[q] = cconj(P);
}

// out[k] = c(k - (n1 - 1)) = Re z[(k - n1 + 1) mod N], k < n1 + n2 - 1
__global__ __launch_bounds__(256) void k_xc_extract(const float2* __restrict__ z, int n1, int n2, size_t N, float* __restrict__ out)
{
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= (size_t)n1 + n2 - 1) return;
    out[k] = z[(k + N - (size_t)(n1 - 1)) & (N - 1)].x;
}

// per block of PEAK_SPAN indices: max |Re z| over the valid lags (index < n2 or >= N - n1 + 1), smallest index on a tie
__global__ __launch_bounds__(256) void k_xc_blockmax(const float2* __restrict__ z, int n1, int n2, size_t N, int span,
                                                     float* __restrict__ bmax, int* __restrict__ bidx)
{
    __shared__ float sv[256];
    __shared__ int si[256];
    float best = -1.f;
    int bi = -1;
    for (int o = threadIdx.x; o < span; o += 256) {
        const size_t idx = (size_t)blockIdx.x * span + o;
        if (idx < (size_t)n2 || idx >= N - (size_t)(n1 - 1)) {
            const float v = fabsf(z[idx].x);
            if (v > best) { best = v; bi = (int)idx; }
        }
    }
    sv[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            const float v = sv[threadIdx.x + k];
            const int j = si[threadIdx.x + k];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && j >= 0 && (si[threadIdx.x] < 0 || j < si[threadIdx.x]))) {
                sv[threadIdx.x] = v; si[threadIdx.x] = j;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { bmax[blockIdx.x] = sv[0]; bidx[blockIdx.x] = si[0]; }
}

// TOPK rounds of an argmax over the block maxima (larger value, then lower block); cand[g] = nominated lag, or INT_MIN
__global__ __launch_bounds__(256) void k_xc_select(float* __restrict__ bmax, const int* __restrict__ bidx, int nbm, int n2, size_t N,
                                                   int* __restrict__ cand)
{
    __shared__ float sv[256];
    __shared__ int sb[256];
    for (int g = 0; g < TOPK; ++g) {
        float best = -1.f;
        int bb = -1;
        for (int b = threadIdx.x; b < nbm; b += 256) {
            const float v = bmax[b];
            if (v > best) { best = v; bb = b; }
        }
        sv[threadIdx.x] = best; sb[threadIdx.x] = bb;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if ((int)threadIdx.x < k) {
                const float v = sv[threadIdx.x + k];
                const int j = sb[threadIdx.x + k];
                if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && j >= 0 && (sb[threadIdx.x] < 0 || j < sb[threadIdx.x]))) {
                    sv[threadIdx.x] = v; sb[threadIdx.x] = j;
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const int b = sb[0];
            if (b >= 0 && sv[0] >= 0.f) {
                const long long idx = bidx[b];
                cand[g] = (int)(idx < n2 ? idx : idx - (long long)N);
                bmax[b] = -2.f;                                  // taken
            } else {
                cand[g] = INT32_MIN;
            }
        }
        __syncthreads();
    }
}

// direct sums c(L) = sum_n a2n[n + L] a1n[n] (f64) for the GROUP lags around every nominated lag, over one chunk of n
__global__ __launch_bounds__(256) void k_xc_direct(const float* __restrict__ an1, int n1, const float* __restrict__ an2, int n2,
                                                   const int* __restrict__ cand, int nchunk, double* __restrict__ dpart)
{
    __shared__ double sh[RED_THREADS];
    const int g = blockIdx.y, chunk = blockIdx.x;
    const int c0 = cand[g];
    double acc[GROUP];
#pragma unroll
    for (int d = 0; d < GROUP; ++d) acc[d] = 0.0;
    if (c0 != INT32_MIN) {
        const long long nb = (long long)chunk * DIRECT_CHUNK;
        const long long ne = min((long long)n1, nb + DIRECT_CHUNK);
        for (long long n = nb + threadIdx.x; n < ne; n += 256) {
            const double x = an1[n];
#pragma unroll
            for (int d = 0; d < GROUP; ++d) {
                const long long i2 = n + c0 - NB + d;
                if (i2 >= 0 && i2 < n2) acc[d] += (double)an2[i2] * x;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < GROUP; ++d) {
        const double s = block_sum(acc[d], sh);
        if (threadIdx.x == 0) dpart[((size_t)g * GROUP + d) * nchunk + chunk] = s;
    }
}

// result = {lag, c(lag), |c| / sqrt(E1 E2), min(std1, std2)}: the largest |c| among the valid candidates, the smallest of them on
// a tie; no candidate (a NaN correlation nominates none): lag = c = strength = 0
__global__ __launch_bounds__(128) void k_xc_pick(const int* __restrict__ cand, const double* __restrict__ dpart, int nchunk, int n1, int n2,
                                                 const double* __restrict__ stats, double* __restrict__ result)
{
    __shared__ double cv[NCAND];
    __shared__ long long cl[NCAND];
    const int t = threadIdx.x;
    if (t < NCAND) {
        const int c0 = cand[t / GROUP];
        const long long L = (long long)c0 - NB + t % GROUP;
        const bool ok = c0 != INT32_MIN && L >= -(long long)(n1 - 1) && L <= (long long)(n2 - 1);
        double s = 0.0;
        for (int i = 0; i < nchunk; ++i) s += dpart[(size_t)t * nchunk + i];
        cv[t] = ok ? s : NAN;
        cl[t] = L;
    }
    __syncthreads();
    if (t == 0) {
        int b = -1;
        for (int i = 0; i < NCAND; ++i) {
            if (isnan(cv[i])) continue;
            if (b < 0 || fabs(cv[i]) > fabs(cv[b]) || (fabs(cv[i]) == fabs(cv[b]) && cl[i] < cl[b])) b = i;
        }
        const double e = stats[2] * stats[6];
        const double c = b >= 0 ? cv[b] : 0.0;
        result[0] = b >= 0 ? (double)cl[b] : 0.0;
        result[1] = c;
        result[2] = e > 0.0 ? fabs(c) / sqrt(e) : 0.0;
        result[3] = fmin(stats[1], stats[5]);
    }
}

template <int LOG_R, bool INV>
void launch_pass(float2* z, const Layout& L, int pass, const float2* tw, const float2* lo, const float2* hi, hipStream_t st)
{
    const int m = L.plan.m, s = (m + 1) / 2;
    int above = 0;
    for (int i = 0; i < pass; ++i) above += L.plan.d[i];
    const int logB = m - above - LOG_R;
    if (logB == 0) {
        constexpr int C = LOG_R >= 10 ? 1 : (1 << (12 - LOG_R));       // 4096 points per workgroup
        k_xc_fft<LOG_R, C, false, INV><<<(unsigned)(L.N / ((size_t)C << LOG_R)), 256, 0, st>>>(z, 0, 0, tw, lo, hi, s);
    } else {
        if constexpr (LOG_R <= 9) {
            k_xc_fft<LOG_R, 16, true, INV><<<(unsigned)(L.N >> (LOG_R + 4)), 256, 0, st>>>(z, logB, above, tw, lo, hi, s);
        }
    }
}

template <bool INV>
int run_pass(float2* z, const Layout& L, int pass, const float2* tw, const float2* lo, const float2* hi, hipStream_t st)
{
    switch (L.plan.d[pass]) {
    case 6: launch_pass<6, INV>(z, L, pass, tw, lo, hi, st); break;
    case 7: launch_pass<7, INV>(z, L, pass, tw, lo, hi, st); break;
    case 8: launch_pass<8, INV>(z, L, pass, tw, lo, hi, st); break;
    case 9: launch_pass<9, INV>(z, L, pass, tw, lo, hi, st); break;
    case 10: launch_pass<10, INV>(z, L, pass, tw, lo, hi, st); break;
    case 11: launch_pass<11, INV>(z, L, pass, tw, lo, hi, st); break;
    case 12: launch_pass<12, INV>(z, L, pass, tw, lo, hi, st); break;
    default: v3d_set_error("xcorr: no FFT pass of 2^%d points", L.plan.d[pass]); return V3D_ERR_UNSUPPORTED;
    }
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

// z (packed) -> circular correlation in Re z
int correlate(const Layout& L, char* ws, hipStream_t st)
{
    const double* stats = reinterpret_cast<const double*>(ws + L.stats);
    float2* z = reinterpret_cast<float2*>(ws + L.z);
    const float2* tw = reinterpret_cast<const float2*>(ws + L.tw);
    const float2* lo = reinterpret_cast<const float2*>(ws + L.twlo);
    const float2* hi = reinterpret_cast<const float2*>(ws + L.twhi);
    for (int p = 0; p < L.plan.passes; ++p) {
        const int rc = run_pass<false>(z, L, p, tw, lo, hi, st);
        if (rc) return rc;
    }
    k_xc_product<<<(unsigned)((L.N + 255) / 256), 256, 0, st>>>(z, L.plan, stats);
    V3D_LAUNCH_CHECK();
    for (int p = L.plan.passes - 1; p >= 0; --p) {
        const int rc = run_pass<true>(z, L, p, tw, lo, hi, st);
        if (rc) return rc;
    }
    return V3D_OK;
}

int prepare(const float* a1, int n1, const float* a2, int n2, void* ws, Layout& L, const char* what)
{
    if (!a1 || !a2 || !ws) { v3d_set_error("%s: null pointer", what); return V3D_ERR_ARG; }
    if (n1 < 1 || n2 < 1) { v3d_set_error("%s: lengths %d, %d (need >= 1)", what, n1, n2); return V3D_ERR_ARG; }
    if ((reinterpret_cast<uintptr_t>(ws) & 15) != 0) { v3d_set_error("%s: workspace must be 16-byte aligned", what); return V3D_ERR_ARG; }
    if (!make_layout(n1, n2, L)) {
        v3d_set_error("%s: n1 + n2 - 1 = %lld exceeds the largest FFT (2^%d)", what, (long long)n1 + n2 - 1, XC_MAX_LOG);
        return V3D_ERR_UNSUPPORTED;
    }
    return V3D_OK;
}

void launch_twiddles(const Layout& L, char* ws, hipStream_t st)
{
    const int m = L.plan.m, s = (m + 1) / 2;
    const int n = (1 << TW_LOG) + (1 << s) + (1 << (m - s));
    k_xc_twiddles<<<(n + 255) / 256, 256, 0, st>>>(reinterpret_cast<float2*>(ws + L.tw), reinterpret_cast<float2*>(ws + L.twlo),
                                                   reinterpret_cast<float2*>(ws + L.twhi), m, s);
}

}  // namespace

extern "C" size_t v3d_xcorr_ws_bytes(int n1, int n2)
{
    Layout L;
    return make_layout(n1, n2, L) ? L.total : 0;
}

extern "C" int v3d_xcorr(const float* a1, int n1, const float* a2, int n2, float* out, void* ws, void* stream)
{
    Layout L;
    const int rc = prepare(a1, n1, a2, n2, ws, L, "v3d_xcorr");
    if (rc) return rc;
    if (!out) { v3d_set_error("v3d_xcorr: null pointer"); return V3D_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(ws);
    double* part = reinterpret_cast<double*>(w + L.part);
    double* stats = reinterpret_cast<double*>(w + L.stats);
    launch_twiddles(L, w, st);
    k_xc_reduce<RED_SQ><<<dim3(RED_BLOCKS, 2), RED_THREADS, 0, st>>>(a1, n1, a2, n2, nullptr, nullptr, nullptr, L.N, stats, part);
    k_xc_finish<RED_SQ><<<1, RED_THREADS, 0, st>>>(part, n1, n2, stats);
    k_xc_reduce<RED_RAW><<<RED_BLOCKS, RED_THREADS, 0, st>>>(a1, n1, a2, n2, nullptr, nullptr, reinterpret_cast<float2*>(w + L.z), L.N,
                                                             stats, part);
    V3D_LAUNCH_CHECK();
    const int rc2 = correlate(L, w, st);
    if (rc2) return rc2;
    const size_t nout = (size_t)n1 + n2 - 1;
    k_xc_extract<<<(unsigned)((nout + 255) / 256), 256, 0, st>>>(reinterpret_cast<const float2*>(w + L.z), n1, n2, L.N, out);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_align_audio(const float* a1, int n1, const float* a2, int n2, double* result, void* ws, void* stream)
{
    Layout L;
    const int rc = prepare(a1, n1, a2, n2, ws, L, "v3d_align_audio");
    if (rc) return rc;
    if (!result) { v3d_set_error("v3d_align_audio: null pointer"); return V3D_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(ws);
    float2* z = reinterpret_cast<float2*>(w + L.z);
    float* an1 = reinterpret_cast<float*>(w + L.an1);
    float* an2 = reinterpret_cast<float*>(w + L.an2);
    double* part = reinterpret_cast<double*>(w + L.part);
    double* stats = reinterpret_cast<double*>(w + L.stats);
    float* bmax = reinterpret_cast<float*>(w + L.bmax);
    int* bidx = reinterpret_cast<int*>(w + L.bidx);
    int* cand = reinterpret_cast<int*>(w + L.cand);
    double* dpart = reinterpret_cast<double*>(w + L.dpart);

    launch_twiddles(L, w, st);
    k_xc_reduce<RED_SUM><<<dim3(RED_BLOCKS, 2), RED_THREADS, 0, st>>>(a1, n1, a2, n2, nullptr, nullptr, nullptr, L.N, stats, part);
    k_xc_finish<RED_SUM><<<1, RED_THREADS, 0, st>>>(part, n1, n2, stats);
    k_xc_reduce<RED_VAR><<<dim3(RED_BLOCKS, 2), RED_THREADS, 0, st>>>(a1, n1, a2, n2, nullptr, nullptr, nullptr, L.N, stats, part);
    k_xc_finish<RED_VAR><<<1, RED_THREADS, 0, st>>>(part, n1, n2, stats);
    k_xc_reduce<RED_NORM><<<RED_BLOCKS, RED_THREADS, 0, st>>>(a1, n1, a2, n2, an1, an2, z, L.N, stats, part);
    k_xc_finish<RED_NORM><<<1, RED_THREADS, 0, st>>>(part, n1, n2, stats);
    V3D_LAUNCH_CHECK();
    const int rc2 = correlate(L, w, st);
    if (rc2) return rc2;
    const int span = (int)(L.N < (size_t)PEAK_SPAN ? L.N : (size_t)PEAK_SPAN);
    k_xc_blockmax<<<(unsigned)L.nbm, 256, 0, st>>>(z, n1, n2, L.N, span, bmax, bidx);
    k_xc_select<<<1, 256, 0, st>>>(bmax, bidx, (int)L.nbm, n2, L.N, cand);
    k_xc_direct<<<dim3((unsigned)L.nchunk, TOPK), RED_THREADS, 0, st>>>(an1, n1, an2, n2, cand, (int)L.nchunk, dpart);
    k_xc_pick<<<1, 128, 0, st>>>(cand, dpart, (int)L.nchunk, n1, n2, stats, result);
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}
