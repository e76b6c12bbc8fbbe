// v3d_guided.hip -- guided-filter joint upsampling of the 1080p depth to the 4K guide frame.
//
// Stands where reference upscale.py:21-73 (upscale_depth_maps_ffmpeg: ffmpeg `scale` filter)
// stands; re-specified by BASELINE.json / SURVEY.md 8a-11 + Appendix B.1 as He-Sun-Tang guided
// filtering:  p = bilinear(depth_lo), I = guide/255,
//   a = cov(I,p) / (var(I) + eps),  b = mean(p) - a*mean(I),  q = mean(a)*I + mean(b)
// with (2r+1)^2 box means clipped at the image border and divided by the true pixel count.
//
// Two sweeps (k_gfm for r in {4, 8}: column-marching strips; k_gf for other radii: LDS tiles), box sums
// separable with sliding windows.  HBM traffic: sweep 1 reads guide + depth_lo, writes a,b; sweep 2 reads a,b +
// guide, writes q.
// Numerics: all sums, a and b are float64 (full rate per instruction on gfx950, but no packed form): next to
// zero-depth regions q is ~1e-4 while the window holds values ~40, and the 1e-3 *relative* parity bar cannot be
// met there with f32 cancellation in cov/var and in box(b).
#include "v3d_common.h"
#include <type_traits>

// 1/x to full double precision: v_rcp_f64 seed (~26 bits) + two Newton steps (5 instructions instead of the
// ~30 of an IEEE division; the last-ulp difference is far inside the 1e-3 parity bar)
__device__ __forceinline__ double gf_rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    return r;
}

// the low-resolution depth comes either as float32 (depth.py's frame-out surface, any provider) or straight as the matcher's
// int16 disparity x16: then depth.py:341 `/16` and depth.py:374 `<= 0 -> 0` happen in the load (the float map never exists)
template <typename TD> __device__ __forceinline__ float gf_ld(const TD* p, size_t i);
// float route: a non-finite sample counts as invalid (0, like depth.py:374's `<= 0 -> 0`): the window sums slide, so a NaN or an
// infinity let in would stay in `s += in - out` for the rest of its strip
template <> __device__ __forceinline__ float gf_ld<float>(const float* p, size_t i) { const float v = p[i]; return fabsf(v) <= 3.402823466e38f ? v : 0.f; }
template <> __device__ __forceinline__ float gf_ld<int16_t>(const int16_t* p, size_t i) { const int d = p[i]; return d > 0 ? (float)d * 0.0625f : 0.f; }
// or as the normalised 16-bit sample of the depth PNG (read_png16(...).astype(float32) on the device: the same float values)
template <> __device__ __forceinline__ float gf_ld<uint16_t>(const uint16_t* p, size_t i) { return (float)p[i]; }

// q leaves either as float32 or as the 16-bit sample of the 4K PNG: v3d_rint_u16 (clamp(rint(q), 0, 65535), NaN -> 0), exactly
// what k_round_u16 (v3d_pre.hip) applies to the float32 value the float instantiation stores
typedef unsigned short v3d_u16x2v __attribute__((ext_vector_type(2)));
typedef unsigned short v3d_u16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void gf_st(float* p, float q) { *p = q; }
__device__ __forceinline__ void gf_st(uint16_t* p, float q) { *p = v3d_rint_u16(q); }

#define GF_TX 64
#define GF_RUN 8      // outputs per thread along x in the horizontal pass
#define GF_RMAX 16
// tile height TY = 4 * RUNY: 16 rows for r <= 8, 8 rows above (keeps the f64 tile inside the 160 KiB LDS)

template <typename TD>
__device__ __forceinline__ double gf_bilinear(const TD* __restrict__ src, int Ws, int Hs, double sx, double sy, int x, int y)
{
    const double fx = (x + 0.5) * sx - 0.5, fy = (y + 0.5) * sy - 0.5;
    const double x0f = floor(fx), y0f = floor(fy);
    const double wx = fx - x0f, wy = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int xa = min(max(x0, 0), Ws - 1), xb = min(max(x0 + 1, 0), Ws - 1);
    const int ya = min(max(y0, 0), Hs - 1), yb = min(max(y0 + 1, 0), Hs - 1);
    const double top = (double)gf_ld(src, (size_t)ya * Ws + xa) * (1.0 - wx) + (double)gf_ld(src, (size_t)ya * Ws + xb) * wx;
    const double bot = (double)gf_ld(src, (size_t)yb * Ws + xa) * (1.0 - wx) + (double)gf_ld(src, (size_t)yb * Ws + xb) * wx;
    return top * (1.0 - wy) + bot * wy;
}

// NQ_IN planes staged (2), NQ_SUM planes summed (4 in sweep 1: I, p, II, Ip; 2 in sweep 2: a, b)
template <int SWEEP, int GF_RUNY, typename TD, typename TO>
__global__ __launch_bounds__(256) void k_gf(const TD* __restrict__ depth_lo, int Wlo, int Hlo,
                                            const uint8_t* __restrict__ guide, int W, int H, int r, double eps,
                                            double* __restrict__ A, double* __restrict__ B, TO* __restrict__ out)
{
    constexpr int NS = SWEEP == 1 ? 4 : 2;
    constexpr int GF_TY = 4 * GF_RUNY;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int rows = GF_TY + 2 * r;                 // staged rows
    const int pitch = (GF_TX + 2 * r) | 1;          // odd pitch: row-adjacent threads hit different banks
    const int hp = GF_TX + 1;                       // pitch of the horizontal-sum planes
    double* t0 = smem;                              // I  (sweep 1) / a (sweep 2)
    double* t1 = t0 + rows * pitch;                 // p  (sweep 1) / b (sweep 2)
    double* hs = t1 + rows * pitch;                 // [NS][rows][hp]

    const int tid = threadIdx.x;
    const int ox = blockIdx.x * GF_TX, oy = blockIdx.y * GF_TY;
    const double sx = (double)Wlo / (double)W, sy = (double)Hlo / (double)H;

    // ---- stage the halo tile; out-of-image entries contribute zero ----
    const int tw = GF_TX + 2 * r;
    for (int i = tid; i < rows * tw; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        const int gx = ox - r + tx, gy = oy - r + ty;
        double v0 = 0.0, v1 = 0.0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            if (SWEEP == 1) {
                v0 = (double)guide[(size_t)gy * W + gx] / 255.0;
                v1 = gf_bilinear(depth_lo, Wlo, Hlo, sx, sy, gx, gy);
            } else {
                v0 = A[(size_t)gy * W + gx];
                v1 = B[(size_t)gy * W + gx];
            }
        }
        t0[ty * pitch + tx] = v0;
        t1[ty * pitch + tx] = v1;
    }
    __syncthreads();

    // ---- horizontal sliding sums: task = (row, run of GF_RUN outputs) ----
    const int nruns = GF_TX / GF_RUN;
    for (int task = tid; task < rows * nruns; task += 256) {
        const int row = task % rows, run = task / rows;
        const double* r0 = t0 + row * pitch + run * GF_RUN;
        const double* r1 = t1 + row * pitch + run * GF_RUN;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int k = 0; k <= 2 * r; k++) {
            const double u = r0[k], v = r1[k];
            s0 += u; s1 += v;
            if (SWEEP == 1) { s2 += u * u; s3 += u * v; }
        }
        double* h = hs + row * hp + run * GF_RUN;
        const int hplane = rows * hp;
        for (int j = 0; j < GF_RUN; j++) {
            h[j] = s0; h[hplane + j] = s1;
            if (SWEEP == 1) { h[2 * hplane + j] = s2; h[3 * hplane + j] = s3; }
            if (j + 1 < GF_RUN) {
                const double un = r0[j + 2 * r + 1], vn = r1[j + 2 * r + 1];  // column entering the window
                const double uo = r0[j], vo = r1[j];                          // column leaving it
                s0 += un - uo; s1 += vn - vo;
                if (SWEEP == 1) { s2 += un * un - uo * uo; s3 += un * vn - uo * vo; }
            }
        }
    }
    __syncthreads();

    // ---- vertical sliding sums + the per-pixel algebra: task = (x, run of GF_RUNY outputs) ----
    {
        const int x = tid % GF_TX, runy = tid / GF_TX;                    // 64 x 4 tasks
        const int hplane = rows * hp;
        const double* h = hs + (runy * GF_RUNY) * hp + x;
        double s[NS];
#pragma unroll
        for (int q = 0; q < NS; q++) s[q] = 0.0;
        for (int k = 0; k <= 2 * r; k++)
#pragma unroll
            for (int q = 0; q < NS; q++) s[q] += h[q * hplane + k * hp];
        const int gx = ox + x;
        const int cx = min(gx + r, W - 1) - max(gx - r, 0) + 1;
        for (int j = 0; j < GF_RUNY; j++) {
            const int gy = oy + runy * GF_RUNY + j;
            if (gx < W && gy < H) {
                const int cy = min(gy + r, H - 1) - max(gy - r, 0) + 1;
                const double cnt = (double)(cx * cy);
                if (SWEEP == 1) {
                    const double mI = s[0] / cnt, mp = s[1] / cnt, mII = s[2] / cnt, mIp = s[3] / cnt;
                    const double var = mII - mI * mI, cov = mIp - mI * mp;
                    const double a = cov / (var + eps);
                    A[(size_t)gy * W + gx] = a;
                    B[(size_t)gy * W + gx] = mp - a * mI;
                } else {
                    const double I = (double)guide[(size_t)gy * W + gx] / 255.0;
                    const float q = (float)((s[0] / cnt) * I + (s[1] / cnt));
                    if constexpr (std::is_same<TO, float>::value) out[(size_t)gy * W + gx] = q;
                    else out[(size_t)gy * W + gx] = v3d_rint_u16(q);
                }
            }
            if (j + 1 < GF_RUNY) {
                const int kn = j + 2 * r + 1;
#pragma unroll
                for (int q = 0; q < NS; q++) s[q] += h[q * hplane + kn * hp] - h[q * hplane + j * hp];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Fast path for r in {4, 8}: column-marching sweeps.  A workgroup owns a strip of 256 - 2r output
// columns (+ r halo each side, one thread per column) and marches down a band of rows, TWO rows per step.
// The vertical box sums slide in REGISTERS (a compile-time ring of the last 2r+1 rows' values per column:
// add the entering row, subtract the leaving one); only the per-row vertical sums cross lanes, through a
// double-buffered LDS row pair, for the 2r+1-tap horizontal sum.  In that phase a thread owns a PAIR of adjacent
// output pixels of one of the two rows: their windows share 2r of 2r+1 columns, so 2r+2 values -- r+1 aligned
// 16-byte LDS reads per quantity -- and 2r+1 adds serve both (half the adds, and ds_read_b128 moves 256 B/clk
// where the ds_read2_b64 pairs the compiler forms from single f64 reads move 128: measured, the one-pixel-per-
// thread version spent 72 % of its time in the LDS pipe).  One barrier per two rows, every input element is read
// once per band (+ 2r warm-up rows), a/b/out leave as 16/16/8-byte stores.
// ------------------------------------------------------------------------------------------------
#ifndef GF_CH
#define GF_CH 3      // 16-byte LDS reads in flight per plane in the horizontal phase
#endif
typedef double v3d_f64x2 __attribute__((ext_vector_type(2)));
typedef float v3d_f32x2 __attribute__((ext_vector_type(2)));
typedef float v3d_f32x4 __attribute__((ext_vector_type(4)));

template <int SWEEP, int RR, typename TD, typename TO>
__global__ __launch_bounds__(256) void k_gfm(const TD* __restrict__ depth_lo, int Wlo, int Hlo,
                                             const uint8_t* __restrict__ guide, int W, int H, double eps, int band_h,
                                             double* __restrict__ A, double* __restrict__ B, TO* __restrict__ out,
                                             size_t depth_stride, size_t guide_stride)
{
    static_assert(RR % 2 == 0, "pairs must not straddle the strip's halo boundary");
    constexpr int R = 2 * RR + 1, NOUT = 256 - 2 * RR;
    // sweep 1 sums {g, g*g} as exact int32 (the guide is 8-bit: sum(I) = sum(g)/255, sum(I*I) = sum(g*g)/255^2) and
    // {p, g*p} in f64; sweep 2 sums {a, b} in f64
    __shared__ __attribute__((aligned(16))) double sVd[2][2][2][256];       // [buffer][row of the pair][quantity][column]
    __shared__ __attribute__((aligned(16))) int2 sVi[2][2][256];            // [buffer][row][column] {sum g, sum g*g}
    {   // frame of the batch
        const size_t f = blockIdx.z, n4 = (size_t)W * H;
        depth_lo += f * depth_stride; guide += f * guide_stride; A += f * 2 * n4; B += f * 2 * n4; out += f * n4;
    }
    const int tid = threadIdx.x;
    const int gx = blockIdx.x * NOUT - RR + tid;                    // vertical phase: this thread's image column
    const int ya = blockIdx.y * band_h, yb = min(ya + band_h, H);
    const bool col_ok = gx >= 0 && gx < W;
    const double sx = (double)Wlo / (double)W, sy = (double)Hlo / (double)H;
    const int nsteps = (yb - ya) + 2 * RR;

    // horizontal phase: row hrow of the step's pair, output pixels (hgx, hgx + 1)
    const int hrow = tid >> 7, hq = tid & 127;
    const int hgx = blockIdx.x * NOUT - RR + 2 * hq;
    const bool pair_in = 2 * hq >= RR && 2 * hq < 256 - RR;
    const bool px0 = pair_in && hgx < W, px1 = pair_in && hgx + 1 < W;
    const bool vec_ok = px1 && (W & 1) == 0;                        // both pixels in the image and rows pair-aligned

    // bilinear source coordinates are separable: the x part is a per-thread constant, the y part per row
    int bxa = 0, bxb = 0; double bwx = 0.0;
    if (SWEEP == 1) {
        const double fx = (gx + 0.5) * sx - 0.5, x0f = floor(fx);
        bwx = fx - x0f;
        bxa = min(max((int)x0f, 0), Wlo - 1); bxb = min(max((int)x0f + 1, 0), Wlo - 1);
    }
    double r0[R], r1[R], v0 = 0.0, v1 = 0.0;     // sweep 1: r1 = p ring, v0 = sum p, v1 = sum g*p ; sweep 2: a, b rings and sums
    int rg[R], vg = 0, vgg = 0;                   // sweep 1: g ring, sum g, sum g*g
#pragma unroll
    for (int j = 0; j < R; j++) { r0[j] = 0.0; r1[j] = 0.0; rg[j] = 0; }

    // inputs of the two rows a step consumes, fetched one step ahead (the loads of step s+1 fly during step s)
    // (loads are UNCONDITIONAL, from clamped addresses, and the out-of-image case is a select afterwards: behind a
    //  branch the compiler's s_waitcnt model can no longer count them and waits for the prefetch it just issued)
    struct RowIn { int g; float a0, a1, b0, b1; double n0, n1; bool in; };
    const int gxc = min(max(gx, 0), W - 1);
    auto fetch_row = [&](int t) -> RowIn {
        RowIn q; q.g = 0; q.a0 = q.a1 = q.b0 = q.b1 = 0.f; q.n0 = q.n1 = 0.0;
        const int e = ya - RR + t;                                       // row entering the window
        q.in = col_ok && e >= 0 && e < H && t < nsteps;
        const size_t o = (size_t)min(max(e, 0), H - 1) * W + gxc;
        if (SWEEP == 1) {
            q.g = guide[o];
            const double fy = (e + 0.5) * sy - 0.5, y0f = floor(fy);
            const TD* ra = depth_lo + (size_t)min(max((int)y0f, 0), Hlo - 1) * Wlo;
            const TD* rb = depth_lo + (size_t)min(max((int)y0f + 1, 0), Hlo - 1) * Wlo;
            q.a0 = gf_ld(ra, bxa); q.a1 = gf_ld(ra, bxb); q.b0 = gf_ld(rb, bxa); q.b1 = gf_ld(rb, bxb);
        } else {
            q.n0 = __builtin_nontemporal_load(A + o); q.n1 = __builtin_nontemporal_load(B + o);
        }
        return q;
    };
    RowIn nx[2] = { fetch_row(0), fetch_row(1) };

    int buf = 0;
    for (int t0 = 0; t0 < nsteps; t0 += 2 * R) {
#pragma unroll
        for (int s = 0; s < R; s++) {
            const int tA = t0 + 2 * s;
            if (tA < nsteps) {                                           // uniform
                const int y0 = ya - 2 * RR + tA;                         // output row completed by the first row of the pair
                const bool emit = y0 >= ya;                              // uniform (2*RR is even: pairs never straddle ya)
                const RowIn cur[2] = { nx[0], nx[1] };
                nx[0] = fetch_row(tA + 2); nx[1] = fetch_row(tA + 3);
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int j = (2 * s + rr) % R;                      // compile-time ring slot
                    if (SWEEP == 1) {
                        int gn = 0; double pn = 0.0;
                        if (cur[rr].in) {
                            gn = cur[rr].g;
                            const int e = ya - RR + tA + rr;
                            const double fy = (e + 0.5) * sy - 0.5, wy = fy - floor(fy);
                            // lerps as a + w * (b - a): one subtract and one fma each (the sweep is VALU-bound; the
                            // last-ulp difference to the (1-w)*a + w*b form is 1e-13 of the 1e-3 bar)
                            const double a0 = (double)cur[rr].a0, b0 = (double)cur[rr].b0;
                            const double top = fma(bwx, (double)cur[rr].a1 - a0, a0);
                            const double bot = fma(bwx, (double)cur[rr].b1 - b0, b0);
                            pn = fma(wy, bot - top, top);
                        }
                        const int go = rg[j]; const double po = r1[j];   // row e - R leaves (zeros during warm-up)
                        rg[j] = gn; r1[j] = pn;
                        vg += gn - go; vgg += gn * gn - go * go;
                        v0 += pn - po; v1 = fma((double)gn, pn, fma(-(double)go, po, v1));
                    } else {
                        const double n0 = cur[rr].in ? cur[rr].n0 : 0.0, n1 = cur[rr].in ? cur[rr].n1 : 0.0;
                        const double o0 = r0[j], o1 = r1[j];
                        r0[j] = n0; r1[j] = n1;
                        v0 += n0 - o0; v1 += n1 - o1;
                    }
                    if (emit) {
                        sVd[buf][rr][0][tid] = v0; sVd[buf][rr][1][tid] = v1;
                        if (SWEEP == 1) sVi[buf][rr][tid] = make_int2(vg, vgg);
                    }
                }
                if (emit) {
                    __syncthreads();
                    const int y = y0 + hrow;
                    if (px0 && y < yb) {
                        // 2r+2 columns hgx-r .. hgx+1+r: the inner 2r are common to both pixels' windows.  Reads go out plane
                        // by plane in groups of three, fenced for the scheduler: all of them at once would hold 100+ registers
                        double fq[2], lq[2], cq[2];                       // per plane: first / last column, common part
#pragma unroll
                        for (int q = 0; q < 2; q++) {
                            const v3d_f64x2* d = reinterpret_cast<const v3d_f64x2*>(&sVd[buf][hrow][q][0]) + (hq - RR / 2);
                            double f = 0.0, l = 0.0, c = 0.0;
#pragma unroll
                            for (int ch = 0; ch <= RR; ch += GF_CH) {
                                v3d_f64x2 w[GF_CH];
#pragma unroll
                                for (int i = 0; i < GF_CH; i++) if (ch + i <= RR) w[i] = d[ch + i];
#pragma unroll
                                for (int i = 0; i < GF_CH; i++) if (ch + i <= RR) {
                                    if (ch + i == 0) { f = w[i].x; c = w[i].y; }
                                    else if (ch + i == RR) { c += w[i].x; l = w[i].y; }
                                    else { c += w[i].x; c += w[i].y; }
                                }
                                asm volatile("" : "+v"(c) :: "memory");   // operand: the chunk's adds cannot sink below the next chunk's reads
                            }
                            fq[q] = f; lq[q] = l; cq[q] = c;
                        }
                        int g0 = 0, gg0 = 0, gl = 0, ggl = 0, cg = 0, cgg = 0;
                        if (SWEEP == 1) {
                            const int4* gi = reinterpret_cast<const int4*>(&sVi[buf][hrow][0]) + (hq - RR / 2);
#pragma unroll
                            for (int ch = 0; ch <= RR; ch += 3) {
                                int4 u[3];
#pragma unroll
                                for (int i = 0; i < 3; i++) if (ch + i <= RR) u[i] = gi[ch + i];
#pragma unroll
                                for (int i = 0; i < 3; i++) if (ch + i <= RR) {
                                    if (ch + i == 0) { g0 = u[i].x; gg0 = u[i].y; cg = u[i].z; cgg = u[i].w; }
                                    else if (ch + i == RR) { cg += u[i].x; cgg += u[i].y; gl = u[i].z; ggl = u[i].w; }
                                    else { cg += u[i].x + u[i].z; cgg += u[i].y + u[i].w; }
                                }
                                asm volatile("" : "+v"(cg), "+v"(cgg) :: "memory");
                            }
                        }
                        const double s0a = cq[0] + fq[0], s0b = cq[0] + lq[0], s1a = cq[1] + fq[1], s1b = cq[1] + lq[1];
                        const int cy = min(y + RR, H - 1) - max(y - RR, 0) + 1;
                        // (window widths recomputed here: two thread constants fewer keep sweep 1 inside 128 VGPRs)
                        const int cx0 = min(hgx + RR, W - 1) - max(hgx - RR, 0) + 1, cx1 = min(hgx + 1 + RR, W - 1) - max(hgx + 1 - RR, 0) + 1;
                        const double inva = gf_rcp((double)(cx0 * cy)), invb = cx1 == cx0 ? inva : gf_rcp((double)(cx1 * cy));
                        const size_t o = (size_t)y * W + hgx;
                        if (SWEEP == 1) {
                            const int sga = cg + g0, sgb = cg + gl, sgga = cgg + gg0, sggb = cgg + ggl;
                            double ab[2][2];
#pragma unroll
                            for (int n = 0; n < 2; n++) {
                                const double inv = n ? invb : inva;
                                const double mI = (double)(n ? sgb : sga) * (inv * (1.0 / 255.0)), mp = (n ? s0b : s0a) * inv;
                                const double mII = (double)(n ? sggb : sgga) * (inv * (1.0 / 65025.0)), mIp = (n ? s1b : s1a) * (inv * (1.0 / 255.0));
                                const double var = fma(-mI, mI, mII), cov = fma(-mI, mp, mIp);
                                const double a = cov * gf_rcp(var + eps);
                                ab[n][0] = a; ab[n][1] = fma(-a, mI, mp);
                            }
                            if (vec_ok) {
                                v3d_f64x2 va = { ab[0][0], ab[1][0] }, vb = { ab[0][1], ab[1][1] };
                                __builtin_nontemporal_store(va, reinterpret_cast<v3d_f64x2*>(A + o));
                                __builtin_nontemporal_store(vb, reinterpret_cast<v3d_f64x2*>(B + o));
                            } else {
                                A[o] = ab[0][0]; B[o] = ab[0][1];
                                if (px1) { A[o + 1] = ab[1][0]; B[o + 1] = ab[1][1]; }
                            }
                        } else {
                            const double Ia = (double)guide[o] * (1.0 / 255.0);
                            const double Ib = px1 ? (double)guide[o + 1] * (1.0 / 255.0) : 0.0;
                            const float qa = (float)((s0a * inva) * Ia + (s1a * inva)), qb = (float)((s0b * invb) * Ib + (s1b * invb));
                            if (vec_ok && (std::is_same<TO, float>::value || (reinterpret_cast<uintptr_t>(out + o) & 3) == 0)) {
                                if constexpr (std::is_same<TO, float>::value) {
                                    v3d_f32x2 vq = { qa, qb };
                                    __builtin_nontemporal_store(vq, reinterpret_cast<v3d_f32x2*>(out + o));
                                } else {
                                    v3d_u16x2v vq = { v3d_rint_u16(qa), v3d_rint_u16(qb) };
                                    __builtin_nontemporal_store(vq, reinterpret_cast<v3d_u16x2v*>(out + o));
                                }
                            } else {
                                gf_st(out + o, qa);
                                if (px1) gf_st(out + o + 1, qb);
                            }
                        }
                    }
                    buf ^= 1;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Fused form for r in {4, 8}: BOTH box stages in one launch, a/b never touch HBM (the two-sweep form moves
// 2 x 16 B per 4K pixel through HBM for the f64 a/b planes: 8 of its 11 GB per 30 frames).
//
// A 512-thread workgroup owns a strip of 256 columns (224 outputs at r = 8) and marches down a band of rows, FOUR
// rows per step, with its eight waves SPECIALISED:
//   waves 0-3 (stage 1)  vertical sliding sums of {g, g*g, p, g*p} in a register ring (k_gfm<1>'s arithmetic), four rows of
//                        column sums into LDS; then horizontal window sums as SLIDING RUNS and the per-pixel algebra -> a, b
//                        of four rows -- written to LDS instead of HBM;
//   waves 4-7 (stage 2)  two steps behind: pick the a/b rows up from LDS (one column per thread), vertical sliding sums in a
//                        second register ring (k_gfm<2>'s arithmetic), horizontal sliding runs, q -> HBM.
// Each role keeps ONE ring (<= 128 VGPRs, four waves per SIMD, two workgroups per CU); putting both rings into one
// thread needs ~180 VGPRs.  All hand-offs are double-buffered LDS rows, so a step costs ONE workgroup barrier: in phase p
// stage 1 runs H1(p-1) then V1(p), stage 2 runs H2(p-3) then V2(p-2).
// SLIDING RUNS (round 4).  In a horizontal phase a lane owns a run of FOUR consecutive outputs of one of the step's four rows,
// so all 256 lanes of a role are busy (4 rows x 64 runs): the run's 2r + 4 columns arrive as r + 2 aligned 16-byte reads per
// f64 plane (2r + 4 per int4 plane), the first window is summed once and each further output costs one add and one subtract
// per plane; the four a/b solves (or q evaluations) are independent and interleave.  Round 3's pair form needed r + 1 pair sums
// + 2 singles per plane for TWO outputs, plus a DPP exchange and an extra LDS row per plane in the vertical phase (gone).
// Why the rotating-worker form of round 3 lost (97-151 us per frame against 75.7): it ran runs on a quarter or an
// eighth of the lanes, and a step lasts as long as its longest wave.  Four rows per step give the runs to every lane.
// LDS: I1 = 2 x 16 KB stage-1 column sums + a 3-deep ring of 16-KB a/b row groups = 80 KB (two workgroups per CU).  Stage 2
// overwrites each a/b row group IN PLACE with its column sums (thread t reads column t and writes column t), so a/b and the
// stage-2 sums share one ring: group j is written by H1 in phase j+1, turned into sums by V2 in phase j+2, read by H2 in phase
// j+3.  The general (f64 stage 1) route needs 96 KB and runs one workgroup per CU; 512-column strips exist for I1 only (160 KB).
// Rows are SWIZZLED in 16-byte chunks (gf_swz2 / gf_swz4): a run's reads stride 32 B (f64) or 64 B (int4) across the lanes,
// 2- and 4-way ds_read_b128 bank conflicts in a plain layout, none swizzled.
// The window sums are re-associated against the two-sweep kernels (equal to rounding, not bit for bit); stage 1's sums are
// exact in both routes (integers or exact dyadic f64), so the I1 and f64 routes give the same bits.
// HBM traffic: guide + depth_lo (x 256/224 strip overlap, + 4r warm-up rows per band) in, q out.
// ------------------------------------------------------------------------------------------------
// 16-byte chunk m of a swizzled row: f64 / int2 rows (a run reads chunks 2l + c on lane l), int4 rows (4l + c)
__device__ __forceinline__ int gf_swz2(int m) { return m ^ ((m >> 3) & 1) ^ ((m >> 4) & 1); }
__device__ __forceinline__ int gf_swz4(int m) { return m ^ ((m >> 4) & 3); }
__device__ __forceinline__ int gf_c8(int c) { return 2 * gf_swz2(c >> 1) + (c & 1); }     // element of 8-byte column c

// A RUN'S ADDRESSES.  c0 and RR are multiples of 4, so a run's first chunk is even (f64 / int2 rows) or a multiple of 4 (int4
// rows): its chunks come in aligned pairs (fours) that share the swizzle's XOR term, and chunk i of a group sits at
// (first | term) ^ i.  The rows are GF_ROW_ALIGN-byte aligned in LDS, so the term is read off the BYTE ADDRESS itself (bits 7, 8
// for gf_swz2, bits 8, 9 for gf_swz4) and a group costs one add, a shift or two and an OR, each further chunk one XOR -- against
// an add, two shifts, an XOR and a shift-add per chunk when gf_swz2 / gf_swz4 are spelled out chunk by chunk.
#define GF_ROW_ALIGN 1024
typedef int gf_i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const v3d_f64x2 gf_lds_f64x2;
typedef __attribute__((address_space(3))) const gf_i32x4 gf_lds_i32x4;
__device__ __forceinline__ uint32_t gf_lds_addr(const void* p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p; }
// byte address of chunk 2 * jp of a run that starts at byte address w0 (chunk 2 * jp + 1: the same ^ 16)
__device__ __forceinline__ uint32_t gf_pair_addr(uint32_t w0, int jp) { const uint32_t w = w0 + 32u * jp; return w | (((w >> 3) ^ (w >> 4)) & 16u); }
// byte address of chunk 4 * jg (chunk 4 * jg + i: the same ^ 16 i)
__device__ __forceinline__ uint32_t gf_quad_addr(uint32_t w0, int jg) { const uint32_t w = w0 + 64u * jg; return w | ((w >> 4) & 48u); }

// window sums of the four outputs c0 .. c0+3 of a swizzled f64 row (columns c0 - RR .. c0 + 3 + RR, r + 2 chunks).  plane: byte
// offset of a further plane with the same rows (a multiple of 512: the swizzle's bits stay, and the addresses of `row` serve
// it at an immediate offset)
template <int RR>
__device__ __forceinline__ void gf_run4(const double* row, int c0, double s[4], uint32_t plane = 0u)
{
    static_assert(RR % 4 == 0, "aligned pairs of chunks, read as 4 + 4 + 2 (r = 8) or 4 + 2 (r = 4)");
    const uint32_t w0 = gf_lds_addr(row) + 8u * (uint32_t)(c0 - RR);
    double c = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < RR + 2; k0 += 4) {
        v3d_f64x2 w[4];
#pragma unroll
        for (int i = 0; i < 4; i += 2) if (k0 + i < RR + 2) {
            const uint32_t a = gf_pair_addr(w0, (k0 + i) / 2);
            w[i] = *(gf_lds_f64x2*)(uintptr_t)(a + plane); w[i + 1] = *(gf_lds_f64x2*)(uintptr_t)((a ^ 16u) + plane);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + i;
            if (k == 0) { l0 = w[i].x; l1 = w[i].y; c = w[i].x; c += w[i].y; }
            else if (k == 1) { l2 = w[i].x; c += w[i].x; c += w[i].y; }
            else if (k < RR) { c += w[i].x; c += w[i].y; }
            else if (k == RR) { c += w[i].x; r1 = w[i].y; }
            else if (k == RR + 1) { r2 = w[i].x; r3 = w[i].y; }
        }
        asm volatile("" : "+v"(c) :: "memory");   // the chunk's adds cannot sink below the next chunk's reads
    }
    s[0] = c; s[1] = (s[0] + r1) - l0; s[2] = (s[1] + r2) - l1; s[3] = (s[2] + r3) - l2;
}

// the same for a swizzled int2 row {sum g, sum g*g} (two columns per chunk)
template <int RR>
__device__ __forceinline__ void gf_run4(const int2* row, int c0, int2 s[4])
{
    const uint32_t w0 = gf_lds_addr(row) + 8u * (uint32_t)(c0 - RR);
    int2 c = make_int2(0, 0), l0 = c, l1 = c, l2 = c, r1 = c, r2 = c, r3 = c;
#pragma unroll
    for (int k0 = 0; k0 < RR + 2; k0 += 4) {
        gf_i32x4 w[4];
#pragma unroll
        for (int i = 0; i < 4; i += 2) if (k0 + i < RR + 2) {
            const uint32_t a = gf_pair_addr(w0, (k0 + i) / 2);
            w[i] = *(gf_lds_i32x4*)(uintptr_t)a; w[i + 1] = *(gf_lds_i32x4*)(uintptr_t)(a ^ 16u);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + i;
            const int2 a = make_int2(w[i].x, w[i].y), b = make_int2(w[i].z, w[i].w);
            if (k == 0) { l0 = a; l1 = b; c = make_int2(a.x + b.x, a.y + b.y); }
            else if (k == 1) { l2 = a; c.x += a.x + b.x; c.y += a.y + b.y; }
            else if (k < RR) { c.x += a.x + b.x; c.y += a.y + b.y; }
            else if (k == RR) { c.x += a.x; c.y += a.y; r1 = b; }
            else if (k == RR + 1) { r2 = a; r3 = b; }
        }
        asm volatile("" : "+v"(c.x), "+v"(c.y) :: "memory");
    }
    s[0] = c;
    s[1] = make_int2(s[0].x + r1.x - l0.x, s[0].y + r1.y - l0.y);
    s[2] = make_int2(s[1].x + r2.x - l1.x, s[1].y + r2.y - l1.y);
    s[3] = make_int2(s[2].x + r3.x - l2.x, s[2].y + r3.y - l2.y);
}

// the same for a swizzled int4 row (I1: {sum g, sum g*g, sum P, sum g*P}, one column per chunk)
template <int RR>
__device__ __forceinline__ void gf_run4(const int4* row, int c0, int4 s[4])
{
    const uint32_t w0 = gf_lds_addr(row) + 16u * (uint32_t)(c0 - RR);
    gf_i32x4 c = { 0, 0, 0, 0 }, l0 = c, l1 = c, l2 = c, r1 = c, r2 = c, r3 = c;
#pragma unroll
    for (int k0 = 0; k0 < 2 * RR + 4; k0 += 4) {
        const uint32_t a = gf_quad_addr(w0, k0 / 4);
        gf_i32x4 u[4];
#pragma unroll
        for (int i = 0; i < 4; i++) u[i] = *(gf_lds_i32x4*)(uintptr_t)(a ^ (16u * i));
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + i;
            if (k < 2 * RR + 1) c += u[i];
            if (k == 0) l0 = u[i];
            else if (k == 1) l1 = u[i];
            else if (k == 2) l2 = u[i];
            else if (k == 2 * RR + 1) r1 = u[i];
            else if (k == 2 * RR + 2) r2 = u[i];
            else if (k == 2 * RR + 3) r3 = u[i];
        }
        asm volatile("" : "+v"(c) :: "memory");   // the group's adds cannot sink below the next group's reads
    }
    // the column leaving is subtracted BEFORE the entering one is added: no intermediate spans more than the 2r + 1 columns of a
    // window, so sum g*P stays below 2^31 on the whole documented domain (an 18-column partial sum passes it from d = 1721 on)
    const gf_i32x4 s1 = c - l0 + r1, s2 = s1 - l1 + r2, s3 = s2 - l2 + r3;
    s[0] = make_int4(c.x, c.y, c.z, c.w); s[1] = make_int4(s1.x, s1.y, s1.z, s1.w);
    s[2] = make_int4(s2.x, s2.y, s2.z, s2.w); s[3] = make_int4(s3.x, s3.y, s3.z, s3.w);
}

// a, b of the four pixels hgx .. hgx+3 of row y from their window sums {sum g, sum g*g} (exact ints), {sum p, sum g*p}
template <int RR>
__device__ __forceinline__ void gf_solve4(const int sg[4], const int sgg[4], const double sp[4], const double sgp[4], int hgx, int y,
                                          int W, int H, double eps, double a[4], double b[4])
{
    const int cy = min(y + RR, H - 1) - max(y - RR, 0) + 1;
    int cx[4];
#pragma unroll
    for (int n = 0; n < 4; n++) cx[n] = min(hgx + n + RR, W - 1) - max(hgx + n - RR, 0) + 1;
    const double inv0 = gf_rcp((double)(int)__umul24((uint32_t)cx[0], (uint32_t)cy));          // (counts <= 2r + 1: a 24-bit multiply is exact)
#pragma unroll
    for (int n = 0; n < 4; n++) {
        const double inv = (n == 0 || cx[n] == cx[0]) ? inv0 : gf_rcp((double)(int)__umul24((uint32_t)cx[n], (uint32_t)cy));
        const double mI = (double)sg[n] * (inv * (1.0 / 255.0)), mp = sp[n] * inv;
        const double mII = (double)sgg[n] * (inv * (1.0 / 65025.0)), mIp = sgp[n] * (inv * (1.0 / 255.0));
        const double var = fma(-mI, mI, mII), cov = fma(-mI, mp, mIp);
        const double aa = cov * gf_rcp(var + eps);
        a[n] = aa; b[n] = fma(-aa, mI, mp);
    }
}

// I1 (int16 disparity in, exact 2x upscale): stage 1's four window sums are EXACT INTEGERS.  The disparity is d/16 (the matcher
// gives d <= 1023) and the x2 bilinear weights are {1,3}/4 per axis, so P = 256 p = sum w d (w in {1,3,9}, sum w = 16) is an
// integer <= 16 d; over a 17 x 17 window sum g P <= 289 * 255 * 16 d, below 2^31 for d <= 1821 (the route's domain: r = 4 has
// 81 instead of 289 and more room; the matcher's 1023 gives sum P < 2^23).  The ring holds (P << 8 | g) in ONE register per row, the vertical sums are four int32
// and cross the lanes as one int4 per column.  The a/b algebra converts the four exact sums to f64 -- the very values the f64 sums
// of the general path hold (they are exact there too) -- so the output is bit-identical to it.
template <int RR, int COLS, typename TD, bool I1, typename TO>
__global__ __launch_bounds__(2 * COLS, I1 ? 4 : 2) void k_gff(const TD* __restrict__ depth_lo, int Wlo, int Hlo,
                                                const uint8_t* __restrict__ guide, int W, int H, double eps, int band_h,
                                                TO* __restrict__ out, size_t depth_stride, size_t guide_stride)
{
    static_assert(RR % 4 == 0, "runs of four must not straddle the strip's halo boundaries");
    static_assert(!I1 || std::is_same<TD, int16_t>::value, "the integer stage 1 takes the int16 disparity");
    static_assert(COLS == 256 || (COLS == 512 && I1), "strip width (512 columns: I1 only, the f64 route's rows exceed the LDS)");
    constexpr int R = 2 * RR + 1, NOUT = COLS - 4 * RR, HR = COLS / 4;   // HR runs of four outputs per row
    // stage 1's column sums of the step's four rows: I1 one int4 {sum g, sum g*g, sum P, sum g*P}; general path {sum p, sum g*p}
    // f64 planes + {sum g, sum g*g} int2
    constexpr int S1D = 2 * 4 * 2 * COLS * 8, S1 = I1 ? 2 * 4 * COLS * 16 : S1D + 2 * 4 * COLS * 8;
    // (every row of these arrays starts on a multiple of 512 bytes, the int4 rows of 1024: gf_run4 reads the swizzle off the address)
    static_assert((COLS * 8) % 512 == 0 && (COLS * 16) % GF_ROW_ALIGN == 0 && S1D % GF_ROW_ALIGN == 0, "row alignment of the swizzled LDS rows");
    __shared__ __attribute__((aligned(GF_ROW_ALIGN))) unsigned char sS1[S1];
    double (*sV1)[4][2][COLS] = reinterpret_cast<double (*)[4][2][COLS]>(sS1);       // [buffer][row][sum p | sum g*p][column]
    int2 (*sVi)[4][COLS] = reinterpret_cast<int2 (*)[4][COLS]>(sS1 + (I1 ? 0 : S1D));  // [buffer][row][column] {sum g, sum g*g}
    int4 (*sVq)[4][COLS] = reinterpret_cast<int4 (*)[4][COLS]>(sS1);                  // I1: [buffer][row][column]
    (void)sV1; (void)sVi; (void)sVq;
    __shared__ __attribute__((aligned(GF_ROW_ALIGN))) double sAB[3][4][2][COLS];    // [ring slot][row][a | b, then sum a | sum b][column]
    {   // frame of the batch
        const size_t f = blockIdx.z, n4 = (size_t)W * H;
        depth_lo += f * depth_stride; guide += f * guide_stride; out += f * n4;
    }
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / COLS));    // 0: stage 1 (first half of the waves), 1: stage 2
    const int t = threadIdx.x % COLS;
    const int gx0 = blockIdx.x * NOUT - 2 * RR;                      // image column of strip column 0
    const int gx = gx0 + t;                                          // vertical phases: this thread's column
    const int ya = blockIdx.y * band_h, yb = min(ya + band_h, H);
    const int nrows = (yb - ya) + 4 * RR;                            // input rows ya - 2r .. yb - 1 + 2r
    const int NS = (nrows + 3) >> 2;                                 // steps (four rows each)
    const int NP = NS + 3;                                           // phases: the last H2 runs three phases behind the last V1

    if (role == 0) {
        // ================= stage 1: guide + depth -> a, b =================
        const bool col_ok = gx >= 0 && gx < W;
        const int gxc = min(max(gx, 0), W - 1);
        uint32_t ring[R];                        // I1: (P << 8) | g of the last 2r+1 rows
        double r1[I1 ? 1 : R];                   // general: p ring
        uint32_t rgw[I1 ? 1 : (R + 3) / 4];      // general: g ring, one BYTE per row
        int vg = 0, vgg = 0, vP = 0, vgP = 0;    // I1: the four column sums; general: sum g, sum g*g
        double v0 = 0.0, v1 = 0.0;               // general: sum p, sum g*p
#pragma unroll
        for (int j = 0; j < R; j++) ring[j] = 0u;
#pragma unroll
        for (int j = 0; j < (I1 ? 1 : R); j++) r1[j] = 0.0;
#pragma unroll
        for (int j = 0; j < (I1 ? 1 : (R + 3) / 4); j++) rgw[j] = 0u;
        (void)ring; (void)r1; (void)rgw;
        // I1: x2 bilinear source columns and weights (quarters): even x = 2k: (k-1, k) x (1, 3); odd: (k, k+1) x (3, 1)
        // general: bilinear source coordinates, separable: the x part is a per-thread constant, the y part per row
        int bxa, bxb, wxa = 0, wxb = 0; double bwx = 0.0;
        const double sx = (double)Wlo / (double)W, sy = (double)Hlo / (double)H;
        if constexpr (I1) {
            const int kx = gx >> 1;
            bxa = min(max((gx & 1) ? kx : kx - 1, 0), Wlo - 1); bxb = min(max((gx & 1) ? kx + 1 : kx, 0), Wlo - 1);
            wxa = (gx & 1) ? 3 : 1; wxb = 4 - wxa;
        } else {
            const double fx = (gx + 0.5) * sx - 0.5, x0f = floor(fx);
            bwx = fx - x0f;
            bxa = min(max((int)x0f, 0), Wlo - 1); bxb = min(max((int)x0f + 1, 0), Wlo - 1);
        }
        (void)wxa; (void)wxb; (void)bwx;
        // GF_BRANCH NOTE (the one place that says it).  Three rare cases of this role are kept as BRANCHES by an empty
        // `asm volatile("")` in their body: the image's last run when W % 4 != 0 (H1), a row outside the image or the band's input
        // (V1), and the rotation of a band that starts on an odd row (V1), whose three copies are spelled as v_mov_b32 in asm.
        // Why not plain C++: hipcc (ROCm 7) if-converts each of them into selects that EVERY step executes -- twelve v_cndmask_b32
        // per run for the first, two per row for the second -- and, for the rotation, computes both row orders (twelve
        // multiply-adds for four) or, given a branch, places the rotation's copies on the even path, the one every default band
        // takes.  The asm carries no semantics of its own (the copies are %3 <- %2 <- %1 <- %0 on four distinct registers); a
        // toolchain that branches here unaided makes the statements unnecessary, not wrong.  tools/isa.sh shows the step's
        // stream; DESIGN.md section 4 has the counts.
        // I1: the inputs of a STEP, fetched one step ahead.  The step's four consecutive 4K rows e0 .. e0+3 (e0 = ya - 2r + 4s,
        // of ya's parity) touch the source rows sb .. sb+3 only, sb = (e0 >> 1) - 1 + (e0 & 1):
        //   e0 even: rows (0,1) x (1,3), (1,2) x (3,1), (1,2) x (1,3), (2,3) x (3,1);  e0 odd: (0,1) x (3,1), (0,1) x (1,3),
        //   (1,2) x (3,1), (1,2) x (1,3) -- the fourth is loaded and not used.
        // So a step loads 4 source rows x {bxa, bxb} and four guide bytes.  Every load is a raw buffer load: the row (clamped on
        // the scalar unit) is the scalar offset, the column a 32-bit lane constant -- no 64-bit address arithmetic per lane.  A
        // lane whose column is outside the image carries V3D_BUF_OOB and reads 0 = "g = 0, P = 0"; rows outside the image or the
        // band's input are zeroed when they enter the ring (uniform).  Loads stay unconditional.
        // (the descriptors' sizes and the row offsets are 32-bit products: launch_gff takes this route only when the guide frame,
        // W * H bytes, is below 2 GiB, and the depth frame is half of that)
        struct StepIn { int16_t d[4][2]; uint8_t g[4]; };
        const __amdgpu_buffer_rsrc_t rs_d = buf_rsrc(depth_lo, (uint32_t)Wlo * (uint32_t)Hlo * 2u), rs_g = buf_rsrc(guide, (uint32_t)W * (uint32_t)H);
        const uint32_t og = col_ok ? (uint32_t)gxc : V3D_BUF_OOB;
        const uint32_t oa = col_ok ? 2u * (uint32_t)bxa : V3D_BUF_OOB, ob = col_ok ? 2u * (uint32_t)bxb : V3D_BUF_OOB;
        const int par = ya & 1;                                                  // uniform: parity of every step's first row
        auto fetch_step = [&](int s) -> StepIn {
            StepIn q;
            const int e0 = ya - 2 * RR + 4 * s, sb = (e0 >> 1) - 1 + par;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t so = (uint32_t)min(max(sb + j, 0), Hlo - 1) * (2u * (uint32_t)Wlo);
                q.d[j][0] = __builtin_amdgcn_raw_buffer_load_b16(rs_d, oa, so, 0);
                q.d[j][1] = __builtin_amdgcn_raw_buffer_load_b16(rs_d, ob, so, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                q.g[i] = __builtin_amdgcn_raw_buffer_load_b8(rs_g, og, (uint32_t)min(max(e0 + i, 0), H - 1) * (uint32_t)W, 0);
            return q;
        };
        (void)rs_d; (void)rs_g; (void)og; (void)oa; (void)ob; (void)par;
        // general: inputs of the four rows a step consumes, fetched one step ahead; loads UNCONDITIONAL, from clamped addresses (see k_gfm)
        struct RowIn { int g; float a0, a1, b0, b1; bool in; };
        struct RowIn4 { RowIn r[4]; };
        auto fetch_rows = [&](int t0) -> RowIn4 {
            RowIn4 q4;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                RowIn& q = q4.r[k];
                const int tt = t0 + k, e = ya - 2 * RR + tt;                     // input row entering the window
                q.in = col_ok && e >= 0 && e < H && tt < nrows;
                const int ec = min(max(e, 0), H - 1);
                q.g = guide[(size_t)ec * W + gxc];
                const double fy = (e + 0.5) * sy - 0.5, y0f = floor(fy);
                const TD* ra = depth_lo + (size_t)min(max((int)y0f, 0), Hlo - 1) * Wlo;
                const TD* rb = depth_lo + (size_t)min(max((int)y0f + 1, 0), Hlo - 1) * Wlo;
                q.a0 = gf_ld(ra, bxa); q.a1 = gf_ld(ra, bxb); q.b0 = gf_ld(rb, bxa); q.b1 = gf_ld(rb, bxb);
            }
            return q4;
        };
        (void)fetch_step; (void)fetch_rows;
        // the inputs of the next step: one type per route, so neither route carries the other's state
        typename std::conditional<I1, StepIn, RowIn4>::type nxt;
        if constexpr (I1) nxt = fetch_step(0);
        else nxt = fetch_rows(0);
        for (int p0 = 0; p0 < NP; p0 += R) {
#pragma clang loop unroll(full)
            for (int sp = 0; sp < R; sp++) {
                const int p = p0 + sp;
                if (p < NP) {                                                    // uniform
                    // (thread constants of the horizontal phase are re-derived per phase: nothing hoisted, nothing spilled)
                    int tl = t;
                    asm volatile("" : "+v"(tl));
                    const int hrow = tl / HR, c0 = 4 * (tl % HR), hgx = gx0 + c0;  // run: outputs c0 .. c0+3 of row hrow
                    // ---- H1(p-1): window sums of the four rows V1(p-1) left in LDS -> a, b of four pixels -> the a/b ring ----
                    const int j = p - 1;
                    if (j >= RR / 2 && j < NS) {                                 // uniform
                        const int y = ya - 3 * RR + 4 * j + hrow;                // centre row of this window
                        double a[4] = { 0.0, 0.0, 0.0, 0.0 }, b[4] = { 0.0, 0.0, 0.0, 0.0 };
                        // a/b columns of the strip; hgx is a multiple of 4, so a run is left of the image or not at all
                        // (one condition, one branch: as a chain of && the zeros above were written once per nested branch)
                        if ((int)(c0 >= RR) & (int)(c0 < COLS - RR) & (int)(y >= 0) & (int)(y < H) & (int)(hgx >= 0) & (int)(hgx < W)) {
                            int sg[4], sgg[4]; double sp_[4], sgp[4];
                            if constexpr (I1) {
                                int4 s[4];
                                gf_run4<RR>(&sVq[j & 1][hrow][0], c0, s);
#pragma unroll
                                for (int n = 0; n < 4; n++) {
                                    sg[n] = s[n].x; sgg[n] = s[n].y;
                                    sp_[n] = (double)s[n].z * (1.0 / 256.0); sgp[n] = (double)s[n].w * (1.0 / 256.0);   // exact
                                }
                            } else {
                                int2 si[4];
                                gf_run4<RR>(&sVi[j & 1][hrow][0], c0, si);
                                gf_run4<RR>(&sV1[j & 1][hrow][0][0], c0, sp_);
                                gf_run4<RR>(&sV1[j & 1][hrow][0][0], c0, sgp, COLS * 8u);
#pragma unroll
                                for (int n = 0; n < 4; n++) { sg[n] = si[n].x; sgg[n] = si[n].y; }
                            }
                            gf_solve4<RR>(sg, sgg, sp_, sgp, hgx, y, W, H, eps, a, b);
                            if (hgx + 3 >= W) {                                  // the image's last run, W % 4 != 0 only (GF_BRANCH NOTE)
                                asm volatile("");
#pragma unroll
                                for (int n = 1; n < 4; n++) if (hgx + n >= W) { a[n] = 0.0; b[n] = 0.0; }
                            }
                        }
                        // rows and columns outside the image (and the strip's halo) hand ZERO a/b to stage 2 (its windows count
                        // in-image pixels only); every column of the four rows is written
                        double* ab = &sAB[j % 3][hrow][0][0];
                        const int e0 = 2 * gf_swz2(c0 >> 1), e1 = 2 * gf_swz2((c0 >> 1) + 1);
                        *reinterpret_cast<v3d_f64x2*>(ab + e0) = v3d_f64x2{ a[0], a[1] };
                        *reinterpret_cast<v3d_f64x2*>(ab + e1) = v3d_f64x2{ a[2], a[3] };
                        *reinterpret_cast<v3d_f64x2*>(ab + COLS + e0) = v3d_f64x2{ b[0], b[1] };
                        *reinterpret_cast<v3d_f64x2*>(ab + COLS + e1) = v3d_f64x2{ b[2], b[3] };
                    }
                    // ---- V1(p): four input rows enter the column's window ----
                    if (p < NS) {
                        const int tA = 4 * p;
                        const bool emit = p >= RR / 2;                           // uniform (2r rows of warm-up: a multiple of 4)
                        if constexpr (I1) {
                            const StepIn cs = nxt;
                            nxt = fetch_step(p + 1);
                            // separable x2 bilinear: the horizontal term once per SOURCE row, then one multiply-add per 4K row.
                            // All factors are below 2^24 (d <= 32767, h <= 4 d, P <= 16 d): 24-bit multiplies, the same integers
                            uint32_t h[4], P4[4];                                // P4: 256 p of the step's four rows
#pragma unroll
                            for (int j = 0; j < 4; j++)                          // depth.py:374: <= 0 -> 0
                                h[j] = __umul24((uint32_t)wxa, (uint32_t)max((int)cs.d[j][0], 0)) + __umul24((uint32_t)wxb, (uint32_t)max((int)cs.d[j][1], 0));
                            P4[0] = __umul24(h[1], 3u) + h[0]; P4[1] = __umul24(h[1], 3u) + h[2];
                            P4[2] = __umul24(h[2], 3u) + h[1]; P4[3] = __umul24(h[2], 3u) + h[3];
                            // a band that starts on an odd row (GF_BRANCH NOTE above): the rows rotate IN PLACE, in asm
                            if (par) {
                                asm volatile("v_mov_b32 %3, %2\n\tv_mov_b32 %2, %1\n\tv_mov_b32 %1, %0"
                                             : "+v"(P4[0]), "+v"(P4[1]), "+v"(P4[2]), "+v"(P4[3]));
                                P4[0] = __umul24(h[0], 3u) + h[1];
                            }
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) {
                                const int slot = (4 * sp + rr) % R;              // compile-time ring slot
                                const int e = ya - 2 * RR + tA + rr;
                                uint32_t gn = cs.g[rr], Pn = P4[rr];             // (a column outside the image read zeros)
                                if (!(e >= 0 && e < H && tA + rr < nrows)) {     // uniform, rare (GF_BRANCH NOTE)
                                    asm volatile("");
                                    gn = 0u; Pn = 0u;
                                }
                                const uint32_t go = ring[slot] & 0xFFu, Po = ring[slot] >> 8;
                                ring[slot] = (Pn << 8) | gn;
                                vg += (int)(gn - go); vgg += (int)(__umul24(gn, gn) - __umul24(go, go));
                                vP += (int)(Pn - Po); vgP += (int)(__umul24(gn, Pn) - __umul24(go, Po));
                                if (emit) sVq[p & 1][rr][gf_swz4(t)] = make_int4(vg, vgg, vP, vgP);
                            }
                        } else {
                            const RowIn4 cur = nxt;
                            nxt = fetch_rows(tA + 4);
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) {
                                const int slot = (4 * sp + rr) % R;              // compile-time ring slot
                                const int e = ya - 2 * RR + tA + rr;             // (in the image when cur.r[rr].in)
                                int gn = 0; double pn = 0.0;
                                if (cur.r[rr].in) {
                                    gn = cur.r[rr].g;
                                    const double fy = (e + 0.5) * sy - 0.5, wy = fy - floor(fy);
                                    const double a0 = (double)cur.r[rr].a0, b0 = (double)cur.r[rr].b0;
                                    const double top = fma(bwx, (double)cur.r[rr].a1 - a0, a0);
                                    const double bot = fma(bwx, (double)cur.r[rr].b1 - b0, b0);
                                    pn = fma(wy, bot - top, top);
                                }
                                const int go = (int)((rgw[slot >> 2] >> (8 * (slot & 3))) & 0xFFu); const double po = r1[slot];
                                rgw[slot >> 2] = (rgw[slot >> 2] & ~(0xFFu << (8 * (slot & 3)))) | ((uint32_t)gn << (8 * (slot & 3)));
                                r1[slot] = pn;
                                vg += gn - go; vgg += gn * gn - go * go;
                                v0 += pn - po; v1 = fma((double)gn, pn, fma(-(double)go, po, v1));
                                if (emit) {
                                    const int ct = gf_c8(t);
                                    sV1[p & 1][rr][0][ct] = v0; sV1[p & 1][rr][1][ct] = v1;
                                    sVi[p & 1][rr][ct] = make_int2(vg, vgg);
                                }
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
    } else {
        // ================= stage 2: a, b -> q (k_gfm<2>'s arithmetic) =================
        double r0[R], r1[R], va = 0.0, vb = 0.0;
#pragma unroll
        for (int j = 0; j < R; j++) { r0[j] = 0.0; r1[j] = 0.0; }
        for (int p0 = 0; p0 < NP; p0 += R) {
#pragma clang loop unroll(full)
            for (int sp = 0; sp < R; sp++) {
                const int p = p0 + sp;
                if (p < NP) {                                                    // uniform
                    // Thread constants are RE-DERIVED from the thread index in every phase (the asm makes the value opaque, so
                    // nothing derived from it can be hoisted out of the loop): with two 34-register rings this role has no
                    // room to keep LDS addresses, window widths and column indices live across phases -- hoisted, they spill.
                    int tl = t;
                    asm volatile("" : "+v"(tl));
                    const int hrow = tl / HR, c0 = 4 * (tl % HR), hgx = gx0 + c0;
                    // ---- H2(p-3): window sums of the a/b column sums -> q of four pixels ----
                    {
                        const int j = p - 3;
                        const int y = ya - 4 * RR + 4 * j + hrow;
                        if (j >= RR && j < NS && c0 >= 2 * RR && c0 < COLS - 2 * RR && hgx < W && y < yb) {
                            double sa[4], sb[4];
                            gf_run4<RR>(&sAB[j % 3][hrow][0][0], c0, sa);
                            gf_run4<RR>(&sAB[j % 3][hrow][0][0], c0, sb, COLS * 8u);
                            const int cy = min(y + RR, H - 1) - max(y - RR, 0) + 1;
                            int cx[4];
#pragma unroll
                            for (int n = 0; n < 4; n++) cx[n] = min(hgx + n + RR, W - 1) - max(hgx + n - RR, 0) + 1;
                            const double inv0 = gf_rcp((double)(int)__umul24((uint32_t)cx[0], (uint32_t)cy));
                            const size_t o = (size_t)y * W + hgx;
                            const bool all_in = hgx + 3 < W;
                            const bool vec_ok = all_in && (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(out + o) | reinterpret_cast<uintptr_t>(guide + o)) & 3) == 0
                                                && (reinterpret_cast<uintptr_t>(out + o) & (4 * sizeof(TO) - 1)) == 0;   // f32x4 / u16x4
                            int g[4];
                            if (vec_ok) {
                                const uint32_t g4 = *reinterpret_cast<const uint32_t*>(guide + o);
#pragma unroll
                                for (int n = 0; n < 4; n++) g[n] = (g4 >> (8 * n)) & 0xFF;
                            } else {
#pragma unroll
                                for (int n = 0; n < 4; n++) g[n] = hgx + n < W ? guide[o + n] : 0;
                            }
                            float q[4];
#pragma unroll
                            for (int n = 0; n < 4; n++) {
                                const double inv = (n == 0 || cx[n] == cx[0]) ? inv0 : gf_rcp((double)(int)__umul24((uint32_t)cx[n], (uint32_t)cy));
                                const double I = (double)g[n] * (1.0 / 255.0);
                                q[n] = (float)((sa[n] * inv) * I + (sb[n] * inv));
                            }
                            if (vec_ok) {
                                if constexpr (std::is_same<TO, float>::value) {
                                    const v3d_f32x4 vq = { q[0], q[1], q[2], q[3] };
                                    __builtin_nontemporal_store(vq, reinterpret_cast<v3d_f32x4*>(out + o));
                                } else {
                                    const v3d_u16x4 vq = { v3d_rint_u16(q[0]), v3d_rint_u16(q[1]), v3d_rint_u16(q[2]), v3d_rint_u16(q[3]) };
                                    __builtin_nontemporal_store(vq, reinterpret_cast<v3d_u16x4*>(out + o));
                                }
                            } else {
#pragma unroll
                                for (int n = 0; n < 4; n++) if (hgx + n < W) gf_st(out + o + n, q[n]);
                            }
                        }
                    }
                    // ---- V2(p-2): the four a/b rows H1(p-2) left in the ring enter the column's window; their column sums
                    //      replace them in place ----
                    {
                        const int j = p - 2;
                        if (j >= RR / 2 && j < NS) {
                            const bool emit = j >= RR;                           // uniform
                            double* col = &sAB[j % 3][0][0][gf_c8(tl)];
#pragma unroll
                            for (int rr = 0; rr < 4; rr++) {
                                const int slot = (4 * sp + rr) % R;              // compile-time ring slot
                                const double n0 = col[rr * 2 * COLS], n1 = col[rr * 2 * COLS + COLS];
                                const double o0 = r0[slot], o1 = r1[slot];
                                r0[slot] = n0; r1[slot] = n1;
                                va += n0 - o0; vb += n1 - o1;
                                if (emit) { col[rr * 2 * COLS] = va; col[rr * 2 * COLS + COLS] = vb; }
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
}

template <int RR, typename TD, typename TO>
static void launch_gff(const TD* depth_lo, int Wlo, int Hlo, const uint8_t* guide, int W, int H, double eps,
                       TO* out, int n, size_t depth_stride, size_t guide_stride, hipStream_t st)
{
    // int16 disparity, exact 2x: stage 1 in exact integers (80 KB of LDS: two workgroups per CU); the f64 route needs 96 KB (one)
    bool i1 = false;
    // (its loads address a frame by 32-bit buffer offsets: a guide of 2 GiB or more takes the f64 route, same bits)
    if constexpr (std::is_same<TD, int16_t>::value) i1 = g_v3d_opt.gf_int1 && W == 2 * Wlo && H == 2 * Hlo && (size_t)W * H < ((size_t)1 << 31);
    const int cols = g_v3d_opt.gf_cols == 512 && i1 ? 512 : 256;     // 512-column strips: I1 only (160 KB, one workgroup per CU)
    int band = g_v3d_opt.gf_band;
    if (band <= 0) {
        // auto: every band pays 4r warm-up rows and the launch runs in whole "rounds" of the resident workgroups (equal-length
        // workgroups), so pick the band count that minimises rounds x (band + 4r)
        int dev = 0, ncu = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        const long slots = (long)ncu * (cols == 256 && i1 ? 2 : 1), strips = v3d_cdiv(W, cols - 4 * RR);
        long best = -1;
        for (int nb = 1; nb <= 64 && nb <= H; nb++) {
            const int b = (v3d_cdiv(H, nb) + 1) & ~1;
            const long wgs = strips * v3d_cdiv(H, b) * n, rounds = (wgs + slots - 1) / slots, cost = rounds * (b + 4 * RR);
            if (best < 0 || cost < best) { best = cost; band = b; }
        }
    }
    const dim3 grid(v3d_cdiv(W, cols - 4 * RR), v3d_cdiv(H, band), n);
    if constexpr (std::is_same<TD, int16_t>::value) {
        if (i1 && cols == 512) {
            hipLaunchKernelGGL((k_gff<RR, 512, TD, true, TO>), grid, dim3(1024), 0, st, depth_lo, Wlo, Hlo, guide, W, H, eps, band, out, depth_stride, guide_stride);
            return;
        }
        if (i1) {
            hipLaunchKernelGGL((k_gff<RR, 256, TD, true, TO>), grid, dim3(512), 0, st, depth_lo, Wlo, Hlo, guide, W, H, eps, band, out, depth_stride, guide_stride);
            return;
        }
    }
    hipLaunchKernelGGL((k_gff<RR, 256, TD, false, TO>), grid, dim3(512), 0, st, depth_lo, Wlo, Hlo, guide, W, H, eps, band, out, depth_stride, guide_stride);
}

template <int RR, typename TD, typename TO>
static void launch_gfm(const TD* depth_lo, int Wlo, int Hlo, const uint8_t* guide, int W, int H, double eps,
                       double* A, double* B, TO* out, int n, size_t depth_stride, size_t guide_stride, hipStream_t st)
{
    // band heights (measured sweep, 30 x 4K frames): each band pays 2r warm-up rows; sweep 1 is VALU-bound, sweep 2
    // is bound by its re-reads of the f64 a/b planes
    const int band1 = g_v3d_opt.gf_band1, band2 = g_v3d_opt.gf_band2;
    const dim3 grid1(v3d_cdiv(W, 256 - 2 * RR), v3d_cdiv(H, band1), n), grid2(v3d_cdiv(W, 256 - 2 * RR), v3d_cdiv(H, band2), n);
    hipLaunchKernelGGL((k_gfm<1, RR, TD, TO>), grid1, dim3(256), 0, st, depth_lo, Wlo, Hlo, guide, W, H, eps, band1, A, B, out, depth_stride, guide_stride);
    hipLaunchKernelGGL((k_gfm<2, RR, TD, TO>), grid2, dim3(256), 0, st, depth_lo, Wlo, Hlo, guide, W, H, eps, band2, A, B, out, depth_stride, guide_stride);
}

extern "C" size_t v3d_guided_upscale_ws_bytes(int W, int H)
{
    if (W < 1 || H < 1) return 0;
    return (size_t)W * H * sizeof(double) * 2;
}

static size_t gf_smem(int r, int ns, int ty)
{
    const int rows = ty + 2 * r;
    const int pitch = (GF_TX + 2 * r) | 1;
    return sizeof(double) * ((size_t)2 * rows * pitch + (size_t)ns * rows * (GF_TX + 1));
}

// n frames: frame f at depth_lo + f*depth_stride (elements), guide + f*guide_stride (bytes), out + f*W*H;
// ws must hold n * v3d_guided_upscale_ws_bytes(W, H)
template <typename TD, typename TO>
static int guided_upscale_batch(const TD* depth_lo, int Wlo, int Hlo, size_t depth_stride, const uint8_t* guide,
                                int W, int H, size_t guide_stride, int n, int r, float eps, TO* out, void* ws, void* stream)
{
    if (n < 1) { v3d_set_error("bad batch"); return V3D_ERR_ARG; }
    if (!depth_lo || !guide || !out || !ws) { v3d_set_error("null pointer"); return V3D_ERR_ARG; }
    if (Wlo < 1 || Hlo < 1 || W < 1 || H < 1) { v3d_set_error("bad geometry"); return V3D_ERR_ARG; }
    if (r < 1 || r > GF_RMAX) { v3d_set_error("radius %d outside [1, %d]", r, GF_RMAX); return V3D_ERR_UNSUPPORTED; }
    if (!(eps >= 0.f)) { v3d_set_error("eps must be >= 0"); return V3D_ERR_ARG; }
    if (((uintptr_t)ws & 15) != 0) { v3d_set_error("workspace must be 16-byte aligned"); return V3D_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    double* A = reinterpret_cast<double*>(ws);
    double* B = A + (size_t)W * H;
    if (!g_v3d_opt.gf_tiled && g_v3d_opt.gf_fused && (r == 4 || r == 8)) {
        if (r == 4) launch_gff<4>(depth_lo, Wlo, Hlo, guide, W, H, (double)eps, out, n, depth_stride, guide_stride, st);
        else launch_gff<8>(depth_lo, Wlo, Hlo, guide, W, H, (double)eps, out, n, depth_stride, guide_stride, st);
        V3D_LAUNCH_CHECK();
        return V3D_OK;
    }
    if (!g_v3d_opt.gf_tiled && (r == 4 || r == 8)) {     // larger rings spill: r = 16 takes the tiled kernel
        if (r == 4) launch_gfm<4>(depth_lo, Wlo, Hlo, guide, W, H, (double)eps, A, B, out, n, depth_stride, guide_stride, st);
        else launch_gfm<8>(depth_lo, Wlo, Hlo, guide, W, H, (double)eps, A, B, out, n, depth_stride, guide_stride, st);
        V3D_LAUNCH_CHECK();
        return V3D_OK;
    }
    for (int f = 0; f < n; f++) {
    const TD* depth_lo_f = depth_lo + (size_t)f * depth_stride; const uint8_t* guide_f = guide + (size_t)f * guide_stride;
    double* A = reinterpret_cast<double*>(ws) + (size_t)f * 2 * W * H; double* B = A + (size_t)W * H; TO* out_f = out + (size_t)f * W * H;
    const int ty = r <= 8 ? 16 : 8;
    const dim3 grid(v3d_cdiv(W, GF_TX), v3d_cdiv(H, ty));
    const size_t sm1 = gf_smem(r, 4, ty), sm2 = gf_smem(r, 2, ty);
    if (ty == 16) {
        // above the default dynamic-LDS limit: opt in (160 KiB per CU on gfx950)
        V3D_HIP_CHECK(hipFuncSetAttribute((const void*)k_gf<1, 4, TD, TO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm1));
        V3D_HIP_CHECK(hipFuncSetAttribute((const void*)k_gf<2, 4, TD, TO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm2));
        hipLaunchKernelGGL((k_gf<1, 4, TD, TO>), grid, dim3(256), sm1, st, depth_lo_f, Wlo, Hlo, guide_f, W, H, r, (double)eps, A, B, out_f);
        hipLaunchKernelGGL((k_gf<2, 4, TD, TO>), grid, dim3(256), sm2, st, depth_lo_f, Wlo, Hlo, guide_f, W, H, r, (double)eps, A, B, out_f);
    } else {
        V3D_HIP_CHECK(hipFuncSetAttribute((const void*)k_gf<1, 2, TD, TO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm1));
        V3D_HIP_CHECK(hipFuncSetAttribute((const void*)k_gf<2, 2, TD, TO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm2));
        hipLaunchKernelGGL((k_gf<1, 2, TD, TO>), grid, dim3(256), sm1, st, depth_lo_f, Wlo, Hlo, guide_f, W, H, r, (double)eps, A, B, out_f);
        hipLaunchKernelGGL((k_gf<2, 2, TD, TO>), grid, dim3(256), sm2, st, depth_lo_f, Wlo, Hlo, guide_f, W, H, r, (double)eps, A, B, out_f);
    }
    }
    V3D_LAUNCH_CHECK();
    return V3D_OK;
}

extern "C" int v3d_guided_upscale_batch(const float* depth_lo, int Wlo, int Hlo, size_t depth_stride, const uint8_t* guide,
                                        int W, int H, size_t guide_stride, int n, int r, float eps, float* out, void* ws, void* stream)
{
    return guided_upscale_batch<float, float>(depth_lo, Wlo, Hlo, depth_stride, guide, W, H, guide_stride, n, r, eps, out, ws, stream);
}

extern "C" int v3d_guided_upscale(const float* depth_lo, int Wlo, int Hlo, const uint8_t* guide, int W, int H,
                                  int r, float eps, float* out, void* ws, void* stream)
{
    return guided_upscale_batch<float, float>(depth_lo, Wlo, Hlo, 0, guide, W, H, 0, 1, r, eps, out, ws, stream);
}

// the same filter fed with the matcher's int16 disparity (x16, <= 0 invalid): depth.py:341 `/16` and :374 `<= 0 -> 0` are
// applied as the values are loaded, so the stereo-only pipeline never writes or re-reads the float32 depth plane
extern "C" int v3d_guided_upscale_disp16_batch(const int16_t* disp16, int Wlo, int Hlo, size_t disp_stride, const uint8_t* guide,
                                               int W, int H, size_t guide_stride, int n, int r, float eps, float* out, void* ws, void* stream)
{
    return guided_upscale_batch<int16_t, float>(disp16, Wlo, Hlo, disp_stride, guide, W, H, guide_stride, n, r, eps, out, ws, stream);
}

// the normalised 16-bit depth samples in, the 16-bit 4K samples out: bit-identical to v3d_guided_upscale_batch on the samples as
// float32 followed by v3d_round_to_u16, without the float32 4K plane or the rounding launch.  Stage 1 runs in f64 on every
// route: sum g * P over a window needs ~37 bits, beyond I1's int32
extern "C" int v3d_guided_upscale_u16_batch(const uint16_t* depth_lo, int Wlo, int Hlo, size_t depth_stride, const uint8_t* guide,
                                            int W, int H, size_t guide_stride, int n, int r, float eps, uint16_t* out, void* ws, void* stream)
{
    return guided_upscale_batch<uint16_t, uint16_t>(depth_lo, Wlo, Hlo, depth_stride, guide, W, H, guide_stride, n, r, eps, out, ws, stream);
}
