/*
 * v3d_hip.h -- C ABI of libv3d_hip.so: the MI355X (gfx950) implementation of the per-frame
 * hot path of video_3d_pipeline (SBS frame -> disparity -> 4K depth).
 *
 * The reference has no FFI of its own (pure Python calling OpenCV / ffmpeg); each entry point
 * below replaces one OpenCV / NumPy / ffmpeg call site of the reference and is what a ctypes
 * binding in the reference's depth.py / upscale.py would bind:
 *
 *   v3d_sbs_to_gray        depth.py:250-268 split_sbs_frame (cv2.resize INTER_LANCZOS4) +
 *                          depth.py:274-275, 337-338 cvtColor BGR->RGB->GRAY
 *   v3d_tb_to_gray         the same two sites for a top-bottom (over-under) frame: the resize runs down the columns
 *   v3d_sgbm_create        depth.py:315-325 cv2.StereoSGBM_create(...)
 *   v3d_sgbm_compute[_batch]  depth.py:341 stereo.compute(left_gray, right_gray) -> int16 x16
 *   v3d_disp_to_depth      depth.py:341 .astype(float32)/16.0 and depth.py:374 clamp <=0 -> 0
 *   v3d_mono_blend         depth.py:344-374 the "hybrid" blend: cv2.resize(mono) INTER_LINEAR, min-max to [0, 64],
 *                          0.7 * disparity + 0.3 * mono, clamp <= 0 -> 0 (the mono map comes from the host: DPT or any provider)
 *   v3d_depth_to_u16[_batch]  depth.py:397-406 save_depth_map min-max normalisation to uint16
 *   v3d_guided_upscale     upscale.py:21-73 upscale_depth_maps_ffmpeg (`scale` filter), re-specified
 *                          as guided-filter joint upsampling
 *   v3d_corr_lookup        CREStereo recurrent correlation lookup (BASELINE.json config 4; the
 *                          reference only names it: depth.py:1, CREStereo_model.txt)
 *   v3d_xcorr[_ws_bytes]   utils.py:147 scipy.signal.correlate(a2, a1, 'full') by FFT on the device
 *   v3d_align_audio        utils.py:137-165 find_audio_offset: normalisation, cross-correlation, peak lag and
 *                          correlation strength (align.py's VideoAligner.find_alignment)
 *   v3d_render_stereo_batch  readme.md:37 step 4 (handed to VisionDepth3D there): DIBR from the 4K frame and its 4K depth
 *                          to a side-by-side 3D frame (convert.py, the declared video-3d-convert step)
 *   v3d_render_stereo_subpixel_batch  the same step in 1/16 pixel with interpolated colours (convert.py --subpixel)
 *   v3d_render_stereo_packed_batch  the same step with the eyes packed top-bottom, row-interleaved or as a red-cyan anaglyph
 *                          (convert.py --layout), the output formats VisionDepth3D offers there
 *   v3d_render_stereo_source_batch  no call site in the reference: the same step with the disocclusions taken from the stored eye
 *                          of the SBS frame the depth was computed from (convert.py --fill-from-source)
 *   v3d_temporal_*, v3d_depth_minmax_batch, v3d_depth_to_u16_range_batch  no call site in the reference (it normalises every
 *                          frame on its own, depth.py:397-406): opt-in temporal stabilisation of the depth sequence
 *   v3d_depth_robust_minmax_batch  no call site in the reference either: opt-in percentile white point of that normalisation
 *   v3d_fill_holes_disp16_batch  no call site in the reference (depth.py:374 turns every invalid disparity into depth 0): opt-in
 *                          filling of the matcher's invalid pixels from their scanline neighbours, before /16
 *   v3d_png_*              depth.py:397-406 save_depth_map writes 16-bit PNGs through cv2.imwrite (zlib on the host): opt-in
 *                          deflate of the final u16 / BGR frames on the device, the host only adds the PNG chunks
 *   v3d_frame_signature_batch, v3d_signature_scores  no call site in the reference (align.py rounds the audio offset to a frame and
 *                          nothing checks the pairing): opt-in frame-accurate matching of SBS frames and 4K frames
 *   v3d_quality_reproj_batch, v3d_quality_flicker_batch  no call site in the reference (its readme only names "quality assessment
 *                          metrics"): opt-in, ground-truth-free measures of a run's own depth -- reprojection error and flicker
 *   v3d_plane_profiles_batch, v3d_profile_match_scores, v3d_warp_u16_batch  no call site in the reference (upscale.py:47-63 scales
 *                          the depth to the 4K size and assumes both releases share one framing): opt-in spatial registration of
 *                          the SBS eye to the 4K frame -- crop, letterbox, scale and shift per axis -- and the warp of the low-res
 *                          depth into the 4K frame's framing (register.py: align --register-spatial)
 *
 * Conventions
 *  - every image/volume pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor's
 *    data_ptr()); nothing here allocates on the steady-state path: workspaces belong to the handle
 *    and are sized at create time;
 *  - memory contract (tests/test_abi_guard_gpu.py holds every entry to it): a typed pointer needs only the natural alignment
 *    of its element type and a `void* ws` 16 bytes, unless the entry's comment says otherwise, and an entry that needs more
 *    refuses with V3D_ERR_ARG; rows are `pitch` bytes apart and only the payload of a row is read, with one exception:
 *    v3d_fill_holes_disp16_batch and v3d_render_stereo[_subpixel|_packed|_source]_batch load the aligned 16-byte blocks that hold a row's payload,
 *    so they touch up to 15 bytes on either side of a frame (never a block that holds no payload byte of the input, and no value
 *    from outside the payload reaches a result): an input of theirs must be readable up to those block borders, as every device
 *    allocation is (tests/test_stereo_emulated.py, tests/test_fill_emulated.py).  v3d_median3x3_i16, v3d_filter_speckles and
 *    v3d_mono_blend[_batch] are held to "payload only" byte-exactly on the host as well, with every buffer ending on its last
 *    payload byte (tests/test_speckle_emulated.py, tests/test_blend_emulated.py), and so is the matcher's L-R check + median on
 *    its WTA records, whose never-written columns [0, 64) may hold anything (tests/test_sgbm_post_emulated.py); workspaces and outputs may
 *    hold anything on entry; nothing outside the stated extent of an output or a workspace is written, inputs included;
 *  - `stream` is a hipStream_t passed as void*; calls enqueue work and do NOT synchronise;
 *  - return 0 on success, negative on error; v3d_last_error() returns the thread-local message;
 *  - a handle is bound to one device and is not thread-safe.
 */
#ifndef V3D_HIP_H
#define V3D_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V3D_OK 0
#define V3D_ERR_ARG (-1)
#define V3D_ERR_HIP (-2)
#define V3D_ERR_UNSUPPORTED (-3)
#define V3D_ERR_LOCKSTEP (-4)   /* a lock-step SGM pass timed out on an over-subscribed GPU: see v3d_sgbm_set_lockstep */

#define V3D_MODE_SGBM 0   /* 5 paths, single pass: cv2.STEREO_SGBM_MODE_SGBM (the reference's default) */
#define V3D_MODE_HH   1   /* 8 paths, two passes: cv2.STEREO_SGBM_MODE_HH */

typedef struct v3d_sgbm v3d_sgbm;

/* mirrors the keyword arguments of cv2.StereoSGBM_create (depth.py:315-325).  Values are normalised as OpenCV does;
   what lies outside the accepted domain makes v3d_sgbm_create return V3D_ERR_UNSUPPORTED (nothing is clamped silently).
   Headroom rule of the packed int16 recurrence, with ftzero = max(preFilterCap, 15) | 1 and P2 after normalisation:
       2*P2 + 25*(2*ftzero + 63) < 32767   and   ftzero <= 31
   i.e. P2 <= 15220 for preFilterCap <= 15, P2 <= 14820 for preFilterCap = 30 or 31; preFilterCap >= 32 is refused. */
typedef struct {
    int minDisparity;       /* m in [-64, 0]; anything else is refused.  The search window is d = xL - xR in [m, m + 64): cost column
                               x1 in [0, W - 64) compares the left image's column x1 + 64 + m with the right image's columns
                               x1 + 64 - d', d' in [0, 64).  Output: disparity x16 (true value, so negative inside the window) at
                               image column x1 + 64 + m; INVALID = 16 (m - 1) at rejected pixels and at every column outside
                               [64 + m, W + m) (64 + m columns on the left, -m on the right); 3x3 median and speckle filter
                               (newVal = 16 (m - 1)) after that.  0 = OpenCV's call in depth.py, bit for bit */
    int numDisparities;     /* must be 64 in this build */
    int blockSize;          /* must be 5 in this build */
    int P1, P2;             /* P1 <= 0 -> 2; P2 <= 0 -> 5; P2 < P1 + 1 -> P1 + 1; then the headroom rule above */
    int disp12MaxDiff;      /* <= 0 -> 1; any larger value (>= 63 switches the left-right check off in effect) */
    int preFilterCap;       /* <= 31; ftzero = max(preFilterCap, 15) | 1, so 0..15 act as 15 and an even value as the next odd one */
    int uniquenessRatio;    /* 0..100; < 0 -> 10; > 100 is refused (OpenCV's literal comparison with a negative factor is not reproduced) */
    int speckleWindowSize;  /* <= 0: no speckle filter; any positive size, also beyond the pixel count (every component is removed) */
    int speckleRange;       /* any; joins neighbours with |a - b| <= 16 * speckleRange, compared in 32 bits */
    int mode;               /* V3D_MODE_SGBM / V3D_MODE_HH */
} v3d_sgbm_params;

/* fills the parameter block depth.py:315-325 uses */
void v3d_sgbm_default_params(v3d_sgbm_params* p);

/* create a matcher whose workspaces hold up to max_batch frames of max_width x max_height */
int v3d_sgbm_create(const v3d_sgbm_params* params, int device, int max_width, int max_height,
                    int max_batch, v3d_sgbm** out);
void v3d_sgbm_destroy(v3d_sgbm* h);
/* bytes of device workspace the handle owns */
size_t v3d_sgbm_workspace_bytes(const v3d_sgbm* h);

/* one frame: left/right gray u8 [H][pitch], disp16 out int16 [H][W] (value x16, 16 (minDisparity - 1) invalid: -16 at the default) */
int v3d_sgbm_compute(v3d_sgbm* h, const uint8_t* left_gray, const uint8_t* right_gray,
                     int W, int H, int pitch, int16_t* disp16_out, void* stream);
/* n frames: frame f at left_gray + f*frame_stride (bytes), output frame f at disp16_out + f*W*H.  Frames must not overlap:
   frame_stride < H*pitch with n > 1 is V3D_ERR_ARG, as in the newer batch entries (n == 1 ignores the stride) */
int v3d_sgbm_compute_batch(v3d_sgbm* h, const uint8_t* left_gray, const uint8_t* right_gray,
                           int n, int W, int H, int pitch, size_t frame_stride,
                           int16_t* disp16_out, void* stream);

/* Lock-step pass and an over-subscribed GPU.  The three top-down SGM paths run as ONE pass whose workgroups must all
   be resident together (sized from the occupancy query at create time).  If another process or stream holds CUs, a
   workgroup's bounded wait for its neighbour strip gives up.  The library then NEVER hands out those disparities:
     - the last launch of the call sets every output pixel of the call to INVALID (16 (minDisparity - 1)) and raises a host-visible flag;
     - every later v3d_sgbm_compute* on the handle returns V3D_ERR_LOCKSTEP until the host reacts;
     - v3d_sgbm_poll_errors (no synchronisation) / v3d_sgbm_sync_errors (device synchronise) return the number of
       workgroups that timed out since the state was last cleared (0 = healthy);
     - v3d_sgbm_set_lockstep(h, 0) synchronises, clears the state and makes later calls use one launch per direction
       (same bits, ~2x the SGM time); (h, 1) clears and keeps the lock-step pass.  Then recompute the batch.
   Both paths are GPU paths; there is no CPU fallback. */
int v3d_sgbm_sync_errors(v3d_sgbm* h);
int v3d_sgbm_poll_errors(const v3d_sgbm* h);
int v3d_sgbm_set_lockstep(v3d_sgbm* h, int enable);
/* make `stream` (hipStream_t) wait until the lock-step pass of the latest compute call on `h` has finished.  A host
   that runs a collective (RCCL) on a side stream orders it behind the pass with this call, and the next compute call
   behind the collective: the collective's workgroups then never take CU slots the pass was sized with. */
int v3d_sgbm_stream_wait_lockstep(v3d_sgbm* h, void* stream);

/* Tuning switches of a handle (defaults = the measured best; results never change): "lockstep" 0/1, "hfused" 0/1,
   "chain_dpl" 4/8, "hsplit" 0/1, "hf_persist" 0/1, "lrm_tiles" 0/1, "vdd_dpl" 0/4/8, "cost_band" >= 8, "cost_xcd" / "vdd_xcd" / "hf_xcd" 0/1, "reserve_cus" (CUs
   other streams keep busy during a lock-step pass), "vdd_spin_limit" (poll rounds per lane; 0 = derived from the row
   count), "vdd_launch_frames" (frames per lock-step launch; 0 = sized from the occupancy query and the call's width; more than are
   co-resident is safe and slow, and such a launch ignores "vdd_xcd": the XCD order is a speed switch and never costs forward
   progress), "vdd_seq" 1..0xFFFFF (test hook: the 20-bit sequence number the next lock-step launch carries, so that the wrap and
   its granule sweep can be reached without 2^20 launches; get returns the number the next launch will carry).
   get also knows the read-only "vdd_frames_per_launch_dpl4" / "_dpl8".  Unknown key or bad value: V3D_ERR_ARG.
   The library reads no environment variables. */
int v3d_sgbm_set_option(v3d_sgbm* h, const char* key, int value);
int v3d_sgbm_get_option(const v3d_sgbm* h, const char* key, int* value);
/* library-wide switches of the handle-less entry points: "gf_fused" 1/0 (guided filter as one launch with a/b kept in LDS /
   as two sweeps with a/b through HBM: same bits), "gf_band" (rows per workgroup of the fused kernel, default 432; 0 = chosen per launch from its round count -- then a frame's last bit may depend on the batch size), "gf_cols" 256/512 (its
   strip width; 512 applies to the int16 exact-2x route, the others run 256), "gf_int1" 1/0 (int16 disparity + exact 2x: stage 1 of the fused kernel in exact integers / in f64: same bits), "gf_band1", "gf_band2" (rows per workgroup of the two sweeps), "gf_tiled" 0/1 (force the LDS-tiled guided
   kernel), "corr_fused" 1/0 (1x9 correlation as one gather-GEMM launch with the warped features staged in LDS / as a warp
   kernel + a GEMM kernel: same bits), "corr_gather" 0/1 (register-only gather-GEMM) */
int v3d_set_option(const char* key, int value);
int v3d_get_option(const char* key, int* value);

/* per-stage HIP-event timing on the caller's stream (what bench.py's `roofline` object reads):
   v3d_sgbm_profile(h, 1) resets and enables; run compute calls; synchronise the stream;
   v3d_sgbm_profile_read fills total_ms[stage] (n >= v3d_sgbm_profile_stage_count()) and returns the
   number of recorded calls.  Only full v3d_sgbm_compute[_batch] calls are recorded. */
int v3d_sgbm_profile(v3d_sgbm* h, int enable);
int v3d_sgbm_profile_stage_count(void);
const char* v3d_sgbm_profile_stage_name(int stage);
int v3d_sgbm_profile_read(v3d_sgbm* h, double* total_ms, int n);

/* stage exports used by the parity tests (same inputs as v3d_sgbm_compute, one frame) */
/* cost volume C[y][x1][d'] int16, P2 folded in (x1 = x - 64 - minDisparity, d' = d - minDisparity) */
int v3d_sgbm_debug_cost_volume(v3d_sgbm* h, const uint8_t* left_gray, const uint8_t* right_gray,
                               int W, int H, int pitch, int16_t* C_out, void* stream);
/* raw disparity before median/speckle (after WTA, uniqueness, sub-pixel, L-R check) and,
   if S_out != NULL, the aggregated volume S[y][x1][d']; the image is placed as v3d_sgbm_params.minDisparity says */
int v3d_sgbm_debug_raw(v3d_sgbm* h, const uint8_t* left_gray, const uint8_t* right_gray,
                       int W, int H, int pitch, int16_t* disp16_out, int16_t* S_out, void* stream);
int v3d_median3x3_i16(const int16_t* src, int W, int H, int16_t* dst, void* stream);
/* labels_ws: device scratch of 3*W*H int32 */
int v3d_filter_speckles(int16_t* img, int W, int H, int newVal, int maxSpeckleSize, int maxDiff,
                        int32_t* labels_ws, void* stream);

/* SBS BGR u8 [H][pitch] (W*3 payload bytes per row) -> gray left/right.
   unsqueeze != 0: outputs are W x H (Lanczos4 x2 horizontal); else (W/2) x H. W must be even. */
int v3d_sbs_to_gray(const uint8_t* sbs_bgr, int W, int H, int pitch, int unsqueeze,
                    uint8_t* left_gray, uint8_t* right_gray, void* stream);
/* n frames in one launch: frame f at sbs_bgr + f*frame_stride bytes; outputs packed [n][H][outW].  frame_stride < H*pitch
   with n > 1 is V3D_ERR_ARG (n == 1 ignores the stride) */
int v3d_sbs_to_gray_batch(const uint8_t* sbs_bgr, int n, int W, int H, int pitch, size_t frame_stride,
                          int unsqueeze, uint8_t* left_gray, uint8_t* right_gray, void* stream);
/* the BGR halves themselves (split_sbs_frame's return value), [H][outW][3] */
int v3d_split_sbs(const uint8_t* sbs_bgr, int W, int H, int pitch, int unsqueeze,
                  uint8_t* left_bgr, uint8_t* right_bgr, void* stream);

/* Top-bottom (over-under) input: the same three entries for a frame whose left eye is on top.  TB BGR u8 [H][pitch] (W*3 payload
   bytes per row), H even, Hh = H / 2: eye e (0 = left = top) is rows e*Hh .. e*Hh + Hh - 1.
   unsqueeze == 0: the eye's rows as they are, outputs W x Hh.
   unsqueeze != 0: outputs W x H, cv2.resize(eye, (W, H), INTER_LANCZOS4) -- split_sbs_frame with the axes swapped.  Per channel of
   eye plane S, t0 / t1 the 2^11-scaled int16 taps of the fractions 0.75 / 0.25 (the ones v3d_sbs_to_gray runs along the row):
     acc(2m)     = sum k = 0 .. 7 of t0[k] S[clamp(m - 4 + k, 0, Hh - 1)][x]
     acc(2m + 1) = sum k = 0 .. 7 of t1[k] S[clamp(m - 3 + k, 0, Hh - 1)][x],    v = clamp((acc + 1024) >> 11, 0, 255);
   rows are clamped per eye: no tap of the top eye's last rows reads the bottom eye's first ones.  Gray is v3d_sbs_to_gray's luma of
   the three clamped channels.  Bit-exact contract: tests/tb_ref.py.
   Memory contract, that of the SBS entries: only the 3 W payload bytes of rows 0 .. H - 1 of each frame are read (no pitch padding,
   nothing before or behind the buffer), tb_bgr needs no alignment, the outputs are written densely, exactly once, and nothing else
   is written.  No allocation, no synchronisation, one launch.
   V3D_ERR_ARG: a null pointer, n < 1, H odd or < 2, W < 1, pitch < 3 W, frame_stride < H*pitch with n > 1 (n == 1 ignores the
   stride).  A refused call enqueues nothing. */
int v3d_tb_to_gray(const uint8_t* tb_bgr, int W, int H, int pitch, int unsqueeze,
                   uint8_t* left_gray, uint8_t* right_gray, void* stream);
/* n frames in one launch: frame f at tb_bgr + f*frame_stride bytes; outputs packed [n][outH][W] */
int v3d_tb_to_gray_batch(const uint8_t* tb_bgr, int n, int W, int H, int pitch, size_t frame_stride,
                         int unsqueeze, uint8_t* left_gray, uint8_t* right_gray, void* stream);
/* the BGR eyes themselves, [outH][W][3] */
int v3d_split_tb(const uint8_t* tb_bgr, int W, int H, int pitch, int unsqueeze,
                 uint8_t* left_bgr, uint8_t* right_bgr, void* stream);

int v3d_disp_to_depth(const int16_t* disp16, size_t n, float* depth_out, void* stream);

/* Non-finite input.  Every entry that takes float data states here what a NaN, +inf, -inf, -0.0, a denormal and a finite value
   outside its range do ("Non-finite input"; pinned on the device by tests/test_nonfinite_gpu.py).  The rule:
   where depth.py's NumPy expression defines the result, that result is the contract; where NumPy's answer is a platform accident
   (any astype of a non-finite or out-of-range float), the contract is written out and no such conversion is ever performed.
     Per-frame min / max (v3d_depth_minmax_batch, mn and hi of v3d_depth_robust_minmax_batch): a frame that holds any NaN, of
       either sign and any payload, yields (NaN, NaN), as ndarray.min() / .max() do; +-inf are ordinary extrema; -0.0 sorts below
       +0.0; denormals are ordinary values.
     v3d_temporal_range: a NaN bound in any admissible frame gives (NaN, NaN) for that target, wherever the frame sits in the window.
     v3d_depth_to_u16[_batch], v3d_depth_to_u16_range_batch: a range that is unordered, flat or holds a NaN gives a frame of 0; so
       does an infinite bound (the finite samples give 0, an infinite one NaN -> 0); a NaN sample gives 0; every other sample is
       clamped to [0, 65535] in float32 before it is converted.  So a frame with one NaN or one infinity is written as 0.
     Fixed point d16 (temporal filters, robust histogram, flicker): a sample is valid iff 1 <= rint(16 D): NaN, -inf, -0.0, a
       denormal and every D < 1/32 are invalid, in every entry, decided on the float before any conversion.  Robust histogram and flicker (v3d_depth_math.h's v3d_d16_tap,
       decided on the float before any conversion): a valid sample above the range, D > 2047.9375 and +inf included, counts as
       d16 = 32767 (the histogram keeps its own last bin, 2047).  The two temporal filters decide validity the same way, on the float, but do
       not clamp the value (the clamp cost their kernel 3 to 4 %: DESIGN.md): their domain is D <= 2047.9375, and an output
       pixel whose window holds a tap above it with a non-zero weight has an unspecified (finite) value; every other pixel is
       exact, and nothing outside `out` is written.  tests/temporal_ref.py states the saturating rule; the tests mask those pixels.
     v3d_mono_blend[_batch]: as the NumPy expression.  A NaN in the resized map makes max > min false: the frame is the stereo
       disparity alone.  +inf in the resized map gives e = 0 at its finite pixels and NaN where the map is +inf; -inf makes every
       pixel of the frame NaN.  The resize multiplies taps of weight 0 too: an infinity under one becomes a NaN of the resized map.
     v3d_guided_upscale[_batch] (float input): domain finite, |v| <= 65535; a non-finite sample is read as 0 (an invalid depth).
     v3d_quality_flicker_batch: d16 as above.
     v3d_corr_lookup: a tap whose coordinate is not inside the plane contributes 0; a NaN, infinite or huge flow has no tap inside. */
/* minmax_ws: device scratch of >= 2 floats */
int v3d_depth_to_u16(const float* depth, size_t n, uint16_t* out, float* minmax_ws, void* stream);

/* n frames in one fixed set of launches: frame f (frame_elems floats at depth + f*frame_stride) -> out + f*frame_elems with
   its OWN min/max, bit-identical to v3d_depth_to_u16 on that frame alone (same order of operations, max == min -> 0; a frame that
   holds a NaN or an infinity -> 0: "Non-finite input" above).
   minmax_ws: device scratch of >= 2n floats; n <= 65535 */
int v3d_depth_to_u16_batch(const float* depth, int n, size_t frame_elems, size_t frame_stride, uint16_t* out,
                           float* minmax_ws, void* stream);

/* the upscaled depth as the 16-bit sample the PNG sink stores (stands where upscale.py:47-59 hands gray16 frames to the
   encoder): out = clamp(rint(depth), 0, 65535), round-half-to-even */
int v3d_round_to_u16(const float* depth, size_t n, uint16_t* out, void* stream);

/* depth.py:344-374: depth_out[H][W] = clamp0(w_stereo * disp16/16 + w_mono * (resize(mono) - min) / (max - min) * 64), float32
   arithmetic in the reference's order (bit-identical to the NumPy expression); max == min leaves the stereo disparity.
   mono: f32 [mh][mw] of any size (cv2.resize INTER_LINEAR semantics; same size = no resize).  depth.py uses 0.7 / 0.3.
   ws: device scratch of v3d_mono_blend_ws_bytes(n) bytes.  Batch: frame f at disp16 + f*W*H, mono + f*mono_stride (floats),
   depth_out + f*W*H.  A map with a NaN leaves the stereo disparity; one with an infinity puts NaN into depth_out ("Non-finite
   input" above): what the NumPy expression gives. */
size_t v3d_mono_blend_ws_bytes(int n);
int v3d_mono_blend(const int16_t* disp16, int W, int H, const float* mono, int mw, int mh,
                   float w_stereo, float w_mono, float* depth_out, void* ws, void* stream);
int v3d_mono_blend_batch(const int16_t* disp16, int n, int W, int H, const float* mono, int mw, int mh, size_t mono_stride,
                         float w_stereo, float w_mono, float* depth_out, void* ws, void* stream);

/* guided-filter joint upsampling: depth_lo f32 [Hlo][Wlo], guide u8 luma [Hhi][Whi] -> out f32 [Hhi][Whi].
   Domain of depth_lo: finite, |v| <= 65535 (the accuracy tests' range).  A NaN or an infinity is read as 0, an invalid depth like
   depth.py:374's `<= 0 -> 0`, so the output is finite everywhere (the window sums slide: a NaN let in would stay for the rest of
   its strip).  -0.0 and denormals are ordinary values.
   ws: device scratch of v3d_guided_upscale_ws_bytes(Whi, Hhi) bytes */
size_t v3d_guided_upscale_ws_bytes(int Whi, int Hhi);
int v3d_guided_upscale(const float* depth_lo, int Wlo, int Hlo, const uint8_t* guide, int Whi, int Hhi,
                       int r, float eps, float* out, void* ws, void* stream);
/* n frames in one launch: frame f at depth_lo + f*depth_stride (floats), guide + f*guide_stride (bytes),
   out + f*Whi*Hhi; ws must hold n * v3d_guided_upscale_ws_bytes(Whi, Hhi) bytes */
int v3d_guided_upscale_batch(const float* depth_lo, int Wlo, int Hlo, size_t depth_stride, const uint8_t* guide,
                             int Whi, int Hhi, size_t guide_stride, int n, int r, float eps, float* out,
                             void* ws, void* stream);
/* the same filter fed with the matcher's int16 disparity (x16, <= 0 = invalid): depth.py:341 `.astype(float32)/16.0` and
   depth.py:374 `disparity[disparity <= 0] = 0` happen as the values are loaded, so the stereo-only pipeline
   (sgbm -> upscale) never writes or re-reads the float32 depth plane.  Bit-identical to v3d_disp_to_depth followed by
   v3d_guided_upscale_batch.  Frame f at disp16 + f*disp_stride (int16 elements).
   Domain: disparities (x16 values) up to 1821 (this build's matcher, numDisparities = 64, never exceeds 1023).  For an exact 2x
   upscale and r <= 8 the filter's first stage runs in exact int32 sums: 256 p <= 16 d, so over a 17 x 17 window
   sum g * 256 p <= 289 * 255 * 16 * d < 2^31 => d <= 1821.  A caller feeding larger values must switch that route off first:
   v3d_set_option("gf_int1", 0) (the f64 route takes the whole int16 range).  Nothing checks the values on the device. */
int v3d_guided_upscale_disp16_batch(const int16_t* disp16, int Wlo, int Hlo, size_t disp_stride, const uint8_t* guide,
                                    int Whi, int Hhi, size_t guide_stride, int n, int r, float eps, float* out,
                                    void* ws, void* stream);
/* the same filter between the two 16-bit PNG sequences of the product: depth_lo holds the normalised u16 samples of the 1080p
   depth maps (what v3d_depth_to_u16 writes), out receives the u16 samples of the 4K maps.  Contract: for every r in [1, 16] and
   every route (gf_fused 1/0, gf_tiled 1) the output is bit-identical to v3d_guided_upscale_batch on the samples converted to
   float32 followed by v3d_round_to_u16 -- without the float32 4K plane or the rounding launch.  Stage 1 always runs in f64
   (sum g * P over a window of u16 samples needs ~37 bits).  Frame f at depth_lo + f*depth_stride (elements), guide +
   f*guide_stride (bytes), out + f*Whi*Hhi; ws as for v3d_guided_upscale_batch. */
int v3d_guided_upscale_u16_batch(const uint16_t* depth_lo, int Wlo, int Hlo, size_t depth_stride, const uint8_t* guide,
                                 int Whi, int Hhi, size_t guide_stride, int n, int r, float eps, uint16_t* out,
                                 void* ws, void* stream);
/* BGR [H][W][3] u8 -> luma u8 with the same weights as cvtColor */
int v3d_bgr_to_gray(const uint8_t* bgr, size_t n_pixels, uint8_t* gray, void* stream);

/* CREStereo-style local group correlation on the matrix cores.
   fl, fr: bf16 [h][w][C] (channel-last), flow: f32 [2][h][w], out: f32 [G*9][h][w];
   C = 64*G; pattern 0 = 1x9, 1 = 3x3.  ws: scratch of v3d_corr_ws_bytes(C,h,w) bytes.  fl_bf16, fr_bf16 and ws are accessed
   eight channels at a time and must be 16-byte aligned (else V3D_ERR_ARG).  flow is data: any float is legal.  A tap whose
   coordinate is not inside the plane contributes 0, so a pixel whose flow is NaN, +-inf or beyond any image (1e30, +-2^31) has a
   warped feature of 0; the coordinate is clamped as a float before it becomes an index, and nothing outside fr is read */
size_t v3d_corr_ws_bytes(int C, int h, int w);
int v3d_corr_lookup(const uint16_t* fl_bf16, const uint16_t* fr_bf16, const float* flow,
                    int C, int h, int w, int G, int pattern, float* out, void* ws, void* stream);

/* Audio cross-correlation (v3d_align.hip).  a1, a2: float32 tracks of n1, n2 samples; N = the smallest power of two
   >= n1 + n2 - 1 and >= 2^10; N > 2^26 (about 25 minutes per track at 22.05 kHz) -> V3D_ERR_UNSUPPORTED.
   ws: device scratch of v3d_xcorr_ws_bytes(n1, n2) bytes (0 = unsupported sizes), shared by both entries; each call
   writes its own twiddle tables into it.
   Domain (what tests/test_align_edges_gpu.py pins): finite samples, |a| <= 1e15, and for v3d_align_audio a std of 0 (a
   constant track) or >= 3e-19; outside it the result is unspecified, except for the following.
   Non-finite input: a NaN, +inf or -inf anywhere in either track is legal.  Both entries return V3D_OK and write nothing
   outside out / result / ws.  v3d_xcorr: every out[k] is NaN.  v3d_align_audio: lag = 0, c = 0 and strength = 0 exactly;
   result[3] is the std of the finite track, NaN when neither track is finite. */
size_t v3d_xcorr_ws_bytes(int n1, int n2);
/* out[k], k in [0, n1+n2-1): scipy.signal.correlate(a2, a1, 'full') of the RAW inputs (no normalisation) */
int v3d_xcorr(const float* a1, int n1, const float* a2, int n2, float* out, void* ws, void* stream);
/* result (device, 4 doubles): lag in samples (a1[n] ~ a2[n+lag]), signed c(lag) of the normalised tracks,
   strength, min(std1, std2).  an = (a - mean) / (std + 1e-10) (f64 mean and population std, rounded to float32);
   c(L) = sum_n a2n[n+L] a1n[n]; strength = |c(lag)| / sqrt(E1 E2), E = sum an^2 (0 when E1 E2 = 0).  The FFT only
   nominates candidate lags (one per block of 4096 lags, the 16 largest blocks, +-2 neighbours each); lag and c come from
   direct f64 sums over the overlap.  A maximum of |c| that is unique among the valid lags -(n1-1) .. n2-1 wins.  Among
   exactly tied lags the call returns one of them, with its exact c and strength: the smallest of those nominated, and
   which are nominated depends on float32 rounding (an all-zero correlation returns some valid lag with c = 0). */
int v3d_align_audio(const float* a1, int n1, const float* a2, int n2, double* result, void* ws, void* stream);

/* DIBR stereo rendering (v3d_stereo.hip): 4K BGR frame + its u16 depth (larger = nearer) -> side-by-side 3D.  Per row and eye
   with gain g: source x lands at t = x + floor((g * (D - convergence) + 2^23) / 2^24) (round-half-up of g/256 * (D - conv)/65536
   pixels; outside [0, W) dropped); the nearest source wins (u32 key (D << 16) | (x + 1)); a hole takes the farther of its nearest
   left / right keys (ties left, black if the row has none); the eye pixel is the winning source's colour.  Full SBS: out
   [n][H][2W][3], left eye first; half SBS: [n][H][W][3], eye pixel x' = (E[2x'] + E[2x'+1] + 1) >> 1 per channel.  Bit-exact
   contract: tests/stereo_ref.py.  Frame f at frame_bgr + f*frame_stride (bytes; rows dense, W*3 bytes), depth + f*depth_stride
   (elements; rows dense), out dense.  V3D_ERR_ARG: null pointer, n < 1, W or H < 1, strides smaller than a frame (n > 1), layout
   not 0/1, odd W for half SBS, |gain| >= 2^24, convergence outside [0, 65535]; V3D_ERR_UNSUPPORTED: W > 8192. */
#define V3D_STEREO_FULL_SBS 0
#define V3D_STEREO_HALF_SBS 1
int v3d_render_stereo_batch(const uint8_t* frame_bgr, size_t frame_stride /* bytes */, const uint16_t* depth,
                            size_t depth_stride /* elements */, int n, int W, int H, int gain_left, int gain_right,
                            int convergence, int layout, uint8_t* out_bgr /* dense [n][H][outW][3] */, void* stream);

/* Sub-pixel DIBR (v3d_stereo.hip): the same inputs, strides, layouts, gains, convergence, refusals and memory contract as
   v3d_render_stereo_batch (natural alignment only, rows and frames at any byte offset, nothing written outside out_bgr, no
   allocation, no synchronisation, one launch), with positions in 1/16 px and colours interpolated along connected spans.
   Per row and eye with gain g, all integers (every floor and >> the mathematical one):
     p(x) = 16 x + floor((g * (D[x] - convergence) + 2^19) / 2^20) (may be negative);
     span of source x: L' = p(x+1) - p(x).  Connected iff x + 1 < W and 0 < L' <= V3D_STEREO_TEAR16 (stretched to at most 2 px):
       L = L', colours between F[x] and F[x+1]; otherwise (last column, fold, tear) a point: L = 16, colour F[x].  It covers the
       integer targets t with p(x) <= 16 t < p(x) + L: the first is (p(x) + 15) >> 4, at most two, none for a compressed span;
     Z[t] = max over the spans that cover t, 0 <= t < W, of the u32 key (D[x] << 16) | (x + 1); targets outside [0, W) are dropped;
     a hit target, x = (Z[t] & 0xFFFF) - 1: F[x] for a point; for a connected span w = 16 t - p(x) and per channel
       floor((2 ((L - w) F[x] + w F[x+1]) + L) / (2 L)) (round-half-up linear interpolation);
     a hole (Z[t] = 0) takes the rendered colour of the target that holds the farther of its nearest left / right keys (ties left,
       the only one if one side has none, black if the row has none);
     full and half SBS as above.  Bit-exact contract: tests/stereo_sub_ref.py. */
#define V3D_STEREO_TEAR16 32
int v3d_render_stereo_subpixel_batch(const uint8_t* frame_bgr, size_t frame_stride /* bytes */, const uint16_t* depth,
                                     size_t depth_stride /* elements */, int n, int W, int H, int gain_left, int gain_right,
                                     int convergence, int layout, uint8_t* out_bgr /* dense [n][H][outW][3] */, void* stream);

/* Output packings (v3d_stereo.hip): the eye images EL, ER ([H][W][3] BGR) of v3d_render_stereo_batch (subpixel = 0) or of
   v3d_render_stereo_subpixel_batch (subpixel = 1), packed for the display as `packing` says, in the same launch:
     V3D_PACK_FULL_SBS, V3D_PACK_HALF_SBS   [H][2W][3] / [H][W][3] (W even): the layouts 0 / 1 of those entries, by their kernels;
     V3D_PACK_FULL_TB           [2H][W][3]: rows 0 .. H-1 = EL, rows H .. 2H-1 = ER;
     V3D_PACK_HALF_TB           [H][W][3], H even: eye row y' = (E[2y'] + E[2y'+1] + 1) >> 1 per channel, EL in rows 0 .. H/2-1, ER in
                                rows H/2 .. H-1;
     V3D_PACK_ROWS              [H][W][3]: row y = EL[y] for even y, ER[y] for odd y (row-interleaved, left eye first);
     V3D_PACK_ANAGLYPH_COLOUR   [H][W][3]: B = ER.B, G = ER.G, R = EL.R (red-cyan);
     V3D_PACK_ANAGLYPH_DUBOIS   [H][W][3]: Dubois' least-squares red-cyan matrices in 1/65536, with (Bl, Gl, Rl) = EL[y][x] and
                                (Br, Gr, Rr) = ER[y][x], floor = the arithmetic >> 16 of the int32 sum, clamp255 to [0, 255]:
       R' = clamp255(floor((29891 Rl + 32800 Gl + 11559 Bl -  2849 Rr -  5763 Gr -   102 Br + 32768) / 65536))
       G' = clamp255(floor((-2627 Rl -  2479 Gl -  1033 Bl + 24804 Rr + 48080 Gr -  1209 Br + 32768) / 65536))
       B' = clamp255(floor(( -997 Rl -  1350 Gl -   358 Bl -  4729 Rr -  7403 Gr + 80373 Br + 32768) / 65536))
       (every row sums to 65536: a pixel that is the same grey in both eyes maps to itself).
   Bit-exact contract: tests/stereo_pack_ref.py.  Inputs, strides, gains and convergence as for v3d_render_stereo_batch; out_bgr
   dense [n][outH][outW][3].  The memory contract is that of the two entries above: natural alignment only; rows and frames at
   any byte offset (the aligned 16-byte blocks that hold a row's payload are loaded, as there); nothing is written outside
   out_bgr, and every byte of out_bgr is written; no allocation, no synchronisation, one launch.  V3D_ERR_ARG: everything
   v3d_render_stereo_batch refuses (null pointer, n < 1, W or H < 1, strides smaller than a frame (n > 1), odd W for
   V3D_PACK_HALF_SBS, |gain| >= 2^24, convergence outside [0, 65535]), subpixel not 0 / 1, packing outside 0 .. 6, odd H for
   V3D_PACK_HALF_TB; V3D_ERR_UNSUPPORTED: W > 8192.  A refused call enqueues nothing. */
#define V3D_PACK_FULL_SBS 0
#define V3D_PACK_HALF_SBS 1
#define V3D_PACK_FULL_TB 2
#define V3D_PACK_HALF_TB 3
#define V3D_PACK_ROWS 4
#define V3D_PACK_ANAGLYPH_COLOUR 5
#define V3D_PACK_ANAGLYPH_DUBOIS 6
int v3d_render_stereo_packed_batch(const uint8_t* frame_bgr, size_t frame_stride /* bytes */, const uint16_t* depth,
                                   size_t depth_stride /* elements */, int n, int W, int H, int gain_left, int gain_right,
                                   int convergence, int subpixel /* 0 | 1 */, int packing /* V3D_PACK_* */,
                                   uint8_t* out_bgr /* dense [n][outH][outW][3] */, void* stream);

/* Source fill (v3d_stereo.hip): v3d_render_stereo_packed_batch, except that a hole takes its colour from the stored eye of the SBS
   frame the depth was computed from, not from the background.  Frame f's SBS image at sbs_bgr + f*sbs_stride (bytes), Hs rows
   `pitch` bytes apart, Ws BGR pixels each; We = Ws / 2 and eye e's column i is SBS column e*We + i (S below: that eye's plane).
   Eye plane P(e) at target (t, y), all integers, 64-bit coordinates:
     u = clamp(ax t + bx, 0, (We - 1) << 16), v = clamp(ay y + by, 0, (Hs - 1) << 16);
     i0 = u >> 16, i1 = min(i0 + 1, We - 1), fx = (u >> 8) & 255; j0, j1, fy from v in the same way; per channel
     P = ((256 - fy) ((256 - fx) S[j0][i0] + fx S[j0][i1]) + fy ((256 - fx) S[j1][i0] + fx S[j1][i1]) + 32768) >> 16
   (v3d_warp_u16_batch's arithmetic with the coordinates clamped to the eye in place of a fill value: no tap leaves its eye's half).
   Render: the shift, the z-buffer and the sub-pixel span scatter are unchanged.  In an eye whose bit is set in fill_eyes (bit 0 the
   left eye, bit 1 the right) a target with Z[t] == 0 takes P(eye)[y][t]; an eye whose bit is clear fills as before; the packings and
   the anaglyph matrices apply to the eye colours afterwards.  fill_eyes = 0 is v3d_render_stereo_packed_batch bit for bit (its
   kernels are launched) and sbs_bgr may then be null.  Bit-exact contract: tests/stereo_source_ref.py.
   Memory contract: that of v3d_render_stereo_packed_batch for the frame, the depth and out_bgr.  The SBS frames are read byte by
   byte, by hole targets only: nothing but the 3 Ws payload bytes of a row is touched, no 16-byte block around them, and sbs_bgr
   needs no alignment.  No allocation, no synchronisation, one launch.
   V3D_ERR_ARG: everything v3d_render_stereo_packed_batch refuses; a null sbs_bgr with fill_eyes != 0; Ws odd or < 2; Hs < 1;
   pitch < 3 Ws; sbs_stride < Hs*pitch with n > 1; fill_eyes outside 0 .. 3; ax or ay outside [2^12, 2^20]; |bx| or |by| above 2^40.
   V3D_ERR_UNSUPPORTED: W > 8192 or We > 8192, looked at after every V3D_ERR_ARG above (a call that is wrong in both ways returns
   V3D_ERR_ARG).  Hs has no bound of its own: v, j0 and j1 are 64-bit in the kernel too, so (Hs - 1) << 16 may pass 2^31.
   A refused call enqueues nothing. */
int v3d_render_stereo_source_batch(const uint8_t* frame_bgr, size_t frame_stride /* bytes */, const uint16_t* depth,
                                   size_t depth_stride /* elements */, int n, int W, int H, int gain_left, int gain_right,
                                   int convergence, int subpixel /* 0 | 1 */, int packing /* V3D_PACK_* */,
                                   const uint8_t* sbs_bgr, size_t sbs_stride /* bytes */, int Ws, int Hs, int pitch,
                                   int fill_eyes /* bit 0: left eye, bit 1: right eye */, int64_t ax, int64_t bx, int64_t ay,
                                   int64_t by, uint8_t* out_bgr /* dense [n][outH][outW][3] */, void* stream);

/* Temporal depth stabilisation (v3d_temporal.hip, its integer arithmetic v3d_temporal_math.h): an opt-in stage between the
   disparity and the u16 normalisation.  A buffer holds T frames: depth f32 (frame u at depth + u*depth_stride elements; <= 0 invalid) and left gray u8 (frame u at gray +
   u*gray_stride bytes), rows dense.  Bit-exact contract, all integers: tests/temporal_ref.py.
     d16_u(p) = (int)rint(16 D_u(p)) (half to even), valid iff >= 1: NaN, -inf, -0.0 and denormals are invalid.  Domain:
       D <= 2047.9375 (d16 <= 32767).  A target pixel whose window holds a tap above it (+inf included) with a non-zero weight
       has an unspecified finite value; nothing else is affected;
     cut[u] = 1 iff sum_p |Y_u(p) - Y_{u-1}(p)| > c*W*H (u >= 1, 64-bit integers; cut[0] = 0); frame u may contribute to target t
       iff |u - t| <= R, 0 <= u < T and no cut lies in (min(t,u), max(t,u)];
     s_k(p) = 3x3 edge-replicated sum of |Y_{t+k} - Y_t|, rw_k = max(0, 256 - floor(256 s_k / (9 tau))), tw_k = R + 1 - |k|,
       w_k = tw_k * rw_k * valid(d16_{t+k}(p)); out16 = floor((2 sum w d16 + sum w) / (2 sum w)), 0 if sum w = 0 or (fill = 0 and
       d16_t(p) invalid); output depth = out16 / 16 (exact in float32), finite whatever the input holds.
       int32 holds every sum for R <= 8 and d16 <= 32767.
   Every entry enqueues on `stream`, never synchronises, never allocates, and takes device pointers only.
   V3D_ERR_ARG: null pointer, T outside [1, 65535], W or H < 1, targets outside the buffer, R outside [0, 8], tau outside [1, 255],
   c outside [0, 256], fill not 0/1, a stride below the frame size (T > 1). */
/* cut_out u8 [T]; ws: device scratch of >= 8*T bytes, 8-byte aligned */
int v3d_temporal_cuts(const uint8_t* gray, size_t gray_stride /* bytes */, int T, int W, int H, int c, void* ws,
                      uint8_t* cut_out, void* stream);
/* minmax_out f32 [T][2]: min and max of each frame, the exact values v3d_depth_to_u16_batch reduces; (NaN, NaN) for a frame that
   holds any NaN, +-inf as ordinary extrema, -0.0 below +0.0 */
int v3d_depth_minmax_batch(const float* depth, int T, size_t frame_elems, size_t frame_stride /* elements */, float* minmax_out,
                           void* stream);
/* lohi_out f32 [n][2] for targets t0 .. t0+n-1: min of the minima, max of the maxima over the frames that may contribute;
   (NaN, NaN) if any bound of any of those frames is NaN, whatever the frame's position in the window */
int v3d_temporal_range(const float* minmax, const uint8_t* cut, int T, int t0, int n, int R, float* lohi_out, void* stream);
/* out f32 dense [n][H][W]: the filtered depth of targets t0 .. t0+n-1, windows clipped to [0, T) */
int v3d_temporal_filter_batch(const float* depth, size_t depth_stride /* elements */, const uint8_t* gray,
                              size_t gray_stride /* bytes */, int T, int W, int H, int t0, int n, int R, int tau, int fill,
                              const uint8_t* cut, float* out, void* stream);
/* Motion compensation of the temporal window (the block search in v3d_temporal_mc.hip, the filter in v3d_temporal.hip: one kernel
   for both filter entries; `--temporal-motion S`, S in 1..32 pixels per frame step).
   Bit-exact contract, all integers: tests/temporal_mc_ref.py.  Blocks are 16x16 luma pixels on a grid anchored at (0,0), edge
   blocks clipped to the frame: BW = ceil(W/16), BH = ceil(H/16), n_b = a block's pixel count.
     Fields: for every frame u of the buffer and v = u+1 (forward, F_u) or v = u-1 (backward, Bk_u), every block b and candidate
       (dx,dy) in [-S,S]^2: sad = sum over b's pixels |Y_u(x,y) - Y_v(clamp(x+dx,0,W-1), clamp(y+dy,0,H-1))|,
       cost = sad + max(n_b >> 2, 1) * (|dx|+|dy|), key = cost * 8192 + (dy+S)*(2S+1) + (dx+S); b's vector is the candidate with
       the smallest key (cost <= 65280 + 64*64, so key < 2^30; ranks <= 4224 < 8192).  F_{T-1} = Bk_0 = 0.
       Storage: int16 [T][BH][BW][2] as (dx,dy).
     resid[u] = sum over blocks of the unpenalised sad of Bk_u's chosen candidates (u64; resid[0] = 0); cut[u] = resid[u] > c*W*H.
       With motion on this rule takes the place of v3d_temporal_cuts'.
     Chained vector of block b from target t to u = t+k: m = 0; for each step j = 0 .. |k|-1 toward u,
       m += F_{t+j}[block containing clamp(c_b + m)] (Bk_{t-j} going backward), c_b = (min(16 bx + 8, W-1), min(16 by + 8, H-1)),
       clamped per coordinate to the frame; |m| <= R*S <= 256 per coordinate.
     Filter: v3d_temporal_filter_batch's arithmetic with frame u read at q = p + m, m the vector of p's block:
       s_k = 3x3 sum over delta of |Y_u(clamp(q+delta)) - Y_t(clamp(p+delta))|, the depth tap is d16_u(q), and a tap whose q lies
       outside the frame has weight 0.  With all-zero fields the output is v3d_temporal_filter_batch's, bit for bit.
   Both entries enqueue on `stream`, never synchronise, never allocate, and take device pointers only.
   V3D_ERR_ARG: as for the entries above, S outside [1, 32], resid not 8-byte aligned, a field not 2-byte aligned. */
/* mv_fwd, mv_bwd int16 [T][BH][BW][2], resid u64 [T] (zeroed by the entry), cut_out u8 [T]: three launches */
int v3d_temporal_motion(const uint8_t* gray, size_t gray_stride /* bytes */, int T, int W, int H, int S, int c, int16_t* mv_fwd,
                        int16_t* mv_bwd, unsigned long long* resid, uint8_t* cut_out, void* stream);
/* out f32 dense [n][H][W]: the compensated filter of targets t0 .. t0+n-1; mv_fwd, mv_bwd and cut as v3d_temporal_motion wrote them */
int v3d_temporal_filter_mc_batch(const float* depth, size_t depth_stride /* elements */, const uint8_t* gray,
                                 size_t gray_stride /* bytes */, int T, int W, int H, int t0, int n, int R, int tau, int fill,
                                 const uint8_t* cut, const int16_t* mv_fwd, const int16_t* mv_bwd, float* out, void* stream);
/* v3d_depth_to_u16_batch with frame f's (min, max) read from lohi[2f], lohi[2f+1] instead of reduced from the frame: same
   float32 operations in the same order, hi == lo -> 0, the result clamped to [0, 65535] before the conversion.  With a frame's
   own min and max it reproduces v3d_depth_to_u16_batch bit for bit.  lohi = (-inf, inf), (NaN, x), (x, NaN), (inf, inf) or any
   other range that is not finite and ordered gives a frame of 0; a NaN sample gives 0.  out dense [n][frame_elems]; n <= 65535 */
int v3d_depth_to_u16_range_batch(const float* depth, int n, size_t frame_elems, size_t frame_stride /* elements */,
                                 const float* lohi, uint16_t* out, void* stream);

/* Robust depth range (v3d_range.hip): v3d_depth_minmax_batch with the max replaced by a percentile of the frame's valid
   disparities, so a handful of mismatched pixels cannot set the white point.  Bit-exact contract, integers up to the last
   conversion: tests/range_ref.py.  q = percentile in parts per 10000, in [5000, 10000]; per frame, with d16 as above:
     hist[b] = #{p: d16(p) == b} for 1 <= b <= 2046, hist[2047] = #{p: d16(p) >= 2047}; n_valid = sum hist;
     k = max(1, ceil(q * n_valid / 10000)) (64-bit); hi16 = the smallest b with hist[1] + .. + hist[b] >= k;
     mn, mx = the frame's float min and max exactly as v3d_depth_minmax_batch gives them (the min includes the invalid zeros);
     hi = mx if n_valid == 0 or hi16 == 2047, else max((float)hi16 / 16, mn); a frame that holds a NaN gives (NaN, NaN); NaN and
     -inf are invalid (not counted), +inf and every D >= 2047/16 land in hist[2047].
   minmax_out f32 [T][2] = (mn, hi): the layout v3d_temporal_range and v3d_depth_to_u16_range_batch read.  At most
   n_valid - k valid pixels of a frame lie above its hi; on depths that are multiples of 1/16 below 2047/16, q = 10000 gives mx.
   ws: device scratch of v3d_depth_robust_minmax_ws_bytes(T) bytes, 16-byte aligned.  Enqueues three launches on `stream`,
   never synchronises, never allocates.  V3D_ERR_ARG: null pointer, T outside [1, 65535], frame_elems < 1, q outside
   [5000, 10000], a stride below the frame size (T > 1), a misaligned ws; V3D_ERR_UNSUPPORTED: frame_elems >= 2^32. */
size_t v3d_depth_robust_minmax_ws_bytes(int T);
int v3d_depth_robust_minmax_batch(const float* depth, int T, size_t frame_elems, size_t frame_stride /* elements */, int q,
                                  void* ws, float* minmax_out, void* stream);

/* Disparity hole filling (v3d_fill.hip): an opt-in stage on the matcher's int16 disparity, directly after the matcher and before
   /16, the hybrid blend, the temporal stage, the range and the normalisation.  Bit-exact contract, all integers:
   tests/fill_ref.py.  Per frame d (int16 [H][W]) a pixel is a hole iff d < 0; a disparity of 0 is valid and stays.
     1. rows: in a row with at least one non-hole pixel, a hole at x takes min(d[a], d[b]) of the nearest non-hole pixels a (left)
        and b (right) of the INPUT row, or the only one if one side has none; non-hole pixels are copied unchanged;
     2. empty rows: a row with no non-hole pixel becomes a copy of the step-1 output of the nearest non-empty row by |r - y|, ties
        to the row above; a frame with no non-hole pixel at all is copied unchanged.
   So the result has no negative value unless the whole frame was invalid, the stage is idempotent, and valid pixels keep their
   bits.  Frame f at disp16 + f*disp_stride (elements; rows dense), out dense [n][H][W]; int16 pointers need 2-byte alignment
   only (W may be odd, frames may start at odd element offsets).  out == disp16 (in place) is allowed iff n == 1 or
   disp_stride == W*H; any other overlap of out with disp16 is not.  ws: device scratch of v3d_fill_holes_ws_bytes(n, H) bytes
   (one non-empty flag per row), 16-byte aligned.  Enqueues two launches on `stream`, never synchronises, never allocates.
   V3D_ERR_ARG: null pointer, n outside [1, 65535], W or H < 1, disp_stride < W*H with n > 1, a misaligned ws, out == disp16
   with another stride; V3D_ERR_UNSUPPORTED: W > 8192 or H > 65535.  v3d_fill_holes_ws_bytes is 0 for arguments the entry
   refuses. */
size_t v3d_fill_holes_ws_bytes(int n, int H);
int v3d_fill_holes_disp16_batch(const int16_t* disp16, size_t disp_stride /* elements */, int n, int W, int H,
                                int16_t* out /* dense [n][H][W] */, void* ws, void* stream);

/* GPU PNG encoding (v3d_png.hip): an opt-in sink stage.  The device turns each final frame into a complete zlib stream
   (RFC 1950 / 1951) whose payload is byte for byte the filtered image the host encoder hands to zlib -- per scanline the byte 1
   (filter "sub") and the samples minus the sample one pixel to the left, gray16 big-endian, BGR8 in RGB order -- and the host
   wraps signature, IHDR, one IDAT with its CRC-32 and IEND around it (utils.png_from_stream).  Bit-exact contract:
   tests/png_ref.py.  Stream: 78 01; per scanline one deflate block (BFINAL = 0) and an empty stored block (000, zero bits to
   the byte boundary, 00 00 FF FF), so every scanline is coded on its own and ends on a byte boundary; then 01 00 00 FF FF and
   the Adler-32 of the payload, big-endian.  Tokens of a scanline of RL = 1 + bpp*W bytes: literals and matches at the single
   distance bpp (2 or 3): with m[i] = i >= bpp && raw[i] == raw[i - bpp], a maximal run of L true positions is L / 258 matches of
   258 and, for r = L % 258, one match if r >= 3, else r literals.  The block is coded with the cheapest (header + codes,
   ties to the lowest index) of the constant code books of csrc/v3d_png_books.h (tools/make_png_books.py); book 0 is deflate's
   fixed code, which spends at most 9 bits per payload byte, so a scanline takes at most ceil(9*RL/8) + 8 bytes and
     v3d_png_stream_bound(fmt, W, H) = 2 + H * (ceil(9*RL/8) + 8) + 9,
     v3d_png_out_bytes(fmt, n, W, H) = n * (that bound rounded up to 16).
   img: frame f at (const char*)img + f*frame_stride (BYTES), rows dense; V3D_PNG_GRAY16: uint16 [H][W], 2-byte alignment;
   V3D_PNG_BGR8: uint8 [H][W][3], any alignment.  out: frame f's stream starts at out[offsets[f]], offsets[0] = 0 and every offset
   is a multiple of 16 (each stream's size rounded up); offsets[n] is the used size; EVERY byte of out up to v3d_png_out_bytes is
   written: what lies between the streams and behind the last one is zero.  A stream's own size is not stored: it closes with
   01 00 00 FF FF and four Adler bytes in front of zero padding, so it ends at the one position e in (offsets[f+1] - 16,
   offsets[f+1]] with out[e-9 .. e-5] = 01 00 00 FF FF (utils.png_stream_end).  A frame's bytes do not depend on n, on its place
   in the batch or on the stride.  offsets: uint64 [n+1], 8-byte aligned.  ws: device scratch of v3d_png_ws_bytes bytes (one
   fixed slot per scanline, row sizes and Adler sums), 16-byte aligned.  Enqueues four launches on `stream`, never synchronises,
   never allocates.  V3D_ERR_ARG: null pointer, n outside [1, 65535], W or H < 1, unknown fmt, frame_stride below a frame with
   n > 1, a misaligned ws, offsets or gray16 image; V3D_ERR_UNSUPPORTED: W > 8192 or H > 65535.  The three size functions return
   0 for arguments the entry refuses. */
#define V3D_PNG_GRAY16 0
#define V3D_PNG_BGR8   1
size_t v3d_png_stream_bound(int fmt, int W, int H);
size_t v3d_png_out_bytes(int fmt, int n, int W, int H);
size_t v3d_png_ws_bytes(int fmt, int n, int W, int H);
int v3d_png_deflate_batch(const void* img, size_t frame_stride /* bytes */, int fmt, int n, int W, int H,
                          uint8_t* out, uint64_t* offsets /* [n+1] */, void* ws, void* stream);

/* Frame matching (v3d_framematch.hip): a compact signature per luma plane and the exact integer correlation of signatures, for
   pairing SBS frames with 4K frames (framematch.py: the align CLI's --refine-video, the pipeline's --check-guide).  No call site
   in the reference (it trusts the rounded audio offset, align.py).  Bit-exact contract, all integers: tests/framematch_ref.py.
   Signature: frame f at gray + f*frame_stride (bytes), rows `pitch` bytes apart, only the W payload bytes of a row are read.
   The plane is cut into a grid of 64 x 36 cells RELATIVE to its size, so planes of different sizes give comparable cells:
     cell (cy, cx) = rows [floor(cy*H/36), floor((cy+1)*H/36)) x columns [floor(cx*W/64), floor((cx+1)*W/64));
     sig[cy*64 + cx] = floor(256 * S / c), S the sum of the cell's bytes, c its pixel count (the mean in 8.8 fixed point).
   Domain 64 <= W <= 8192, 36 <= H <= 8192 (else V3D_ERR_UNSUPPORTED): then 1 <= c <= 128 * 228, 256 * 255 * c < 2^31 and
   sig <= 65280.  sig_out dense uint16 [n][2304].  V3D_ERR_ARG: null pointer, n outside [1, 65535], pitch < W, frame_stride <
   H*pitch with n > 1.
   Scores of na x nb signatures, with G = 2304 and 64-bit integer sums (every term <= 2304^2 * 65280^2 < 2.3e16 < 2^63):
     num[i][j] = G * sum(a_i * b_j) - sum(a_i) * sum(b_j);   var_a[i] = G * sum(a_i^2) - (sum a_i)^2;   var_b likewise.
   The host forms the zero-mean normalised correlation Z = num / sqrt((double)var_a * (double)var_b); a pair with a zero variance
   (a flat frame) has none.  Z does not change under a gain or an offset of either plane.  V3D_ERR_ARG: null pointer, na or nb
   outside [1, 4096].  Both entries enqueue one launch on `stream`, never synchronise, never allocate, take device pointers only
   and write nothing outside their outputs. */
#define V3D_SIG_GW 64
#define V3D_SIG_GH 36
#define V3D_SIG_CELLS 2304
int v3d_frame_signature_batch(const uint8_t* gray, int n, int W, int H, int pitch, size_t frame_stride,
                              uint16_t* sig_out /* dense [n][2304] */, void* stream);
int v3d_signature_scores(const uint16_t* sig_a, int na, const uint16_t* sig_b, int nb,
                         int64_t* num_out /* [na][nb] */, int64_t* var_a_out /* [na] */, int64_t* var_b_out /* [nb] */,
                         void* stream);

/* Stereo quality report (v3d_quality.hip): two opt-in measures that need no ground truth, on planes a depth pass already holds
   on the device (quality.py: --quality-report).  No call site in the reference.  Bit-exact contract, all integers:
   tests/quality_ref.py.
   Reprojection: frame f's grays at left_gray / right_gray + f*frame_stride (bytes), rows `pitch` bytes apart, only the W payload
   bytes of a row are read; its disparity at disp16 + f*disp_stride (elements), rows dense, 2-byte alignment only.  Per pixel
   (x, y) with d = disp16[y][x]:
     valid iff d >= 1 (any other int16 is invalid; d up to 32767 is legal); u = 16 x - d; the pixel is COMPARED iff valid and u >= 0;
     for a compared pixel i = u >> 4, f = u & 15, r16 = (16 - f) R[y][i] + f R[y][i+1] (d >= 1 gives i + 1 <= W - 1: no clamp);
     e = |16 L[y][x] - r16| (0 <= e <= 4080);  e0 = 16 |L[y][x] - R[y][x]| (the same pixel at disparity 0).
   Record of a frame, u64 [8]: 0 n_valid = #{d >= 1} over all pixels; then over the compared pixels 1 n_cmp = their number,
   2 sad = sum e, 3 ssd = sum e^2, 4 n_bad = #{e > 16 bad_thr}, 5 sad0 = sum e0, 6 ssd0 = sum e0^2, 7 n_bad0 = #{e0 > 16 bad_thr}.
   A frame's record does not depend on n, on its place in the batch or on the strides.  Headroom: e^2 <= 16 646 400, so a u32
   holds the ssd of at most 258 pixels (a lane sums at most 128 before widening); over 8192 x 65535 pixels every field stays
   below 2^53.  No floating point anywhere in this entry.
   Flicker: the buffers the temporal entries take -- depth f32 (frame u at depth + u*depth_stride elements) and gray u8 (frame u
   at gray + u*gray_stride bytes), rows dense, T >= 2.  d16 = v3d_d16_tap(D): rint(16 D), valid iff >= 1 (NaN, -inf and <= 0 are
   invalid), +inf and every value above 32767 count as 32767 (the temporal filters do not saturate: "Non-finite input" above).  Record of pair u (frames u and u+1), u64 [4]:
     0 luma_sad = sum_p |Y_{u+1} - Y_u| over all pixels (the sum v3d_temporal_cuts thresholds: the host applies the same cut rule);
     1 n_still = #{p: |Y_{u+1} - Y_u| <= still and both d16 valid};  2 flicker = sum over those of |d16_{u+1} - d16_u|;
     3 n_jump = #{those with |d16_{u+1} - d16_u| > jump16}.
   ws: device scratch of the entry's _ws_bytes (one partial record per workgroup), 16-byte aligned; out: 8-byte aligned.  Both
   entries enqueue two launches on `stream`, never synchronise, never allocate, use no atomics on global memory, and write nothing
   outside out and ws, which may hold anything on entry.  V3D_ERR_ARG: null pointer, n outside [1, 65535], T outside [2, 65535],
   W or H < 1, pitch < W, a stride below a frame with more than one frame, bad_thr or still outside [0, 255], jump16 outside
   [0, 32767], ws not 16-byte aligned, out not 8-byte aligned; V3D_ERR_UNSUPPORTED: W > 8192 or H > 65535.  The _ws_bytes functions
   return 0 for arguments the entry refuses. */
#define V3D_QUALITY_REPROJ_FIELDS 8
#define V3D_QUALITY_FLICKER_FIELDS 4
size_t v3d_quality_reproj_ws_bytes(int n, int W, int H);
int v3d_quality_reproj_batch(const uint8_t* left_gray, const uint8_t* right_gray, int n, int W, int H, int pitch,
                             size_t frame_stride /* bytes */, const int16_t* disp16, size_t disp_stride /* elements */,
                             int bad_thr, uint64_t* out /* [n][8] */, void* ws, void* stream);
size_t v3d_quality_flicker_ws_bytes(int T, int W, int H);
int v3d_quality_flicker_batch(const float* depth, size_t depth_stride /* elements */, const uint8_t* gray,
                              size_t gray_stride /* bytes */, int T, int W, int H, int still, int jump16,
                              uint64_t* out /* [T-1][4] */, void* ws, void* stream);

/* Spatial registration (v3d_register.hip): fit the left eye of the SBS clip to the 4K frame with one affine map per axis and
   resample the low-res depth into the 4K frame's framing (register.py: the align CLI's --register-spatial, the upscale and
   pipeline CLIs' spatial block).  No call site in the reference.  Bit-exact contract, all integers, no floating point in any of
   the three entries: tests/register_ref.py.
   Profiles: frame f at gray + f*frame_stride (bytes), rows `pitch` bytes apart, only the W payload bytes of a row are read;
     col[f][x] = sum_y Y[y][x],  row[f][y] = sum_x Y[y][x]   (u32, dense [n][W] and [n][H]; 255 * 8192 < 2^21).
   Domain 1 <= W, H <= 8192 (above: V3D_ERR_UNSUPPORTED).  Two launches: the column sums of row bands go to ws (device scratch of
   v3d_plane_profiles_ws_bytes, 16-byte aligned, any content on entry), the second launch adds the bands; no atomics on global
   memory.  A frame's profiles do not depend on n, on its place in the batch or on the strides.  V3D_ERR_ARG: null pointer, n
   outside [1, 65535], W or H < 1, pitch < W, frame_stride < H*pitch with n > 1, ws not 16-byte aligned.
   Match: prof_a u32 dense [K][na] (source: the eye), prof_b u32 dense [K][nb] (target: the 4K frame), cand int64 [C][2] = (a, b)
   in Q16, out int64 [K][C][6].  Every floor and >> is the mathematical one, every number a 64-bit integer:
     target bin edges  t_j = floor(j * nb * 65536 / bins), j = 0 .. bins;   source edges  s_j = ((a * t_j) >> 16) + b;
     integral of a profile P of length n at p in [0, n * 65536]:  I(p) = pre[p >> 16] * 65536 + (p & 65535) * P[p >> 16],
       pre[i] = sum of P[k] over k < i, P[n] read as 0;   mean over [lo, hi) = floor((I(hi) - I(lo)) / (hi - lo));
     mb_j = mean of B over [t_j, t_j+1);  ma_j = mean of A over [s_j, s_j+1), valid iff 0 <= s_j and s_j+1 <= na * 65536;
     for j = 0 .. bins - 2 the pair is valid iff the bins j and j + 1 are: da = ma_j+1 - ma_j, db = mb_j+1 - mb_j;
     record = (n_pairs, sum da, sum db, sum da*db, sum da^2, sum db^2) over the valid pairs.
   Headroom: profile samples below 2^21 (what the profiles entry writes) give |d| < 2^21, products < 2^42 and sums over at most
   1023 pairs < 2^52; larger samples are legal memory-wise and wrap in the record.  The host forms the zero-mean normalised
   correlation from the six sums; it has none if a variance is 0 or n_pairs < bins / 2.  Candidate domain 2^12 <= a <= 2^20,
   |b| <= 2^29.  cand is device memory, which the entry cannot read without synchronising: a candidate outside the domain is
   refused in band, its record is (-1, 0, 0, 0, 0, 0) and nothing is computed for it; the binding refuses a host-side
   candidate list with ValueError before anything is enqueued.  ws: device scratch of v3d_profile_match_ws_bytes (the prefix
   sums of every frame's profiles, built by the first of the two launches), 16-byte aligned; cand and out 8-byte aligned.
   V3D_ERR_ARG: null pointer, K outside [1, 4096], C outside [1, 65535], na or nb < 1, bins outside [8, 1024], nb < bins, a
   misaligned pointer; V3D_ERR_UNSUPPORTED: na or nb > 8192.
   Warp: frame f at src + f*src_stride (elements), rows dense, 2-byte alignment only (odd widths and odd element offsets are
   legal); out dense u16 [n][Ho][Wo].  Per output pixel (x, y): u = ax * x + bx, v = ay * y + by, Q16 source-index coordinates;
     out = fill  if u is outside [0, (Ws - 1) * 65536] or v outside [0, (Hs - 1) * 65536];  else with
     i0 = u >> 16, i1 = min(i0 + 1, Ws - 1), fx = (u >> 8) & 255, j0, j1, fy likewise from v,
     out = ((256 - fy) * ((256 - fx) * s[j0][i0] + fx * s[j0][i1]) + fy * ((256 - fx) * s[j1][i0] + fx * s[j1][i1]) + 32768) >> 16
   (at most 65535 * 65536 + 32768 < 2^32).  The identity (65536, 0, 65536, 0) with Wo = Ws, Ho = Hs is a bit copy.  One launch.
   V3D_ERR_ARG: null pointer, n outside [1, 65535], a size < 1, src_stride < Ws*Hs with n > 1, ax or ay outside [2^12, 2^20],
   |bx| or |by| > 2^40, out overlapping src; V3D_ERR_UNSUPPORTED: Ws or Wo > 8192, Hs or Ho > 65535.
   All three entries enqueue on `stream`, never synchronise, never allocate, take device pointers only and write nothing outside
   their outputs and workspaces; a refused call enqueues nothing; the _ws_bytes functions return 0 for arguments their entry
   refuses. */
#define V3D_MATCH_FIELDS 6
size_t v3d_plane_profiles_ws_bytes(int n, int W, int H);
int v3d_plane_profiles_batch(const uint8_t* gray, int n, int W, int H, int pitch, size_t frame_stride /* bytes */,
                             uint32_t* col_out /* [n][W] */, uint32_t* row_out /* [n][H] */, void* ws, void* stream);
size_t v3d_profile_match_ws_bytes(int K, int na, int nb);
int v3d_profile_match_scores(const uint32_t* prof_a, int na, const uint32_t* prof_b, int nb, int K,
                             const int64_t* cand /* [C][2] */, int C, int bins, int64_t* out /* [K][C][6] */, void* ws, void* stream);
int v3d_warp_u16_batch(const uint16_t* src, int n, int Ws, int Hs, size_t src_stride /* elements */,
                       int64_t ax, int64_t bx, int64_t ay, int64_t by, uint16_t fill,
                       uint16_t* out /* [n][Ho][Wo] */, int Wo, int Ho, void* stream);

/* Colour matching (v3d_colour.hip): per-channel histogram transfer between two releases of a film (colour.py: the convert CLI's
   --match-colour, which corrects the SBS clip's right eye before v3d_render_stereo_source_batch samples it).  No call site in the
   reference.  Bit-exact contract, all integers, no floating point in any of the three entries: tests/colour_ref.py.
   Images: frame f at base + f*frame_stride (bytes), rows `pitch` bytes apart, pixel x of a row in its bytes 3x .. 3x+2 (channel
   c = byte 3x + c); the rectangle is the pixels [x0, x1) x [y0, y1).  No alignment is needed anywhere.
   Histogram: hist[f][c][v] = the number of pixels of frame f's rectangle whose byte c equals v; u32 dense [n][3][256], OVERWRITTEN
   (zeroing it is part of the entry: it may hold anything).  Two launches; sums of integers, so the order of the atomics cannot
   change a bit, and a frame's histogram does not depend on n, on its place in the batch, on the pitch or on the strides.  Memory
   contract: a row of the rectangle is read as the aligned 16-byte blocks that hold at least one of its bytes and nothing else is
   touched; bytes of such a block outside the rectangle are not counted.  V3D_ERR_ARG: null pointer, n outside [1, 65535], W or H
   outside [1, 65535] (an area stays below 2^32: no counter can wrap), pitch < 3W, frame_stride < H*pitch with n > 1, a rectangle
   that is empty or leaves the image.
   Table: table j is built from the frames [j*group, min(n, (j+1)*group)) of hist_src and hist_dst (both u32 [n][3][256], e.g. what
   the entry above wrote), summed per bin in 64 bits.  Per channel, with Cs and Cf the inclusive prefix sums of the two sums and
   Ns = Cs[255], Nf = Cf[255] the totals:
     lut[j][c][v] = the smallest u with Cf[u] * Ns >= Cs[v] * Nf,   the identity v if Ns == 0 or Nf == 0.
   The two products are compared exactly (totals reach 2^32 * 65535 < 2^48, products 2^96: 128-bit integers).  u exists
   (u = 255 satisfies it) and, Cs being non-decreasing, the table is monotone: v <= v' gives lut[v] <= lut[v'].  A level below
   the source's first occupied one has Cs = 0 and maps to 0.  lut u8 dense [ceil(n/group)][3][256].  One launch.  V3D_ERR_ARG: null
   pointer, n outside [1, 65535], group outside [1, n].
   Apply: for every pixel of the rectangle and channel c: dst = lut[f*lut_stride + 256 c + src]; lut_stride 0 = one table for all
   frames, else >= 768 bytes from one frame's table to the next.  dst has the source's size, its own pitch and frame stride.  Only
   the rectangle's bytes of src and of lut's tables are read, and no byte of dst outside the rectangle is written or read.  dst ==
   src with dst_pitch == pitch and (n == 1 or dst_stride == src_stride) is the in-place case; any other overlap of the two images'
   extents is refused.  One launch.  V3D_ERR_ARG: as the histogram's for both images, lut_stride in [1, 767], such an overlap.
   All three entries enqueue on `stream`, never synchronise, never allocate, read no environment and take device pointers only; a
   refused call enqueues nothing. */
int v3d_bgr_hist_batch(const uint8_t* bgr, size_t frame_stride /* bytes */, int n, int W, int H, int pitch,
                       int x0, int y0, int x1, int y1, uint32_t* hist /* [n][3][256] */, void* stream);
int v3d_colour_lut_batch(const uint32_t* hist_src, const uint32_t* hist_dst, int n, int group,
                         uint8_t* lut /* [ceil(n/group)][3][256] */, void* stream);
int v3d_bgr_lut_batch(const uint8_t* src, size_t src_stride /* bytes */, int n, int W, int H, int pitch,
                      int x0, int y0, int x1, int y1, const uint8_t* lut, int lut_stride /* bytes; 0: one table */,
                      uint8_t* dst, size_t dst_stride /* bytes */, int dst_pitch, void* stream);

/* Source-verified eye (v3d_verify.hip): a rendered eye checked, cell by cell and IN PLACE, against the stored eye of the SBS frame
   (the convert CLI's --verify-source, right after v3d_render_stereo_source_batch).  No call site in the reference.  Bit-exact
   contract, all integers: tests/verify_ref.py.
   Frame f's eye image E at eye_bgr + f*eye_stride (bytes), H rows `eye_pitch` bytes apart, W BGR pixels each: the right eye of a
   full-SBS output is base + 3W with pitch 6W, that of a full top-bottom output base + 3WH with pitch 3W.  The SBS frames, the map
   and P = P(eye)[y][t] are those of v3d_render_stereo_source_batch above: the same u, v, clamps, fx, fy and rounding.
   Cells: cx = (65536 + ax - 1) / ax by cy = (65536 + ay - 1) / ay targets (the targets one stored sample spans; 1 .. 16 each).
   Cell (p, r) holds the targets [p cx, min((p+1) cx, W)) x [r cy, min((r+1) cy, H)), npix of them.  Per cell and channel c:
     A_c = sum E, B_c = sum P over the cell;   m = |A_0 - B_0| + |A_1 - B_1| + |A_2 - B_2|;   replaced iff m > tau * npix.
   Every target of a replaced cell takes P; every other byte of E stays.  replaced[f] = the number of replaced cells of frame f,
   OVERWRITTEN (zeroing it is part of the entry: it may hold anything).  Sums are at most 255 * 256: int32 throughout.
   Memory contract: E is read at its rows' payload bytes only (3W per row) and written at the bytes of replaced cells only; the
   SBS rows are read at the payload bytes of the sampled eye's half only; neither needs any alignment.  No value outside a cell's
   own targets reaches its decision.  Two launches, no allocation, no synchronisation.
   V3D_ERR_ARG: null pointer; n, W or H < 1; eye_pitch < 3W; eye_stride < H*eye_pitch with n > 1; Ws odd or < 2; Hs < 1;
   pitch < 3 Ws; sbs_stride < Hs*pitch with n > 1; eye not 0 or 1; ax or ay outside [2^12, 2^20]; |bx| or |by| above 2^40; tau
   outside [0, 765] (765 = 3 * 255 can never be passed: nothing is replaced).  V3D_ERR_UNSUPPORTED: W > 8192 or Ws/2 > 8192, looked
   at after every V3D_ERR_ARG.  A refused call enqueues nothing. */
int v3d_verify_eye_source_batch(uint8_t* eye_bgr, size_t eye_stride /* bytes */, int eye_pitch /* bytes */, int n, int W, int H,
                                const uint8_t* sbs_bgr, size_t sbs_stride /* bytes */, int Ws, int Hs, int pitch, int eye /* 0 | 1 */,
                                int64_t ax, int64_t bx, int64_t ay, int64_t by, int tau,
                                uint32_t* replaced /* [n], overwritten */, void* stream);

/* Rendered-eye fidelity (v3d_fidelity.hip): a rendered eye MEASURED against the stored eye of the SBS frame (the convert CLI's
   --fidelity-report).  No call site in the reference.  Bit-exact contract, all integers: tests/fidelity_ref.py.
   The eye image E, the SBS frames, the map and P = P(eye)[y][t] are exactly those of v3d_verify_eye_source_batch above: the same
   u, v, clamps, fx, fy and rounding, the same addressing of an eye inside a full-SBS or full top-bottom output.  Both images are
   read only.
   Cells as in the verify entry: cx = (65536 + ax - 1) / ax by cy = (65536 + ay - 1) / ay targets, ncx = ceil(W / cx) by
   ncy = ceil(H / cy) of them, ragged last cells of npix targets.  Per cell and channel c (0 = B): A_c = sum E, B_c = sum P,
     a_c = (2 A_c + npix) / (2 npix),  b_c = (2 B_c + npix) / (2 npix)        (the cell means, u8; / floors).
   Colour record over all cells: n_cells = ncx ncy;  sad = sum_cells sum_c |a_c - b_c|;  ssd = sum sum (a_c - b_c)^2;
     n_bad = #{cells: sum_c |a_c - b_c| > bad_thr}.
   Luma of a cell: Ya = (9798 a_2 + 19235 a_1 + 3735 a_0 + 16384) >> 15, Yb likewise from b.
   SSIM (the x264 / ffmpeg form) over windows of 8 x 8 cells at stride 4: window (i, j) covers the cells [4i, 4i+8) x [4j, 4j+8)
   for every i, j with 4i + 8 <= ncx and 4j + 8 <= ncy (n_win of them, possibly 0).  Per window
     s1 = sum Ya, s2 = sum Yb, ss = sum (Ya^2 + Yb^2), s12 = sum Ya Yb;  vars = 64 ss - s1^2 - s2^2;  covar = 64 s12 - s1 s2;
     C1 = 416, C2 = 235963;  A = 2 s1 s2 + C1, B = s1^2 + s2^2 + C1, C = 2 covar + C2, D = vars + C2   (A <= B, |C| <= D, all
     below 2^31);  q1 = floor(A 2^20 / B), q2 = floor(|C| 2^20 / D);  Q = sign(C) ((q1 q2) >> 20), in [-2^20, 2^20].
   out row of frame f, int64 [V3D_FIDELITY_FIELDS]: n_cells, sad, ssd, n_bad, n_win, ssim_q20 = sum Q; OVERWRITTEN.  A frame's
   record does not depend on n, on its place in the batch, on pitches or on strides.
   Memory contract: E is read at its rows' payload bytes only (3W per row), the SBS rows at the payload bytes of the sampled eye's
   half only; neither needs any alignment.  ws: device scratch of v3d_eye_fidelity_ws_bytes, 16-byte aligned, any content on
   entry; out: 8-byte aligned.  Nothing outside out and ws is written.  At most three launches, no allocation, no synchronisation,
   no atomics on global memory (per-workgroup partial sums in ws and a reducing launch).
   V3D_ERR_ARG and V3D_ERR_UNSUPPORTED: exactly those of v3d_verify_eye_source_batch, with bad_thr in [0, 765] in place of tau;
   also V3D_ERR_ARG for a null or misaligned ws or out.  _ws_bytes returns 0 for arguments the entry refuses.  A refused call
   enqueues nothing. */
#define V3D_FIDELITY_FIELDS 6
size_t v3d_eye_fidelity_ws_bytes(int n, int W, int H, int64_t ax, int64_t ay);
int v3d_eye_fidelity_batch(const uint8_t* eye_bgr, size_t eye_stride /* bytes */, int eye_pitch /* bytes */, int n, int W, int H,
                           const uint8_t* sbs_bgr, size_t sbs_stride /* bytes */, int Ws, int Hs, int pitch, int eye /* 0 | 1 */,
                           int64_t ax, int64_t bx, int64_t ay, int64_t by, int bad_thr,
                           int64_t* out /* [n][V3D_FIDELITY_FIELDS] */, void* ws, void* stream);

/* Source-fused eye (v3d_fuse.hip): the low band of a rendered eye taken from the stored eye of the SBS frame, the detail above the
   stored eye's resolution kept from the render, IN PLACE (the convert CLI's --fuse-source, after the render and the verification).
   No call site in the reference.  Bit-exact contract, all integers: tests/fuse_ref.py.
   The eye image E, the SBS frames, the map and P = P(eye)[y][t] are exactly those of v3d_verify_eye_source_batch above: the same
   u, v, clamps, fx, fy and rounding, the same addressing of an eye inside a full-SBS or full top-bottom output.
   Per axis (coefficient a, offset b, Nd targets, Ns samples): q(t) = clamp(a t + b, 0, (Ns - 1) << 16) in 64 bits,
   near(t) = (q + 32768) >> 16, lo = near(0), hi = near(Nd - 1); i0 = q >> 16, i1 = min(i0 + 1, Ns - 1), f = (q >> 8) & 255 as in P.
   With a <= 65536 near never steps by more than 1: every sample of [lo, hi] owns at least one target.
   Means plane, for j in [jlo, jhi], i in [ilo, ihi] and channel c:  A = sum of E[y][t][c] over the targets with near_y(y) = j and
   near_x(t) = i, N their number (64-bit sums: under the clamps a first or last sample may own any share of the image);
     M[j][i][c] = (2 A + N) / (2 N)        (/ floors).
   Low band: LP[y][t][c] = P's bilinear formula ((...) + 32768) >> 16 with the same fx, fy over M in place of the stored eye, the
   tap indices clamped once more to the populated range: clamp(i0, ilo, ihi), clamp(i1, ilo, ihi), and likewise for j.
   Result: E[y][t][c] = clamp(E - LP + P, 0, 255).  Every payload byte of E is written; nothing else outside ws is.
   Memory contract: E is read and written at its rows' payload bytes only (3W per row, any pitch, any byte offset), the SBS rows
   are read at the payload bytes of the sampled eye's half only; neither needs any alignment.  ws: device scratch of
   v3d_fuse_eye_source_ws_bytes(n, Ws, Hs) = n * Hs * (Ws/2) * 3 bytes rounded up to 16 (0 for n < 1, Ws odd or < 2, Hs < 1 or
   Ws/2 > 8192), 16-byte aligned, any content on entry: it holds M, of which only the populated range is written and read.  Two
   launches (the means of the whole eye, then the result: a single launch would read targets another workgroup has written
   already), no allocation, no synchronisation.
   V3D_ERR_ARG: everything v3d_verify_eye_source_batch refuses for the same arguments; a null ws or one that is not 16-byte
   aligned.  V3D_ERR_UNSUPPORTED, looked at after every V3D_ERR_ARG: W > 8192 or Ws/2 > 8192; ax or ay above 65536 (the stored
   eye is finer than the frame: a sample could own no target, and fusing has nothing to add).  A refused call enqueues nothing. */
size_t v3d_fuse_eye_source_ws_bytes(int n, int Ws, int Hs);
int v3d_fuse_eye_source_batch(uint8_t* eye_bgr, size_t eye_stride /* bytes */, int eye_pitch /* bytes */, int n, int W, int H,
                              const uint8_t* sbs_bgr, size_t sbs_stride /* bytes */, int Ws, int Hs, int pitch, int eye /* 0 | 1 */,
                              int64_t ax, int64_t bx, int64_t ay, int64_t by, void* ws, void* stream);

const char* v3d_last_error(void);
const char* v3d_version(void);

#ifdef __cplusplus
}
#endif
#endif
