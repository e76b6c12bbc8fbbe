// v3d_sgbm.hip -- semi-global block matching for gfx950 (MI355X), D = 64, blockSize = 5: the handle and the C-ABI.
//
// Replaces cv2.StereoSGBM_create(...).compute(left_gray, right_gray) as invoked at
// reference depth.py:315-325, 341 (OpenCV MODE_SGBM 5-path default, MODE_HH 8-path optional).
// The kernels live in one file per stage (map, volume layout and stage entry points: v3d_sgbm_internal.h).
#include "v3d_sgbm_internal.h"
#include <string.h>

static const char* const g_stage_names[V3D_NSTAGE] = { "prefilter", "cost", "chain_v2", "chain_d1", "chain_d3", "chain_h0",
    "chain_v2r", "chain_d1r", "chain_d3r", "chain_h4_wta", "lrcheck", "median", "speckles" };

extern "C" void v3d_sgbm_default_params(v3d_sgbm_params* p)
{
    p->minDisparity = 0; p->numDisparities = 64; p->blockSize = 5; p->P1 = 8 * 3 * 25; p->P2 = 32 * 3 * 25;
    p->disp12MaxDiff = 1; p->preFilterCap = 0; p->uniquenessRatio = 10; p->speckleWindowSize = 100;
    p->speckleRange = 32; p->mode = V3D_MODE_SGBM;
}

template <typename T> static int ws_alloc(T** p, size_t n, size_t* total)
{
    const size_t b = ((n * sizeof(T)) + 255) & ~(size_t)255;
    V3D_HIP_CHECK(hipMalloc((void**)p, b));
    *total += b;
    return V3D_OK;
}

static void vdd_size_launches(v3d_sgbm* h)
{
    h->vdd_mf4 = sgbm_vdd_frames_per_launch(h, 4, h->maxW - V3D_D);
    h->vdd_mf8 = sgbm_vdd_frames_per_launch(h, 8, h->maxW - V3D_D);
}

// Tuning switches of a handle (A/B work, tests, tools): the defaults are the measured best, nothing here changes results.
// X(key, field of the handle, the values `value` may take, what it does)
#define V3D_SGBM_OPTIONS(X) \
    X("lockstep", vdd_mode, value == 0 || value == 1, "top-down paths in one co-resident lock-step pass (k_vdd) / 0: one launch per direction (k_chain); reads back 0 where a frame's strips cannot be co-resident") \
    X("hfused", hfused, value == 0 || value == 1, "both horizontal paths + WTA in one launch (k_hfused) / 0: two k_chain launches") \
    X("chain_dpl", dpl, value == 4 || value == 8, "disparities per lane in k_chain and k_hfused") \
    X("hsplit", hsplit, value == 0 || value == 1, "1: k_hfused's left-to-right scan as its own launch (measured: no gain; kept for A/B)") \
    X("vdd_dpl", vdd_dpl, value == 0 || value == 4 || value == 8, "k_vdd strip mapping (0 = choose per call from the batch size)") \
    X("cost_band", cost_band, value >= 8 && value <= 65536, "rows per k_cost workgroup") \
    X("cost_xcd", cost_xcd, value == 0 || value == 1, "XCD-contiguous workgroup order of k_cost") \
    X("vdd_xcd", vdd_xcd, value == 0 || value == 1, "XCD-contiguous workgroup order of k_vdd; speed only, so a launch of more frames than are co-resident ignores it (forward progress there rests on dispatch order = strip order)") \
    X("hf_xcd", hf_xcd, value == 0 || value == 1, "XCD-contiguous workgroup order of k_hfused") \
    X("hf_persist", hf_persist, value == 0 || value == 1, "k_hfused as the resident number of waves drawing row groups from a ticket counter / 0: one wave per row group") \
    X("lrm_tiles", lrm_tiles, value == 0 || value == 1, "L-R check + median as a row march over full-width bands / 1: as 128 x 16 tiles (also the form for W > 4096)") \
    X("reserve_cus", reserve_cus, value >= 0 && value <= h->ncu, "CUs other streams keep busy while a lock-step pass runs (shrinks the frames per launch)") \
    X("vdd_spin_limit", vdd_spin_limit, value >= -1, "poll rounds a lane may wait in a lock-step pass (0 = 64 per row + 4096; -1 = test hook: every workgroup reports a time-out, which drives the guard / V3D_ERR_LOCKSTEP path deterministically)") \
    X("vdd_launch_frames", vdd_launch_frames, value >= 0, "frames per lock-step launch (0 = from the occupancy query); larger than the chip holds is safe, slow: such a launch runs in plain blockIdx order whatever vdd_xcd says") \
    X("vdd_seq", vdd_seq, value >= 1 && value <= 0xFFFFF, "test hook: the 20-bit sequence number the next lock-step launch carries (reaches the wrap and its granule sweep without 2^20 launches); reads back the number the next launch will carry")

extern "C" int v3d_sgbm_set_option(v3d_sgbm* h, const char* key, int value)
{
    if (!h || !key) { v3d_set_error("null argument"); return V3D_ERR_ARG; }
#define X(name, field, ok, doc)                                                                                         \
    if (!strcmp(key, name)) {                                                                                           \
        if (!(ok)) { v3d_set_error("option %s: value %d out of range", key, value); return V3D_ERR_ARG; }               \
        h->field = value;                                                                                               \
        vdd_size_launches(h);                                   /* reserve_cus; the other keys leave the sizes as they are */ \
        return V3D_OK;                                                                                                  \
    }
    V3D_SGBM_OPTIONS(X)
#undef X
    v3d_set_error("unknown option %s", key);
    return V3D_ERR_ARG;
}
extern "C" int v3d_sgbm_get_option(const v3d_sgbm* h, const char* key, int* value)
{
    if (!h || !key || !value) { v3d_set_error("null argument"); return V3D_ERR_ARG; }
    if (!strcmp(key, "lockstep")) { *value = vdd_usable(h) ? 1 : 0; return V3D_OK; }       // what a compute call will do, not the stored flag
    if (!strcmp(key, "vdd_seq")) { const int s = (int)(h->vdd_seq & 0xFFFFFu); *value = s ? s : 1; return V3D_OK; }   // the counter runs on; 0 is skipped (launch_vdd)
#define X(name, field, ok, doc) if (!strcmp(key, name)) { *value = h->field; return V3D_OK; }
    V3D_SGBM_OPTIONS(X)
#undef X
    if (!strcmp(key, "vdd_frames_per_launch_dpl4")) { *value = h->vdd_mf4; return V3D_OK; }   // read-only: the co-residency bounds in force
    if (!strcmp(key, "vdd_frames_per_launch_dpl8")) { *value = h->vdd_mf8; return V3D_OK; }
    v3d_set_error("unknown option %s", key);
    return V3D_ERR_ARG;
}

extern "C" int v3d_sgbm_create(const v3d_sgbm_params* prm, int device, int maxW, int maxH, int maxB, v3d_sgbm** out)
{
    if (!prm || !out) { v3d_set_error("null argument"); return V3D_ERR_ARG; }
    // minDisparity m in [-64, 0]: the left record of cost column x1 is read at image column x1 + 64 + m, which must stay inside
    // the image for every x1 in [0, W - 64); outside that range the cost region would have to shrink
    if (prm->minDisparity < -V3D_D || prm->minDisparity > 0 || prm->numDisparities != V3D_D || prm->blockSize != 5) {
        v3d_set_error("this build supports -64 <= minDisparity <= 0, numDisparities=64, blockSize=5 (got %d, %d, %d)",
                      prm->minDisparity, prm->numDisparities, prm->blockSize);
        return V3D_ERR_UNSUPPORTED;
    }
    if (prm->mode != V3D_MODE_SGBM && prm->mode != V3D_MODE_HH) { v3d_set_error("unsupported mode %d", prm->mode); return V3D_ERR_UNSUPPORTED; }
    if (maxW <= V3D_D + 4 || maxH < 1 || maxB < 1) { v3d_set_error("bad geometry %dx%d batch %d", maxW, maxH, maxB); return V3D_ERR_ARG; }
    // one frame's cost volume must stay below 2 GiB: k_cost addresses it through a range-checked buffer whose
    // out-of-range marker is bit 31 of the byte offset
    if ((size_t)maxW * maxH * V3D_D >= ((size_t)1 << 30)) { v3d_set_error("frame too large for 31-bit volume byte offsets"); return V3D_ERR_UNSUPPORTED; }
    V3D_HIP_CHECK(hipSetDevice(device));
    v3d_sgbm* h = new v3d_sgbm();                         // every tuning field at its default (v3d_sgbm_internal.h)
    h->prm = *prm; h->device = device; h->maxW = maxW; h->maxH = maxH; h->maxB = maxB;
    h->P1 = prm->P1 > 0 ? prm->P1 : 2;
    h->P2 = prm->P2 > 0 ? prm->P2 : 5; if (h->P2 < h->P1 + 1) h->P2 = h->P1 + 1;
    h->ftzero = (prm->preFilterCap > 15 ? prm->preFilterCap : 15) | 1;
    h->uniq = prm->uniquenessRatio >= 0 ? prm->uniquenessRatio : 10;
    // uniquenessRatio > 100 makes 100 - uniq negative: OpenCV then rejects a pixel with min S == 0 as soon as a far
    // disparity has S > 0, which wta_pixel's threshold form (T1 = 0 there) cannot express.  Meaningless as a ratio: refused.
    if (h->uniq > 100) {
        const int uq = h->uniq; delete h;
        v3d_set_error("uniquenessRatio=%d is outside the accepted range (need uniquenessRatio <= 100; negative means 10)", uq);
        return V3D_ERR_UNSUPPORTED;
    }
    if (h->uniq < 100) v3d_t1_magic(100 - h->uniq, &h->t1_mul, &h->t1_shift);
    h->d12 = prm->disp12MaxDiff > 0 ? prm->disp12MaxDiff : 1;
    // int16 headroom of the packed recurrence: L <= C <= P2 + 25*(2*ftzero + 63) and delta = min L + P2
    // must stay below 32767 (OpenCV forms delta in int32; the reference's P2 = 2400 is far inside)
    if (2 * h->P2 + 25 * (2 * h->ftzero + 63) >= 32767 || h->ftzero > 31) {   // ftzero <= 31: BT bytes add pairwise without carry in k_cost
        const int p2 = h->P2; delete h;
        v3d_set_error("P2=%d / preFilterCap exceed the int16 range of the packed SGM recurrence (need 2*P2 + 25*(2*ftzero+63) < 32767)", p2);
        return V3D_ERR_UNSUPPORTED;
    }
    const size_t px = (size_t)maxW * maxH * maxB, vol = vol_frame(maxH, maxW - V3D_D) * maxB;
    int rc = 0;
    rc |= ws_alloc(&h->rec, px, &h->bytes);
    rc |= ws_alloc(&h->C, c_frame(maxH, maxW - V3D_D) * maxB, &h->bytes);   rc |= ws_alloc(&h->S, vol, &h->bytes);
    rc |= ws_alloc(&h->wta, px, &h->bytes); rc |= ws_alloc(&h->labels, px * 3, &h->bytes);
    {   // checkpoints: per frame, per wave (DPL rows), per K-pixel block: 64 lanes x (DPL/2 + 1) dwords
        const int W1m = maxW - V3D_D;
        const size_t c4 = (size_t)v3d_cdiv(maxH, 4) * v3d_cdiv(W1m, 16) * 64 * 3, c8 = (size_t)v3d_cdiv(maxH, 8) * v3d_cdiv(W1m, 8) * 64 * 5;
        rc |= ws_alloc(&h->ckpt, (c4 > c8 ? c4 : c8) * maxB, &h->bytes);
    }
    {
        const int nstrips_max = v3d_cdiv(maxW - V3D_D, 64);          // granule ring sized for the narrower strips
        const size_t ng = (size_t)maxB * nstrips_max * 2 * VDD_RING * VDD_GRAN;
        rc |= ws_alloc(&h->gran, ng, &h->bytes); h->gran_bytes = ng * sizeof(unsigned long long);
        rc |= ws_alloc(&h->vdd_err, 64, &h->bytes);
        h->hf_ticket = h->vdd_err ? h->vdd_err + 32 : nullptr;       // k_hfused's ticket counter shares the small allocation
        if (!rc) { (void)hipMemset(h->gran, 0, ng * sizeof(unsigned long long)); (void)hipMemset(h->vdd_err, 0, 64 * sizeof(int)); }
        if (!rc && hipHostMalloc((void**)&h->err_host, 64, hipHostMallocDefault) != hipSuccess) { h->err_host = nullptr; rc = 1; }
        if (h->err_host) *h->err_host = 0;
        if (!rc && hipEventCreateWithFlags(&h->vdd_done_ev, hipEventDisableTiming) != hipSuccess) { h->vdd_done_ev = nullptr; rc = 1; }
        // all strips of a launch must be resident together: bound frames per launch by the occupancy query
        int b4 = 0, b8 = 0, ncu = 0;
        sgbm_vdd_occupancy(&b4, &b8);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
        h->vdd_occ4 = b4 > 2 ? 2 : b4; h->vdd_occ8 = b8 > 2 ? 2 : b8; h->ncu = ncu;
        vdd_size_launches(h);
    }
    if (rc) { v3d_sgbm_destroy(h); return V3D_ERR_HIP; }
    *out = h;
    return V3D_OK;
}

extern "C" void v3d_sgbm_destroy(v3d_sgbm* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    void* ptrs[] = { h->rec, h->C, h->S, h->wta, h->labels, h->ckpt, h->gran, h->vdd_err };
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (h->err_host) (void)hipHostFree(h->err_host);
    if (h->vdd_done_ev) (void)hipEventDestroy(h->vdd_done_ev);
    for (hipEvent_t e : h->prof_ev) (void)hipEventDestroy(e);
    delete h;
}

extern "C" size_t v3d_sgbm_workspace_bytes(const v3d_sgbm* h) { return h ? h->bytes : 0; }

static int check_geometry(const v3d_sgbm* h, int n, int W, int H, int pitch)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    if (n < 1 || n > h->maxB || W > h->maxW || H > h->maxH || (size_t)W * H > (size_t)h->maxW * h->maxH) {
        v3d_set_error("frame %dx%d x%d exceeds the handle's workspace (%dx%d x%d)", W, H, n, h->maxW, h->maxH, h->maxB);
        return V3D_ERR_ARG;
    }
    if (W <= V3D_D + 4 || H < 1 || pitch < W) { v3d_set_error("bad frame geometry W=%d H=%d pitch=%d (need W > 68)", W, H, pitch); return V3D_ERR_ARG; }
    return V3D_OK;
}

// A lock-step pass of an earlier call timed out (k_vdd_guard raised the host flag): that call's output was
// invalidated on the device, and the handle refuses further work until the host has reacted --
// v3d_sgbm_set_lockstep(h, 0 or 1) clears the state.  No synchronisation here: one read of pinned memory.
static int lockstep_state(const v3d_sgbm* h)
{
    if (h->err_host && *(volatile int*)h->err_host != 0) {
        v3d_set_error("a lock-step SGM pass of an earlier call timed out (%d workgroups): its output was set to INVALID; "
                      "call v3d_sgbm_set_lockstep(h, 0) and recompute", *(volatile int*)h->err_host);
        return V3D_ERR_LOCKSTEP;
    }
    return V3D_OK;
}

// stages: 1 = cost volume, 2 = aggregation + WTA + LR check (raw), 3 = median + speckles (final)
static int run_sgbm(v3d_sgbm* h, const uint8_t* left, const uint8_t* right, int n, int W, int H, int pitch,
                    size_t frame_stride, int16_t* out, int last_stage, hipStream_t st)
{
    int rc = check_geometry(h, n, W, H, pitch);
    if (rc) return rc;
    if (!left || !right || !out) { v3d_set_error("null image pointer"); return V3D_ERR_ARG; }
    if (n > 1 && frame_stride < (size_t)H * pitch) { v3d_set_error("frame stride %zu below the frame size %zu (H * pitch)", frame_stride, (size_t)H * pitch); return V3D_ERR_ARG; }
    if ((rc = lockstep_state(h)) != V3D_OK) return rc;
    const size_t npx = (size_t)W * H * n;
    bool lockstep_ran = false;

    if ((rc = sgbm_cost_volume(h, left, right, n, W, H, pitch, frame_stride, st)) != V3D_OK) return rc;
    prof_mark(h, ST_V2, st);
    if (last_stage == 1) return V3D_OK;
    if ((rc = sgbm_aggregate_wta(h, n, W, H, st, &lockstep_ran)) != V3D_OK) return rc;
    prof_mark(h, ST_LRCHECK, st);
    if (last_stage == 2) {
        if ((rc = sgbm_lrcheck_median(h, n, W, H, out, false, st)) != V3D_OK) return rc;
        if (lockstep_ran && (rc = sgbm_lockstep_guard(h, out, npx, st)) != V3D_OK) return rc;
        prof_mark(h, ST_MEDIAN, st);
        return V3D_OK;
    }
    prof_mark(h, ST_MEDIAN, st);
    if ((rc = sgbm_lrcheck_median(h, n, W, H, out, true, st)) != V3D_OK) return rc;
    prof_mark(h, ST_SPECKLE, st);
    if ((rc = sgbm_speckles(h, out, n, W, H, st)) != V3D_OK) return rc;
    if (lockstep_ran && (rc = sgbm_lockstep_guard(h, out, npx, st)) != V3D_OK) return rc;
    prof_mark(h, V3D_NSTAGE, st);
    if (h->prof_on && h->prof_calls < V3D_PROF_MAX_CALLS) h->prof_calls++;
    return V3D_OK;
}

// ---- per-stage timing: enable (resets the counters), run any number of compute calls, synchronise the
// stream, then read.  Events are recorded on the caller's stream between the stage launches. ----
// synchronises the device and returns how many k_vdd workgroups gave up waiting for a neighbour (0 = healthy)
extern "C" int v3d_sgbm_sync_errors(v3d_sgbm* h)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    int e = 0;
    V3D_HIP_CHECK(hipSetDevice(h->device));
    V3D_HIP_CHECK(hipDeviceSynchronize());
    V3D_HIP_CHECK(hipMemcpy(&e, h->vdd_err, sizeof(int), hipMemcpyDeviceToHost));
    return e;
}

extern "C" int v3d_sgbm_set_lockstep(v3d_sgbm* h, int enable)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    V3D_HIP_CHECK(hipSetDevice(h->device));
    V3D_HIP_CHECK(hipDeviceSynchronize());
    V3D_HIP_CHECK(hipMemset(h->vdd_err, 0, sizeof(int)));
    *(volatile int*)h->err_host = 0;
    h->vdd_mode = enable ? 1 : 0;
    return V3D_OK;
}

// non-blocking: > 0 once k_vdd_guard of a finished call has seen time-outs (the flag travels with the call's last launch)
extern "C" int v3d_sgbm_poll_errors(const v3d_sgbm* h)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    return h->err_host ? *(volatile int*)h->err_host : 0;
}

// make `stream` wait until the lock-step pass of the most recent compute call on this handle has finished (no-op if
// none ran).  For hosts that run a collective on a side stream: RCCL workgroups that land on a CU take a slot the
// co-resident pass was sized with, so order the collective BEHIND the pass (it then overlaps the horizontal pass,
// the post-filters and the upscale instead) and the next compute call behind the collective.
extern "C" int v3d_sgbm_stream_wait_lockstep(v3d_sgbm* h, void* stream)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    if (!h->vdd_ev_recorded) return V3D_OK;
    V3D_HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, h->vdd_done_ev, 0));
    return V3D_OK;
}

extern "C" int v3d_sgbm_profile(v3d_sgbm* h, int enable)
{
    if (!h) { v3d_set_error("null handle"); return V3D_ERR_ARG; }
    if (enable && h->prof_ev.empty()) {
        V3D_HIP_CHECK(hipSetDevice(h->device));
        h->prof_ev.resize((size_t)V3D_PROF_MAX_CALLS * (V3D_NSTAGE + 1));
        for (auto& e : h->prof_ev) V3D_HIP_CHECK(hipEventCreate(&e));
    }
    h->prof_on = enable != 0;
    h->prof_calls = 0;
    return V3D_OK;
}
extern "C" int v3d_sgbm_profile_stage_count(void) { return V3D_NSTAGE; }
extern "C" const char* v3d_sgbm_profile_stage_name(int i) { return (i >= 0 && i < V3D_NSTAGE) ? g_stage_names[i] : ""; }
// total_ms[i] = summed duration of stage i over the recorded calls; returns the number of calls (or < 0)
extern "C" int v3d_sgbm_profile_read(v3d_sgbm* h, double* total_ms, int n)
{
    if (!h || !total_ms || n < V3D_NSTAGE) { v3d_set_error("bad argument"); return V3D_ERR_ARG; }
    for (int i = 0; i < V3D_NSTAGE; i++) total_ms[i] = 0.0;
    for (int c = 0; c < h->prof_calls; c++)
        for (int i = 0; i < V3D_NSTAGE; i++) {
            float ms = 0.f;
            const hipEvent_t a = h->prof_ev[(size_t)c * (V3D_NSTAGE + 1) + i], b = h->prof_ev[(size_t)c * (V3D_NSTAGE + 1) + i + 1];
            V3D_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
            total_ms[i] += ms;
        }
    return h->prof_calls;
}

extern "C" int v3d_sgbm_compute(v3d_sgbm* h, const uint8_t* l, const uint8_t* r, int W, int H, int pitch, int16_t* out, void* stream)
{
    return run_sgbm(h, l, r, 1, W, H, pitch, 0, out, 3, (hipStream_t)stream);
}
extern "C" int v3d_sgbm_compute_batch(v3d_sgbm* h, const uint8_t* l, const uint8_t* r, int n, int W, int H, int pitch,
                                      size_t frame_stride, int16_t* out, void* stream)
{
    return run_sgbm(h, l, r, n, W, H, pitch, frame_stride, out, 3, (hipStream_t)stream);
}
extern "C" int v3d_sgbm_debug_cost_volume(v3d_sgbm* h, const uint8_t* l, const uint8_t* r, int W, int H, int pitch, int16_t* C_out, void* stream)
{
    int16_t dummy;
    int rc = run_sgbm(h, l, r, 1, W, H, pitch, 0, &dummy, 1, (hipStream_t)stream);
    if (rc) return rc;
    return sgbm_export_cost(h, W, H, C_out, (hipStream_t)stream);
}
extern "C" int v3d_sgbm_debug_raw(v3d_sgbm* h, const uint8_t* l, const uint8_t* r, int W, int H, int pitch, int16_t* out, int16_t* S_out, void* stream)
{
    int rc = run_sgbm(h, l, r, 1, W, H, pitch, 0, out, 2, (hipStream_t)stream);
    if (rc) return rc;
    // S holds sum of all directions but the last (the last one is only ever formed on-chip)
    if (S_out) V3D_HIP_CHECK(hipMemcpyAsync(S_out, h->S, (size_t)(W - V3D_D) * H * V3D_D * sizeof(int16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return V3D_OK;
}
