"""ctypes binding of libv3d_hip.so (include/v3d_hip.h) over PyTorch-ROCm device buffers.

PyTorch is plumbing only: it owns device memory and streams; every kernel on the hot path is
in libv3d_hip.so.  There is NO CPU fallback: if the library is missing or a call fails this
module raises.
"""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libv3d_hip.so")
_lib = None

ERR_LOCKSTEP = -4      # V3D_ERR_LOCKSTEP
STEREO_FULL_SBS, STEREO_HALF_SBS = 0, 1      # V3D_STEREO_FULL_SBS / V3D_STEREO_HALF_SBS
STEREO_MAX_WIDTH = 8192
# V3D_PACK_*: the packings of v3d_render_stereo_packed_batch (0 and 1 are the two layouts above)
(STEREO_PACK_FULL_SBS, STEREO_PACK_HALF_SBS, STEREO_PACK_FULL_TB, STEREO_PACK_HALF_TB, STEREO_PACK_ROWS,
 STEREO_PACK_ANAGLYPH_COLOUR, STEREO_PACK_ANAGLYPH_DUBOIS) = range(7)


class NativeError(RuntimeError):
    pass


class LockstepTimeout(NativeError):
    """a lock-step SGM pass timed out on an over-subscribed GPU; the call's output was invalidated on the device.
    React with StereoSGBM.set_lockstep(False) and recompute (include/v3d_hip.h)."""


class SgbmParams(C.Structure):
    """mirror of v3d_sgbm_params == keyword arguments of cv2.StereoSGBM_create (depth.py:315-325)"""
    _fields_ = [(n, C.c_int) for n in (
        "minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff",
        "preFilterCap", "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")]


vp, ci, sz, fl, cs, i64 = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_char_p, C.c_int64
# every symbol include/v3d_hip.h declares, once: name -> (restype, argtypes).  lib() binds exactly these rows and
# tests/test_abi.py holds each of them to the header's declaration
SIGNATURES = {
    "v3d_sgbm_default_params": (None, [C.POINTER(SgbmParams)]),
    "v3d_sgbm_create": (ci, [C.POINTER(SgbmParams), ci, ci, ci, ci, C.POINTER(vp)]),
    "v3d_sgbm_destroy": (None, [vp]),
    "v3d_sgbm_workspace_bytes": (sz, [vp]),
    "v3d_sgbm_compute": (ci, [vp, vp, vp, ci, ci, ci, vp, vp]),
    "v3d_sgbm_compute_batch": (ci, [vp, vp, vp, ci, ci, ci, ci, sz, vp, vp]),
    "v3d_sgbm_sync_errors": (ci, [vp]),
    "v3d_sgbm_poll_errors": (ci, [vp]),
    "v3d_sgbm_set_lockstep": (ci, [vp, ci]),
    "v3d_sgbm_stream_wait_lockstep": (ci, [vp, vp]),
    "v3d_sgbm_set_option": (ci, [vp, cs, ci]),
    "v3d_sgbm_get_option": (ci, [vp, cs, C.POINTER(ci)]),
    "v3d_set_option": (ci, [cs, ci]),
    "v3d_get_option": (ci, [cs, C.POINTER(ci)]),
    "v3d_sgbm_profile": (ci, [vp, ci]),
    "v3d_sgbm_profile_stage_count": (ci, []),
    "v3d_sgbm_profile_stage_name": (cs, [ci]),
    "v3d_sgbm_profile_read": (ci, [vp, C.POINTER(C.c_double), ci]),
    "v3d_sgbm_debug_cost_volume": (ci, [vp, vp, vp, ci, ci, ci, vp, vp]),
    "v3d_sgbm_debug_raw": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp]),
    "v3d_median3x3_i16": (ci, [vp, ci, ci, vp, vp]),
    "v3d_filter_speckles": (ci, [vp, ci, ci, ci, ci, ci, vp, vp]),
    "v3d_sbs_to_gray": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_sbs_to_gray_batch": (ci, [vp, ci, ci, ci, ci, sz, ci, vp, vp, vp]),
    "v3d_split_sbs": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_tb_to_gray": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_tb_to_gray_batch": (ci, [vp, ci, ci, ci, ci, sz, ci, vp, vp, vp]),
    "v3d_split_tb": (ci, [vp, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_disp_to_depth": (ci, [vp, sz, vp, vp]),
    "v3d_depth_to_u16": (ci, [vp, sz, vp, vp, vp]),
    "v3d_depth_to_u16_batch": (ci, [vp, ci, sz, sz, vp, vp, vp]),
    "v3d_round_to_u16": (ci, [vp, sz, vp, vp]),
    "v3d_mono_blend_ws_bytes": (sz, [ci]),
    "v3d_mono_blend": (ci, [vp, ci, ci, vp, ci, ci, fl, fl, vp, vp, vp]),
    "v3d_mono_blend_batch": (ci, [vp, ci, ci, ci, vp, ci, ci, sz, fl, fl, vp, vp, vp]),
    "v3d_guided_upscale_ws_bytes": (sz, [ci, ci]),
    "v3d_guided_upscale": (ci, [vp, ci, ci, vp, ci, ci, ci, fl, vp, vp, vp]),
    "v3d_guided_upscale_batch": (ci, [vp, ci, ci, sz, vp, ci, ci, sz, ci, ci, fl, vp, vp, vp]),
    "v3d_guided_upscale_disp16_batch": (ci, [vp, ci, ci, sz, vp, ci, ci, sz, ci, ci, fl, vp, vp, vp]),
    "v3d_guided_upscale_u16_batch": (ci, [vp, ci, ci, sz, vp, ci, ci, sz, ci, ci, fl, vp, vp, vp]),
    "v3d_bgr_to_gray": (ci, [vp, sz, vp, vp]),
    "v3d_corr_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_corr_lookup": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_xcorr_ws_bytes": (sz, [ci, ci]),
    "v3d_xcorr": (ci, [vp, ci, vp, ci, vp, vp, vp]),
    "v3d_align_audio": (ci, [vp, ci, vp, ci, vp, vp, vp]),
    "v3d_render_stereo_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "v3d_render_stereo_subpixel_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "v3d_render_stereo_packed_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "v3d_render_stereo_source_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, sz, ci, ci, ci, ci, i64, i64, i64, i64,
                                            vp, vp]),
    "v3d_temporal_cuts": (ci, [vp, sz, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_depth_minmax_batch": (ci, [vp, ci, sz, sz, vp, vp]),
    "v3d_temporal_range": (ci, [vp, vp, ci, ci, ci, ci, vp, vp]),
    "v3d_temporal_filter_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_temporal_motion": (ci, [vp, sz, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
    "v3d_temporal_filter_mc_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
    "v3d_depth_to_u16_range_batch": (ci, [vp, ci, sz, sz, vp, vp, vp]),
    "v3d_depth_robust_minmax_ws_bytes": (sz, [ci]),
    "v3d_depth_robust_minmax_batch": (ci, [vp, ci, sz, sz, ci, vp, vp, vp]),
    "v3d_fill_holes_ws_bytes": (sz, [ci, ci]),
    "v3d_fill_holes_disp16_batch": (ci, [vp, sz, ci, ci, ci, vp, vp, vp]),
    "v3d_png_stream_bound": (sz, [ci, ci, ci]),
    "v3d_png_out_bytes": (sz, [ci, ci, ci, ci]),
    "v3d_png_ws_bytes": (sz, [ci, ci, ci, ci]),
    "v3d_png_deflate_batch": (ci, [vp, sz, ci, ci, ci, ci, vp, vp, vp, vp]),
    "v3d_frame_signature_batch": (ci, [vp, ci, ci, ci, ci, sz, vp, vp]),
    "v3d_signature_scores": (ci, [vp, ci, vp, ci, vp, vp, vp, vp]),
    "v3d_quality_reproj_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_quality_reproj_batch": (ci, [vp, vp, ci, ci, ci, ci, sz, vp, sz, ci, vp, vp, vp]),
    "v3d_quality_flicker_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_quality_flicker_batch": (ci, [vp, sz, vp, sz, ci, ci, ci, ci, ci, vp, vp, vp]),
    "v3d_plane_profiles_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_plane_profiles_batch": (ci, [vp, ci, ci, ci, ci, sz, vp, vp, vp, vp]),
    "v3d_profile_match_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_profile_match_scores": (ci, [vp, ci, vp, ci, ci, vp, ci, ci, vp, vp, vp]),
    "v3d_warp_u16_batch": (ci, [vp, ci, ci, ci, sz, i64, i64, i64, i64, C.c_uint16, vp, ci, ci, vp]),
    "v3d_bgr_hist_batch": (ci, [vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
    "v3d_colour_lut_batch": (ci, [vp, vp, ci, ci, vp, vp]),
    "v3d_bgr_lut_batch": (ci, [vp, sz, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, sz, ci, vp]),
    "v3d_verify_eye_source_batch": (ci, [vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, ci, ci, i64, i64, i64, i64, ci, vp, vp]),
    "v3d_eye_fidelity_ws_bytes": (sz, [ci, ci, ci, i64, i64]),
    "v3d_eye_fidelity_batch": (ci, [vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, ci, ci, i64, i64, i64, i64, ci, vp, vp, vp]),
    "v3d_fuse_eye_source_ws_bytes": (sz, [ci, ci, ci]),
    "v3d_fuse_eye_source_batch": (ci, [vp, sz, ci, ci, ci, ci, vp, sz, ci, ci, ci, ci, i64, i64, i64, i64, vp, vp]),
    "v3d_last_error": (cs, []),
    "v3d_version": (cs, []),
}
EXPORTS = tuple(SIGNATURES)
del vp, ci, sz, fl, cs, i64


def lib_path():
    return _LIB_PATH


def use_library(path):
    """load another build of libv3d_hip.so instead of the in-tree one (development tools only -- tools/envopts.py; the
    product never calls this and reads no environment variable).  Must come before the first lib()."""
    global _LIB_PATH
    if _lib is not None:
        raise NativeError("use_library() after the library was loaded")
    _LIB_PATH = os.path.abspath(path)


def lib():
    """load libv3d_hip.so (built by `make -C video-3d-pipeline_amd/csrc` or __graft_entry__.build())"""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise NativeError(
                f"{_LIB_PATH} not found: build it with `make -C video-3d-pipeline_amd/csrc` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        cls = LockstepTimeout if rc == ERR_LOCKSTEP else NativeError
        raise cls(f"{what} failed (rc={rc}): {lib().v3d_last_error().decode()}")


def set_option(key, value):
    """library-wide tuning switch (v3d_set_option): gf_band1, gf_band2, gf_tiled, gf_fused, corr_gather"""
    _check(lib().v3d_set_option(key.encode(), int(value)), f"v3d_set_option({key})")


def get_option(key):
    """current value of a library-wide switch (v3d_get_option)"""
    v = C.c_int()
    _check(lib().v3d_get_option(key.encode(), C.byref(v)), f"v3d_get_option({key})")
    return v.value


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(entry, device, *args):
    """the one way an entry that takes a stream is launched: with `device` (the tensors' own) current, on that device's
    current stream, and an error raised under the entry's own name.  args: ready ctypes values, every one but the stream"""
    with torch.cuda.device(device):
        rc = getattr(lib(), entry)(*args, _stream())
    _check(rc, entry)


def _out(out, shape, dtype, device):
    """a caller's result tensor checked against `shape`, or a fresh one"""
    shape = tuple(shape)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != shape:
        raise NativeError(f"out: expected shape {shape}, got {tuple(out.shape)}")
    return out


def _scratch(need, device, cache=None, key=None):
    """uint8 device scratch of `need` bytes (a number, or a callable asked only when something is allocated), never fewer than
    16.  With a cache, allocated once per (key, device) and kept; else from the caching allocator, nothing in the steady state"""
    key = (key, device.index)
    ws = cache.get(key) if cache is not None else None
    if ws is None:
        ws = torch.empty(max(int(need() if callable(need) else need), 16), dtype=torch.uint8, device=device)
        if cache is not None:
            cache[key] = ws
    return ws


def _dev(t, dtype, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeError(f"{what}: expected a device tensor")
    if t.dtype != dtype or not t.is_contiguous():
        raise NativeError(f"{what}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
    return C.c_void_p(t.data_ptr())


def resolve_device(device=None):
    """one place that turns None / 'cuda' / 'cuda:i' / i / torch.device into a device WITH an index: a bare 'cuda'
    means the CURRENT device (torch.cuda.set_device), never silently GPU 0"""
    if isinstance(device, int):
        return torch.device("cuda", device)
    d = torch.device("cuda") if device is None else torch.device(device)
    if d.type != "cuda":
        raise NativeError(f"device {device!r}: this build only has the MI355X (HIP) path")
    return d if d.index is not None else torch.device("cuda", torch.cuda.current_device())


def default_params(**kw):
    p = SgbmParams()
    lib().v3d_sgbm_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown StereoSGBM parameter {k!r}")
        setattr(p, k, int(v))
    return p


class StereoSGBM:
    """GPU stand-in for the object cv2.StereoSGBM_create returns (depth.py:315-325); `.compute`
    mirrors depth.py:341 on device tensors."""

    def __init__(self, max_width, max_height, max_batch=1, device=None, options=None, **params):
        """device: None = the current device (what torch.cuda.set_device / LOCAL_RANK selected), an index, or a
        torch.device; options: {key: int} for v3d_sgbm_set_option (tuning switches, results never change)"""
        self.params = default_params(**params)
        self.max_width, self.max_height, self.max_batch = int(max_width), int(max_height), int(max_batch)
        self.device = resolve_device(device)
        h = C.c_void_p()
        _check(lib().v3d_sgbm_create(C.byref(self.params), self.device.index, self.max_width, self.max_height,
                                     self.max_batch, C.byref(h)), "v3d_sgbm_create")
        self._h = h
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, key, value):
        _check(lib().v3d_sgbm_set_option(self._h, key.encode(), int(value)), f"v3d_sgbm_set_option({key})")

    def get_option(self, key):
        v = C.c_int()
        _check(lib().v3d_sgbm_get_option(self._h, key.encode(), C.byref(v)), f"v3d_sgbm_get_option({key})")
        return v.value

    def poll_errors(self):
        """non-blocking: lock-step time-outs reported so far by finished calls (0 = healthy)"""
        return int(lib().v3d_sgbm_poll_errors(self._h))

    def stream_wait_lockstep(self, stream):
        """make the torch stream `stream` wait for the lock-step pass of the latest compute() (order collectives behind it)"""
        _check(lib().v3d_sgbm_stream_wait_lockstep(self._h, C.c_void_p(stream.cuda_stream)), "v3d_sgbm_stream_wait_lockstep")

    def close(self):
        if getattr(self, "_h", None):
            lib().v3d_sgbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # interpreter shutdown: module globals may already be gone
            pass

    @property
    def workspace_bytes(self):
        return int(lib().v3d_sgbm_workspace_bytes(self._h))

    def compute(self, left, right, out=None):
        """left/right: uint8 [H,W] or [N,H,W] device tensors -> int16 disparity x16 (-16 invalid)"""
        batched = left.dim() == 3
        l3 = left if batched else left[None]
        r3 = right if batched else right[None]
        n, H, W = l3.shape
        if r3.shape != l3.shape:
            raise NativeError("left/right shape mismatch")
        if out is None:
            out = torch.empty((n, H, W), dtype=torch.int16, device=l3.device)
        o3 = out if out.dim() == 3 else out[None]
        _call("v3d_sgbm_compute_batch", self.device, self._h, _dev(l3, torch.uint8, "left"), _dev(r3, torch.uint8, "right"),
              n, W, H, W, H * W, _dev(o3, torch.int16, "out"))
        return out if batched else o3[0]

    def sync_errors(self):
        """device-synchronise; number of lock-step (k_vdd) workgroups that timed out on a neighbour (0 = healthy)"""
        return int(lib().v3d_sgbm_sync_errors(self._h))

    def set_lockstep(self, enable: bool):
        """switch the co-resident lock-step pass on/off for later compute() calls (off = one launch per direction);
        synchronises and clears the time-out counter"""
        _check(lib().v3d_sgbm_set_lockstep(self._h, int(bool(enable))), "v3d_sgbm_set_lockstep")

    def profile(self, enable=True):
        """per-stage HIP-event timing on the current stream: enable, run compute(), synchronize, read_profile()"""
        _check(lib().v3d_sgbm_profile(self._h, int(bool(enable))), "v3d_sgbm_profile")

    def read_profile(self):
        """-> (calls, {stage: total_ms}) ; the stream must be synchronised first"""
        n = lib().v3d_sgbm_profile_stage_count()
        buf = (C.c_double * n)()
        calls = lib().v3d_sgbm_profile_read(self._h, buf, n)
        if calls < 0:
            _check(calls, "v3d_sgbm_profile_read")
        return calls, {lib().v3d_sgbm_profile_stage_name(i).decode(): buf[i] for i in range(n)}

    def debug_cost_volume(self, left, right):
        H, W = left.shape
        out = torch.empty((H, W - 64, 64), dtype=torch.int16, device=left.device)
        _call("v3d_sgbm_debug_cost_volume", self.device, self._h, _dev(left, torch.uint8, "left"), _dev(right, torch.uint8, "right"),
              W, H, W, _dev(out, torch.int16, "C"))
        return out

    def debug_raw(self, left, right, want_S=False):
        H, W = left.shape
        out = torch.empty((H, W), dtype=torch.int16, device=left.device)
        S = torch.empty((H, W - 64, 64), dtype=torch.int16, device=left.device) if want_S else None
        _call("v3d_sgbm_debug_raw", self.device, self._h, _dev(left, torch.uint8, "left"), _dev(right, torch.uint8, "right"),
              W, H, W, _dev(out, torch.int16, "disp"), _dev(S, torch.int16, "S") if want_S else None)
        return (out, S) if want_S else out


def median3x3(img):
    H, W = img.shape
    out = torch.empty_like(img)
    _call("v3d_median3x3_i16", img.device, _dev(img, torch.int16, "img"), W, H, _dev(out, torch.int16, "out"))
    return out


def filter_speckles(img, new_val=-16, max_size=100, max_diff=512):
    H, W = img.shape
    out = img.clone()
    ws = torch.empty(3 * H * W, dtype=torch.int32, device=img.device)
    _call("v3d_filter_speckles", img.device, _dev(out, torch.int16, "img"), W, H, new_val, max_size, max_diff,
          _dev(ws, torch.int32, "ws"))
    return out


def sbs_to_gray(sbs, unsqueeze=True):
    """sbs: uint8 [H,W,3] BGR device tensor -> (left_gray, right_gray) uint8 [H, W or W/2]"""
    H, W, ch = sbs.shape
    if ch != 3:
        raise NativeError("expected HxWx3")
    if W % 2:
        raise ValueError("SBS frame width must be even")
    ow = W if unsqueeze else W // 2
    L = torch.empty((H, ow), dtype=torch.uint8, device=sbs.device)
    R = torch.empty_like(L)
    _call("v3d_sbs_to_gray", sbs.device, _dev(sbs, torch.uint8, "sbs"), W, H, W * 3, int(bool(unsqueeze)),
          _dev(L, torch.uint8, "L"), _dev(R, torch.uint8, "R"))
    return L, R


def sbs_to_gray_batch(sbs, unsqueeze=True, out=None):
    """sbs: uint8 [N,H,W,3] -> (left, right) uint8 [N,H,outW], one launch"""
    n, H, W, ch = sbs.shape
    if W % 2:
        raise ValueError("SBS frame width must be even")
    ow = W if unsqueeze else W // 2
    if out is None:
        out = (torch.empty((n, H, ow), dtype=torch.uint8, device=sbs.device), torch.empty((n, H, ow), dtype=torch.uint8, device=sbs.device))
    _call("v3d_sbs_to_gray_batch", sbs.device, _dev(sbs, torch.uint8, "sbs"), n, W, H, W * 3, H * W * 3, int(bool(unsqueeze)),
          _dev(out[0], torch.uint8, "L"), _dev(out[1], torch.uint8, "R"))
    return out


def split_sbs(sbs, unsqueeze=True):
    H, W, ch = sbs.shape
    if W % 2:
        raise ValueError("SBS frame width must be even")
    ow = W if unsqueeze else W // 2
    L = torch.empty((H, ow, 3), dtype=torch.uint8, device=sbs.device)
    R = torch.empty_like(L)
    _call("v3d_split_sbs", sbs.device, _dev(sbs, torch.uint8, "sbs"), W, H, W * 3, int(bool(unsqueeze)),
          _dev(L, torch.uint8, "L"), _dev(R, torch.uint8, "R"))
    return L, R


def _tb_out_height(H, unsqueeze):
    if H % 2 or H < 2:
        raise ValueError("top-bottom frame height must be even")
    return H if unsqueeze else H // 2


def tb_to_gray(tb, unsqueeze=True):
    """tb: uint8 [H,W,3] BGR device tensor, left eye on top -> (left_gray, right_gray) uint8 [H or H/2, W]"""
    H, W, ch = tb.shape
    if ch != 3:
        raise NativeError("expected HxWx3")
    L = torch.empty((_tb_out_height(H, unsqueeze), W), dtype=torch.uint8, device=tb.device)
    R = torch.empty_like(L)
    _call("v3d_tb_to_gray", tb.device, _dev(tb, torch.uint8, "tb"), W, H, W * 3, int(bool(unsqueeze)),
          _dev(L, torch.uint8, "L"), _dev(R, torch.uint8, "R"))
    return L, R


def tb_to_gray_batch(tb, unsqueeze=True, out=None):
    """tb: uint8 [N,H,W,3] -> (left, right) uint8 [N,outH,W], one launch"""
    n, H, W, ch = tb.shape
    oh = _tb_out_height(H, unsqueeze)
    if out is None:
        out = (torch.empty((n, oh, W), dtype=torch.uint8, device=tb.device), torch.empty((n, oh, W), dtype=torch.uint8, device=tb.device))
    _call("v3d_tb_to_gray_batch", tb.device, _dev(tb, torch.uint8, "tb"), n, W, H, W * 3, H * W * 3, int(bool(unsqueeze)),
          _dev(out[0], torch.uint8, "L"), _dev(out[1], torch.uint8, "R"))
    return out


def split_tb(tb, unsqueeze=True):
    H, W, ch = tb.shape
    L = torch.empty((_tb_out_height(H, unsqueeze), W, 3), dtype=torch.uint8, device=tb.device)
    R = torch.empty_like(L)
    _call("v3d_split_tb", tb.device, _dev(tb, torch.uint8, "tb"), W, H, W * 3, int(bool(unsqueeze)),
          _dev(L, torch.uint8, "L"), _dev(R, torch.uint8, "R"))
    return L, R


def bgr_to_gray(bgr, out=None):
    if out is None:
        out = torch.empty(bgr.shape[:-1], dtype=torch.uint8, device=bgr.device)
    if bgr.shape[-1] != 3 or tuple(out.shape) != tuple(bgr.shape[:-1]):
        raise NativeError(f"bgr_to_gray: shapes {tuple(bgr.shape)} -> {tuple(out.shape)}")
    _call("v3d_bgr_to_gray", bgr.device, _dev(bgr, torch.uint8, "bgr"), out.numel(), _dev(out, torch.uint8, "gray"))
    return out


def disp_to_depth(disp16, out=None):
    if out is None:
        out = torch.empty(disp16.shape, dtype=torch.float32, device=disp16.device)
    _call("v3d_disp_to_depth", disp16.device, _dev(disp16, torch.int16, "disp16"), disp16.numel(), _dev(out, torch.float32, "out"))
    return out


def mono_blend(disp16, mono, w_stereo=0.7, w_mono=0.3, out=None):
    """depth.py:344-374 on the device.  disp16: int16 [H,W] or [N,H,W]; mono: float32 [mh,mw] or [N,mh,mw] (any size)
    -> float32 depth like disp16's shape: clamp0(w_stereo * disp16/16 + w_mono * minmax64(resize(mono)))"""
    batched = disp16.dim() == 3
    d3 = disp16 if batched else disp16[None]
    m3 = mono if mono.dim() == 3 else mono[None]
    n, H, W = d3.shape
    if m3.shape[0] != n:
        raise NativeError(f"mono batch {m3.shape[0]} != disparity batch {n}")
    mh, mw = m3.shape[1:]
    if out is None:
        out = torch.empty(d3.shape, dtype=torch.float32, device=d3.device)
    o3 = out if out.dim() == 3 else out[None]
    ws = _scratch(lib().v3d_mono_blend_ws_bytes(n), d3.device)
    _call("v3d_mono_blend_batch", d3.device, _dev(d3, torch.int16, "disp16"), n, W, H, _dev(m3, torch.float32, "mono"), mw, mh,
          mh * mw, float(w_stereo), float(w_mono), _dev(o3, torch.float32, "out"), _dev(ws, torch.uint8, "ws"))
    return out if batched else o3[0]


def depth_to_u16(depth):
    out = torch.empty(depth.shape, dtype=torch.int16, device=depth.device)   # torch has no uint16 math; raw bits
    ws = torch.empty(2, dtype=torch.float32, device=depth.device)
    _call("v3d_depth_to_u16", depth.device, _dev(depth, torch.float32, "depth"), depth.numel(), _dev(out, torch.int16, "out"),
          _dev(ws, torch.float32, "ws"))
    return out


_mm_ws = {}


def depth_to_u16_batch(depth, out=None):
    """float32 [n,H,W] -> per-frame min-max normalised uint16 bit patterns in an int16 [n,H,W] tensor, one fixed launch set;
    frame f is bit-identical to depth_to_u16(depth[f]).  The min/max scratch is allocated once per (n, device)."""
    n = depth.shape[0]
    if out is None:
        out = torch.empty(depth.shape, dtype=torch.int16, device=depth.device)
    if depth.dim() != 3 or tuple(out.shape) != tuple(depth.shape):
        raise NativeError(f"depth_to_u16_batch: expected [n,H,W] in and out, got {tuple(depth.shape)} -> {tuple(out.shape)}")
    ws = _scratch(8 * n, depth.device, _mm_ws, n)                     # two floats per frame
    per = depth[0].numel() if n else 0
    _call("v3d_depth_to_u16_batch", depth.device, _dev(depth, torch.float32, "depth"), n, per, per, _dev(out, torch.int16, "out"),
          _dev(ws, torch.uint8, "ws"))
    return out


def round_to_u16(depth):
    """float32 device tensor -> clamp(rint(x), 0, 65535) as uint16 bit patterns in an int16 tensor (torch has no uint16 math)"""
    out = torch.empty(depth.shape, dtype=torch.int16, device=depth.device)
    _call("v3d_round_to_u16", depth.device, _dev(depth, torch.float32, "depth"), depth.numel(), _dev(out, torch.int16, "out"))
    return out


_gf_ws = {}


def _gf_scratch(Whi, Hhi, n, device):
    """the guided filter's workspace for n frames of Whi x Hhi, allocated once per geometry and device"""
    return _scratch(lambda: int(lib().v3d_guided_upscale_ws_bytes(Whi, Hhi)) * n, device, _gf_ws, (Whi, Hhi, n))


def guided_upscale(depth_lo, guide, r=8, eps=1e-3, out=None):
    """depth_lo f32 [Hlo,Wlo], guide u8 [Hhi,Whi] -> f32 [Hhi,Whi] (upscale.py's scale step, re-specified)"""
    Hlo, Wlo = depth_lo.shape
    Hhi, Whi = guide.shape
    if out is None:
        out = torch.empty((Hhi, Whi), dtype=torch.float32, device=guide.device)
    ws = _gf_scratch(Whi, Hhi, 1, guide.device)
    _call("v3d_guided_upscale", guide.device, _dev(depth_lo, torch.float32, "depth_lo"), Wlo, Hlo, _dev(guide, torch.uint8, "guide"),
          Whi, Hhi, int(r), float(eps), _dev(out, torch.float32, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def guided_upscale_batch(depth_lo, guide, r=8, eps=1e-3, out=None):
    """depth_lo [N,Hlo,Wlo] (contiguous): float32 depth, or the matcher's int16 disparity x16 (then `/16` and `<= 0 -> 0`
    of depth.py:341, 374 happen inside the filter's loads: same bits, no float plane); guide u8 [N,Hhi,Whi] (frames may be
    strided) -> f32 [N,Hhi,Whi], one launch.
    int16 domain: values up to 1821 (the matcher's never exceed 1023).  An exact 2x upscale with r <= 8 then takes the
    integer first stage, whose int32 window sums hold 289 * 255 * 16 * d < 2^31; larger values need set_option("gf_int1", 0)
    first (the f64 route takes the whole int16 range).  Nothing checks this on the device: a check would cost a sync."""
    n, Hlo, Wlo = depth_lo.shape
    _, Hhi, Whi = guide.shape
    if guide.stride(2) != 1 or guide.stride(1) != Whi:
        raise NativeError("guide frames must be dense HxW images")
    if out is None:
        out = torch.empty((n, Hhi, Whi), dtype=torch.float32, device=guide.device)
    ws = _gf_scratch(Whi, Hhi, n, guide.device)
    if guide.dtype != torch.uint8 or not guide.is_cuda:
        raise NativeError("guide: expected a uint8 device tensor")
    if depth_lo.dtype == torch.int16:
        entry, src = "v3d_guided_upscale_disp16_batch", _dev(depth_lo, torch.int16, "disp16")
    else:
        entry, src = "v3d_guided_upscale_batch", _dev(depth_lo, torch.float32, "depth_lo")
    _call(entry, guide.device, src, Wlo, Hlo, Hlo * Wlo, C.c_void_p(guide.data_ptr()), Whi, Hhi, guide.stride(0), n, int(r),
          float(eps), _dev(out, torch.float32, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def guided_upscale_u16_batch(depth_u16, guide, r=8, eps=1e-3, out=None):
    """depth_u16: the normalised 16-bit depth samples as an int16-viewed [N,Hlo,Wlo] tensor; guide u8 [N,Hhi,Whi] (frames may
    be strided) -> the 16-bit 4K samples, int16-viewed [N,Hhi,Whi], one launch.  Bit-identical to
    round_to_u16(guided_upscale_batch(u16 as float32)) on every route (include/v3d_hip.h)."""
    n, Hlo, Wlo = depth_u16.shape
    _, Hhi, Whi = guide.shape
    if guide.shape[0] != n:
        raise NativeError(f"guide batch {guide.shape[0]} != depth batch {n}")
    if guide.dtype != torch.uint8 or not guide.is_cuda:
        raise NativeError("guide: expected a uint8 device tensor")
    if guide.stride(2) != 1 or guide.stride(1) != Whi:
        raise NativeError("guide frames must be dense HxW images")
    out = _out(out, (n, Hhi, Whi), torch.int16, guide.device)
    ws = _gf_scratch(Whi, Hhi, n, guide.device)
    _call("v3d_guided_upscale_u16_batch", guide.device, _dev(depth_u16, torch.int16, "depth_u16"), Wlo, Hlo, Hlo * Wlo,
          C.c_void_p(guide.data_ptr()), Whi, Hhi, guide.stride(0), n, int(r), float(eps),
          _dev(out, torch.int16, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def corr_lookup(fl, fr, flow, groups=4, pattern=0):
    """fl, fr: bf16 [h,w,C]; flow f32 [2,h,w] -> f32 [groups*9,h,w]"""
    h, w, Cc = fl.shape
    out = torch.empty((groups * 9, h, w), dtype=torch.float32, device=fl.device)
    ws = _scratch(lib().v3d_corr_ws_bytes(Cc, h, w), fl.device)
    _call("v3d_corr_lookup", fl.device, _dev(fl, torch.bfloat16, "fl"), _dev(fr, torch.bfloat16, "fr"),
          _dev(flow, torch.float32, "flow"), Cc, h, w, groups, pattern, _dev(out, torch.float32, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def _xcorr_args(a1, a2, what):
    if a1.dim() != 1 or a2.dim() != 1:
        raise NativeError(f"{what}: expected 1-D tracks, got {tuple(a1.shape)} and {tuple(a2.shape)}")
    if a1.device != a2.device:
        raise NativeError(f"{what}: tracks on {a1.device} and {a2.device}")
    n1, n2 = a1.numel(), a2.numel()
    nbytes = int(lib().v3d_xcorr_ws_bytes(n1, n2)) if 1 <= n1 < 2 ** 31 and 1 <= n2 < 2 ** 31 else 0
    if nbytes == 0:
        raise NativeError(f"{what}: lengths {n1}, {n2} unsupported (need >= 1 and n1 + n2 - 1 <= 2^26)")
    ws = _scratch(nbytes, a1.device)
    return (_dev(a1, torch.float32, "a1"), n1, _dev(a2, torch.float32, "a2"), n2), ws


def xcorr(a1, a2):
    """float32 device tracks [n1], [n2] -> float32 [n1 + n2 - 1]: scipy.signal.correlate(a2, a1, 'full') of the raw
    tracks (index k = lag + n1 - 1), by FFT on the device (v3d_xcorr)"""
    args, ws = _xcorr_args(a1, a2, "xcorr")
    out = torch.empty(a1.numel() + a2.numel() - 1, dtype=torch.float32, device=a1.device)
    _call("v3d_xcorr", a1.device, *args, _dev(out, torch.float32, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def align_audio(a1, a2):
    """float32 device tracks -> float64 device tensor [lag, c(lag), strength, min(std1, std2)] (v3d_align_audio): the lag
    (in samples, a1[n] ~ a2[n + lag]) that maximises |c| of find_audio_offset's normalised tracks (utils.py:137-165)"""
    args, ws = _xcorr_args(a1, a2, "align_audio")
    out = torch.empty(4, dtype=torch.float64, device=a1.device)
    _call("v3d_align_audio", a1.device, *args, _dev(out, torch.float64, "result"), _dev(ws, torch.uint8, "ws"))
    return out


def stereo_gains(max_shift=48.0, convergence=0.5, eye_split=0.5):
    """user parameters of the DIBR step -> (gain_left, gain_right, conv), the integers v3d_render_stereo_batch takes:
    gain_left = floor(max_shift * eye_split * 256 + 0.5), gain_right = -floor(max_shift * (1 - eye_split) * 256 + 0.5),
    conv = floor(convergence * 65535 + 0.5).  max_shift: parallax in pixels between depth 65535 and depth 0 (>= 0, < 65536);
    convergence: the depth at the screen plane, eye_split: the left eye's share of the shift (both in [0, 1])."""
    import math
    vals = {"max_shift": max_shift, "convergence": convergence, "eye_split": eye_split}
    for k, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{k} must be a finite number, got {v!r}")
    if not 0 <= max_shift < 65536:
        raise ValueError(f"max_shift must be in [0, 65536) pixels, got {max_shift}")
    if not 0 <= convergence <= 1:
        raise ValueError(f"convergence must be in [0, 1], got {convergence}")
    if not 0 <= eye_split <= 1:
        raise ValueError(f"eye_split must be in [0, 1], got {eye_split}")
    gl = math.floor(max_shift * eye_split * 256 + 0.5)
    gr = -math.floor(max_shift * (1 - eye_split) * 256 + 0.5)
    conv = math.floor(convergence * 65535 + 0.5)
    if max(abs(gl), abs(gr)) >= 1 << 24:
        raise ValueError(f"max_shift {max_shift} gives a gain beyond 2^24")
    return gl, gr, conv


def _stereo_io(frames, depth_u16, out, out_size):
    """the checks both DIBR wrappers make -> (n, H, W, out).  out_size(W, H) -> (outW, outH) makes the wrapper's own argument
    checks, after those of the inputs and before that of out (allocated here if None)."""
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.dtype != torch.uint8 or not frames.is_cuda:
        raise NativeError(f"frames: expected a uint8 [n,H,W,3] device tensor, got {frames.dtype} {tuple(frames.shape)}")
    n, H, W, _ = frames.shape
    if frames.stride(3) != 1 or frames.stride(2) != 3 or frames.stride(1) != 3 * W:
        raise NativeError("frames: rows must be dense HxWx3 images (only the frame stride may differ)")
    if tuple(depth_u16.shape) != (n, H, W):
        raise NativeError(f"depth {tuple(depth_u16.shape)} does not match frames {tuple(frames.shape)}")
    oW, oH = out_size(W, H)
    return n, H, W, _out(out, (n, oH, oW, 3), torch.uint8, frames.device)


def render_stereo_batch(frames, depth_u16, gain_left, gain_right, convergence, layout=STEREO_FULL_SBS, out=None, subpixel=False):
    """DIBR (v3d_render_stereo_batch): frames u8 [n,H,W,3] BGR on the device (frames may be strided: rows dense), depth_u16 the
    u16 depth samples as an int16-viewed contiguous [n,H,W] tensor -> u8 [n,H,2W,3] (full SBS, left eye first) or [n,H,W,3]
    (half SBS).  Bit-exact contract: tests/stereo_ref.py.  subpixel: v3d_render_stereo_subpixel_batch instead, positions in
    1/16 px and colours interpolated along connected spans (contract: tests/stereo_sub_ref.py)."""
    def out_size(W, H):
        if layout not in (STEREO_FULL_SBS, STEREO_HALF_SBS):
            raise ValueError(f"layout must be {STEREO_FULL_SBS} (full SBS) or {STEREO_HALF_SBS} (half SBS), got {layout!r}")
        return (2 * W if layout == STEREO_FULL_SBS else W), H
    n, H, W, out = _stereo_io(frames, depth_u16, out, out_size)
    entry = "v3d_render_stereo_subpixel_batch" if subpixel else "v3d_render_stereo_batch"
    _call(entry, frames.device, C.c_void_p(frames.data_ptr()), frames.stride(0), _dev(depth_u16, torch.int16, "depth_u16"),
          H * W, n, W, H, int(gain_left), int(gain_right), int(convergence), int(layout), _dev(out, torch.uint8, "out"))
    return out


def stereo_output_size(packing, W, H):
    """(outW, outH) of a W x H frame rendered with packing code `packing` (STEREO_PACK_*): full SBS is twice as wide, full
    top-bottom twice as high, every other packing W x H.  ValueError for an unknown code, an odd W for half SBS, an odd H for
    half top-bottom."""
    if isinstance(packing, bool) or not isinstance(packing, (int, np.integer)) or not 0 <= packing <= STEREO_PACK_ANAGLYPH_DUBOIS:
        raise ValueError(f"packing must be one of 0 .. {STEREO_PACK_ANAGLYPH_DUBOIS} (STEREO_PACK_*), got {packing!r}")
    if packing == STEREO_PACK_HALF_SBS and W % 2:
        raise ValueError(f"half SBS needs an even width, got {W}")
    if packing == STEREO_PACK_HALF_TB and H % 2:
        raise ValueError(f"half top-bottom needs an even height, got {H}")
    return (2 * W if packing == STEREO_PACK_FULL_SBS else W), (2 * H if packing == STEREO_PACK_FULL_TB else H)


def render_stereo_packed_batch(frames, depth_u16, gain_left, gain_right, convergence, packing, out=None, subpixel=False):
    """DIBR with the eyes packed for the display (v3d_render_stereo_packed_batch): the inputs of render_stereo_batch ->
    u8 [n,outH,outW,3] (stereo_output_size): side by side, top-bottom, row-interleaved or a red-cyan anaglyph, in one launch.
    Bit-exact contract: tests/stereo_pack_ref.py.  subpixel: the eyes of the sub-pixel renderer."""
    def out_size(W, H):
        if not isinstance(subpixel, (bool, np.bool_)):
            raise ValueError(f"subpixel must be True or False, got {subpixel!r}")
        return stereo_output_size(packing, W, H)
    n, H, W, out = _stereo_io(frames, depth_u16, out, out_size)
    _call("v3d_render_stereo_packed_batch", frames.device, C.c_void_p(frames.data_ptr()), frames.stride(0),
          _dev(depth_u16, torch.int16, "depth_u16"), H * W, n, W, H, int(gain_left), int(gain_right), int(convergence),
          int(bool(subpixel)), int(packing), _dev(out, torch.uint8, "out"))
    return out


def render_stereo_source_batch(frames, depth_u16, gain_left, gain_right, convergence, packing, sbs, fill_eyes, ax, bx, ay, by,
                               out=None, subpixel=False):
    """render_stereo_packed_batch with the holes of the eyes named by fill_eyes (bit 0 left, bit 1 right) sampled from the stored
    eye of the SBS frames (v3d_render_stereo_source_batch): sbs u8 [n,Hs,Ws,3] BGR on the device (rows may be pitched, frames
    strided; None only with fill_eyes = 0), target (t, y) reads eye coordinates (ax t + bx, ay y + by) in Q16, clamped to the eye.
    Bit-exact contract: tests/stereo_source_ref.py."""
    def out_size(W, H):
        if not isinstance(subpixel, (bool, np.bool_)):
            raise ValueError(f"subpixel must be True or False, got {subpixel!r}")
        if isinstance(fill_eyes, bool) or not isinstance(fill_eyes, (int, np.integer)) or not 0 <= fill_eyes <= 3:
            raise ValueError(f"fill_eyes must be 0 .. 3 (bit 0: left eye, bit 1: right eye), got {fill_eyes!r}")
        return stereo_output_size(packing, W, H)
    n, H, W, out = _stereo_io(frames, depth_u16, out, out_size)
    if sbs is None:
        if fill_eyes:
            raise NativeError("sbs: fill_eyes != 0 needs the SBS frames")
        sp, ss, Ws, Hs, pitch = C.c_void_p(None), 6, 2, 1, 6     # the smallest legal geometry: the entry checks it all the same
    else:
        if not isinstance(sbs, torch.Tensor) or not sbs.is_cuda or sbs.dtype != torch.uint8 or sbs.dim() != 4 or sbs.shape[3] != 3:
            raise NativeError("sbs: expected a uint8 [n,Hs,Ws,3] device tensor")
        if sbs.shape[0] != n:
            raise NativeError(f"sbs holds {sbs.shape[0]} frames, frames {n}")
        if sbs.stride(3) != 1 or sbs.stride(2) != 3:
            raise NativeError("sbs: pixels must be dense BGR triples (only the row pitch and the frame stride may differ)")
        _, Hs, Ws, _ = sbs.shape
        sp, ss, pitch = C.c_void_p(sbs.data_ptr()), sbs.stride(0), sbs.stride(1) if Hs > 1 else 3 * Ws
    _call("v3d_render_stereo_source_batch", frames.device, C.c_void_p(frames.data_ptr()), frames.stride(0),
          _dev(depth_u16, torch.int16, "depth_u16"), H * W, n, W, H, int(gain_left), int(gain_right), int(convergence),
          int(bool(subpixel)), int(packing), sp, ss, int(Ws), int(Hs), int(pitch), int(fill_eyes), int(ax), int(bx), int(ay), int(by),
          _dev(out, torch.uint8, "out"))
    return out


TEMPORAL_MAX_RADIUS = 8


def _clip(t, dtype, what):
    """a [T,H,W] device tensor whose frames are dense HxW images (only the frame stride may differ) -> (pointer, frame stride)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 3:
        raise NativeError(f"{what}: expected a {dtype} [T,H,W] device tensor")
    T, H, W = t.shape
    if T < 1 or H < 1 or W < 1:
        raise NativeError(f"{what}: empty clip {tuple(t.shape)}")
    if t.stride(2) != 1 or t.stride(1) != W or (T > 1 and t.stride(0) < H * W):
        raise NativeError(f"{what}: frames must be dense HxW images (only the frame stride may differ)")
    return C.c_void_p(t.data_ptr()), (t.stride(0) if T > 1 else H * W)


def _temporal_window(T, t0, n, radius):
    n = T - t0 if n is None else n
    if not 0 <= radius <= TEMPORAL_MAX_RADIUS:
        raise ValueError(f"temporal radius must be in [0, {TEMPORAL_MAX_RADIUS}], got {radius}")
    if t0 < 0 or n < 1 or t0 + n > T:
        raise ValueError(f"targets {t0}..{t0 + n - 1} outside a buffer of {T} frames")
    return n


def temporal_cuts(gray, cut_threshold=20):
    """left gray u8 [T,H,W] -> u8 [T] scene-cut flags on the device (v3d_temporal_cuts): cut[u] = 1 iff the mean absolute
    luma difference between frames u-1 and u exceeds cut_threshold levels"""
    if not 0 <= cut_threshold <= 256:
        raise ValueError(f"cut threshold must be in [0, 256], got {cut_threshold}")
    g, gs = _clip(gray, torch.uint8, "gray")
    T, H, W = gray.shape
    ws = torch.empty(T, dtype=torch.int64, device=gray.device)
    out = torch.empty(T, dtype=torch.uint8, device=gray.device)
    _call("v3d_temporal_cuts", gray.device, g, gs, T, W, H, int(cut_threshold), _dev(ws, torch.int64, "ws"), _dev(out, torch.uint8, "cut"))
    return out


def depth_minmax_batch(depth):
    """float32 [T,H,W] -> float32 [T,2] on the device: each frame's min and max (v3d_depth_minmax_batch)"""
    d, ds = _clip(depth, torch.float32, "depth")
    T, H, W = depth.shape
    out = torch.empty((T, 2), dtype=torch.float32, device=depth.device)
    _call("v3d_depth_minmax_batch", depth.device, d, T, H * W, ds, _dev(out, torch.float32, "minmax"))
    return out


RANGE_Q_MIN, RANGE_Q_OFF = 5000, 10000


def depth_robust_minmax_batch(depth, q):
    """float32 [T,H,W] -> float32 [T,2] on the device: each frame's min and its robust white point, the q/10000 quantile of the
    valid fixed-point disparities (v3d_depth_robust_minmax_batch; contract: tests/range_ref.py).  The histogram workspace is
    a torch allocation from the caching allocator: nothing is allocated in the steady state."""
    if isinstance(q, bool) or int(q) != q or not RANGE_Q_MIN <= q <= RANGE_Q_OFF:
        raise ValueError(f"range quantile must be an integer in [{RANGE_Q_MIN}, {RANGE_Q_OFF}], got {q!r}")
    d, ds = _clip(depth, torch.float32, "depth")
    T, H, W = depth.shape
    ws = _scratch(lib().v3d_depth_robust_minmax_ws_bytes(T), depth.device)
    out = torch.empty((T, 2), dtype=torch.float32, device=depth.device)
    _call("v3d_depth_robust_minmax_batch", depth.device, d, T, H * W, ds, int(q), _dev(ws, torch.uint8, "ws"),
          _dev(out, torch.float32, "minmax"))
    return out


def temporal_range(minmax, cut, radius, t0=0, n=None):
    """per-frame (min, max) [T,2] + cut flags [T] -> the clip-stable (lo, hi) [n,2] of targets t0 .. t0+n-1 (v3d_temporal_range)"""
    T = minmax.shape[0]
    n = _temporal_window(T, t0, n, radius)
    if tuple(minmax.shape) != (T, 2) or tuple(cut.shape) != (T,):
        raise NativeError(f"temporal_range: minmax {tuple(minmax.shape)} / cut {tuple(cut.shape)} do not describe one clip")
    out = torch.empty((n, 2), dtype=torch.float32, device=minmax.device)
    _call("v3d_temporal_range", minmax.device, _dev(minmax, torch.float32, "minmax"), _dev(cut, torch.uint8, "cut"), T, t0, n,
          int(radius), _dev(out, torch.float32, "lohi"))
    return out


def _temporal_filter_args(depth, gray, radius, tau, cut, t0, n, out, fields=None):
    """what both temporal filters check and prepare: the two clips, cut (and the two motion fields, if given) against them, the
    window, tau and `out` -> ((depth pointer, stride, gray pointer, stride, T, W, H, n), out)"""
    d, ds = _clip(depth, torch.float32, "depth")
    g, gs = _clip(gray, torch.uint8, "gray")
    T, H, W = depth.shape
    if tuple(gray.shape) != (T, H, W) or tuple(cut.shape) != (T,):
        raise NativeError(f"gray {tuple(gray.shape)} / cut {tuple(cut.shape)} do not match depth {tuple(depth.shape)}")
    fshape = (T, -(-H // 16), -(-W // 16), 2)
    if fields is not None and any(tuple(f.shape) != fshape for f in fields):
        raise NativeError(f"fields {tuple(fields[0].shape)} / {tuple(fields[1].shape)}: expected {fshape}")
    n = _temporal_window(T, t0, n, radius)
    if not 1 <= tau <= 255:
        raise ValueError(f"temporal tau must be in [1, 255], got {tau}")
    return (d, ds, g, gs, T, W, H, n), _out(out, (n, H, W), torch.float32, depth.device)


def temporal_filter_batch(depth, gray, radius, tau, cut, fill=True, t0=0, n=None, out=None):
    """the temporal filter (v3d_temporal_filter_batch): depth f32 [T,H,W] (<= 0 invalid), left gray u8 [T,H,W], cut u8 [T] ->
    filtered depth f32 [n,H,W] of targets t0 .. t0+n-1.  Bit-exact contract: tests/temporal_ref.py."""
    (d, ds, g, gs, T, W, H, n), out = _temporal_filter_args(depth, gray, radius, tau, cut, t0, n, out)
    _call("v3d_temporal_filter_batch", depth.device, d, ds, g, gs, T, W, H, t0, n, int(radius), int(tau), int(bool(fill)),
          _dev(cut, torch.uint8, "cut"), _dev(out, torch.float32, "out"))
    return out


TEMPORAL_MAX_SEARCH = 32


def temporal_motion(gray, search, cut_threshold=20):
    """left gray u8 [T,H,W] -> (forward fields, backward fields) int16 [T,BH,BW,2] as (dx,dy) per 16x16 block, the compensated
    residual int64 [T] and the scene-cut flags u8 [T] it gives, all on the device (v3d_temporal_motion; `search` = S pixels per
    frame step, 1..32).  Bit-exact contract: tests/temporal_mc_ref.py."""
    if isinstance(search, bool) or int(search) != search or not 1 <= search <= TEMPORAL_MAX_SEARCH:
        raise ValueError(f"motion search radius must be an integer in [1, {TEMPORAL_MAX_SEARCH}], got {search!r}")
    if not 0 <= cut_threshold <= 256:
        raise ValueError(f"cut threshold must be in [0, 256], got {cut_threshold}")
    g, gs = _clip(gray, torch.uint8, "gray")
    T, H, W = gray.shape
    BH, BW = -(-H // 16), -(-W // 16)
    fwd = torch.empty((T, BH, BW, 2), dtype=torch.int16, device=gray.device)
    bwd = torch.empty((T, BH, BW, 2), dtype=torch.int16, device=gray.device)
    resid = torch.empty(T, dtype=torch.int64, device=gray.device)
    cut = torch.empty(T, dtype=torch.uint8, device=gray.device)
    _call("v3d_temporal_motion", gray.device, g, gs, T, W, H, int(search), int(cut_threshold), _dev(fwd, torch.int16, "mv_fwd"),
          _dev(bwd, torch.int16, "mv_bwd"), _dev(resid, torch.int64, "resid"), _dev(cut, torch.uint8, "cut"))
    return fwd, bwd, resid, cut


def temporal_filter_mc_batch(depth, gray, radius, tau, cut, mv_fwd, mv_bwd, fill=True, t0=0, n=None, out=None):
    """temporal_filter_batch with every neighbouring frame read along the chained block vectors of temporal_motion's fields
    (v3d_temporal_filter_mc_batch).  Bit-exact contract: tests/temporal_mc_ref.py."""
    (d, ds, g, gs, T, W, H, n), out = _temporal_filter_args(depth, gray, radius, tau, cut, t0, n, out, (mv_fwd, mv_bwd))
    _call("v3d_temporal_filter_mc_batch", depth.device, d, ds, g, gs, T, W, H, t0, n, int(radius), int(tau), int(bool(fill)),
          _dev(cut, torch.uint8, "cut"), _dev(mv_fwd, torch.int16, "mv_fwd"), _dev(mv_bwd, torch.int16, "mv_bwd"),
          _dev(out, torch.float32, "out"))
    return out


def depth_to_u16_range_batch(depth, lohi, out=None):
    """float32 [n,H,W] + (lo, hi) float32 [n,2] on the device -> uint16 bit patterns in an int16 [n,H,W] tensor: depth_to_u16_batch
    with the range given instead of reduced (v3d_depth_to_u16_range_batch)"""
    d, ds = _clip(depth, torch.float32, "depth")
    n, H, W = depth.shape
    if tuple(lohi.shape) != (n, 2):
        raise NativeError(f"lohi: expected shape {(n, 2)}, got {tuple(lohi.shape)}")
    out = _out(out, (n, H, W), torch.int16, depth.device)
    _call("v3d_depth_to_u16_range_batch", depth.device, d, n, H * W, ds, _dev(lohi, torch.float32, "lohi"), _dev(out, torch.int16, "out"))
    return out


FILL_MAX_WIDTH, FILL_MAX_HEIGHT = 8192, 65535


def fill_holes_disp16_batch(disp, out=None, ws=None):
    """int16 disparity [n,H,W] on the device (frames dense HxW, only the frame stride may differ; < 0 = hole) -> the filled
    disparity, dense [n,H,W] (v3d_fill_holes_disp16_batch; bit-exact contract: tests/fill_ref.py).  out=None allocates the result;
    out=disp fills in place (a single frame or a dense batch).  ws: a uint8 device tensor of at least v3d_fill_holes_ws_bytes(n, H)
    bytes, 16-byte aligned (a caller's staging buffer); None takes one from the caching allocator."""
    d, ds = _clip(disp, torch.int16, "disp")
    n, H, W = disp.shape
    out = _out(out, (n, H, W), torch.int16, disp.device)
    need = lib().v3d_fill_holes_ws_bytes(n, H)
    if ws is None:
        ws = _scratch(need, disp.device)
    elif need and ws.numel() < need:
        raise NativeError(f"ws: {ws.numel()} bytes, the fill needs {need}")
    o = C.c_void_p(out.data_ptr()) if out is disp else _dev(out, torch.int16, "out")
    _call("v3d_fill_holes_disp16_batch", disp.device, d, ds, n, W, H, o, _dev(ws, torch.uint8, "ws"))
    return out


PNG_GRAY16, PNG_BGR8 = 0, 1          # V3D_PNG_GRAY16 / V3D_PNG_BGR8
PNG_MAX_WIDTH, PNG_MAX_HEIGHT = 8192, 65535


def png_deflate_batch(frames, out=None, offsets=None, ws=None):
    """final frames on the device -> one zlib stream per frame (v3d_png_deflate_batch; bit-exact contract: tests/png_ref.py).
    frames: int16 [n,H,W] holding uint16 bit patterns (16-bit gray) or uint8 [n,H,W,3] in BGR order (written as RGB); frames dense,
    only the frame stride may differ.  Returns (out uint8 [v3d_png_out_bytes], offsets int64 [n+1]) on the device: frame f's
    stream starts at out[offsets[f]], offsets[n] is the used size (utils.png_stream_end finds a stream's last byte).  out / offsets
    / ws: a caller's buffers of at least the sizes the library states; None takes them from the caching allocator."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
        raise NativeError("frames: expected a device tensor")
    if frames.dtype == torch.int16 and frames.dim() == 3:
        fmt, item, (n, H, W) = PNG_GRAY16, 2, frames.shape
        dense = frames.stride(2) == 1 and frames.stride(1) == W
    elif frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3:
        fmt, item, (n, H, W, _) = PNG_BGR8, 1, frames.shape
        dense = frames.stride(3) == 1 and frames.stride(2) == 3 and frames.stride(1) == 3 * W
    else:
        raise NativeError(f"frames: expected int16 [n,H,W] or uint8 [n,H,W,3], got {frames.dtype} {tuple(frames.shape)}")
    if not dense or min(n, H, W) < 1:
        raise NativeError("frames: frames must be dense, non-empty images (only the frame stride may differ)")
    L = lib()
    need_out, need_ws = L.v3d_png_out_bytes(fmt, n, W, H), L.v3d_png_ws_bytes(fmt, n, W, H)
    if not need_out:
        raise NativeError(f"png_deflate_batch: {n} frames of {W}x{H} are outside the encoder's range (W <= {PNG_MAX_WIDTH}, H and n <= {PNG_MAX_HEIGHT})")
    dev = frames.device
    out = torch.empty(need_out, dtype=torch.uint8, device=dev) if out is None else out
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev) if offsets is None else offsets
    ws = _scratch(need_ws, dev) if ws is None else ws
    if out.numel() < need_out or ws.numel() < need_ws or offsets.numel() < n + 1:
        raise NativeError(f"png_deflate_batch: out / ws / offsets of {out.numel()} / {ws.numel()} / {offsets.numel()}, need {need_out} / {need_ws} / {n + 1}")
    _call("v3d_png_deflate_batch", dev, C.c_void_p(frames.data_ptr()), frames.stride(0) * item, fmt, n, W, H,
          _dev(out, torch.uint8, "out"), _dev(offsets, torch.int64, "offsets"), _dev(ws, torch.uint8, "ws"))
    return out, offsets


SIG_GW, SIG_GH, SIG_CELLS = 64, 36, 2304      # V3D_SIG_GW / V3D_SIG_GH / V3D_SIG_CELLS
SIG_MIN_WIDTH, SIG_MIN_HEIGHT, SIG_MAX_SIDE, SIG_MAX_COUNT = 64, 36, 8192, 4096


def frame_signature_batch(gray, out=None):
    """luma planes u8 [n,H,W] on the device (frames dense HxW, only the frame stride may differ) -> their signatures, the
    64 x 36 cell means in 8.8 fixed point as uint16 bit patterns in an int16 [n,2304] tensor (v3d_frame_signature_batch;
    bit-exact contract: tests/framematch_ref.py).  out: a caller's [n,2304] int16 tensor (a slice of a resident table)."""
    g, gs = _clip(gray, torch.uint8, "gray")
    n, H, W = gray.shape
    out = _out(out, (n, SIG_CELLS), torch.int16, gray.device)
    _call("v3d_frame_signature_batch", gray.device, g, n, W, H, W, gs, _dev(out, torch.int16, "sig"))
    return out


def signature_scores(sig_a, sig_b):
    """signatures [na,2304] and [nb,2304] (int16-viewed uint16, device) -> (num int64 [na,nb], var_a int64 [na], var_b int64
    [nb]) on the device: the integer numerator and variances of the zero-mean normalised correlation (v3d_signature_scores);
    framematch.zncc divides them on the host."""
    for t, what in ((sig_a, "sig_a"), (sig_b, "sig_b")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != SIG_CELLS or t.shape[0] < 1:
            raise NativeError(f"{what}: expected an int16 [n,{SIG_CELLS}] device tensor")
    na, nb = sig_a.shape[0], sig_b.shape[0]
    dev = sig_a.device
    num = torch.empty((na, nb), dtype=torch.int64, device=dev)
    va = torch.empty(na, dtype=torch.int64, device=dev)
    vb = torch.empty(nb, dtype=torch.int64, device=dev)
    _call("v3d_signature_scores", dev, _dev(sig_a, torch.int16, "sig_a"), na, _dev(sig_b, torch.int16, "sig_b"), nb,
          _dev(num, torch.int64, "num"), _dev(va, torch.int64, "var_a"), _dev(vb, torch.int64, "var_b"))
    return num, va, vb


QUALITY_REPROJ_FIELDS, QUALITY_FLICKER_FIELDS = 8, 4      # V3D_QUALITY_REPROJ_FIELDS / V3D_QUALITY_FLICKER_FIELDS
QUALITY_MAX_WIDTH, QUALITY_MAX_HEIGHT = 8192, 65535


def _quality_buffers(what, need, rows, fields, out, ws, device):
    if not need:
        raise NativeError(f"{what}: outside the entry's range (W <= {QUALITY_MAX_WIDTH}, H and the frame count <= {QUALITY_MAX_HEIGHT})")
    out = _out(out, (rows, fields), torch.int64, device)
    if ws is None:
        ws = _scratch(need, device)
    elif ws.numel() < need:
        raise NativeError(f"ws: {ws.numel()} bytes, {what} needs {need}")
    return out, ws


def quality_reproj_batch(lg, rg, disp16, bad_thr=16, out=None, ws=None, right_shift=0):
    """left / right gray u8 [n,H,W] and the int16 disparity [n,H,W] on the device (frames dense HxW, only the frame strides may
    differ) -> the reprojection records, int64 [n,8]: n_valid, n_cmp, sad, ssd, n_bad, sad0, ssd0, n_bad0 in 1/16 gray levels
    (v3d_quality_reproj_batch; bit-exact contract: tests/quality_ref.py).  out / ws: a caller's buffers; None takes them from the
    caching allocator.
    right_shift k > 0 (a disparity rebiased by a search window [-k, 64 - k), depth.py --min-disparity): columns [0, W - k) of the left
    gray and of the disparity (made dense) against the right gray advanced by k bytes, same pitch: R'[i] = R[i + k], so u = 16 x - d
    addresses the true match and the record's "disparity 0" is the disparity -k."""
    k = int(right_shift)
    l, ls = _clip(lg, torch.uint8, "left gray")
    r, rs = _clip(rg, torch.uint8, "right gray")
    d, ds = _clip(disp16, torch.int16, "disp16")
    n, H, W = lg.shape
    if tuple(rg.shape) != (n, H, W) or tuple(disp16.shape) != (n, H, W) or rs != ls:
        raise NativeError(f"right gray {tuple(rg.shape)} / disp16 {tuple(disp16.shape)} do not match left gray {tuple(lg.shape)} (one frame stride for both grays)")
    if isinstance(bad_thr, bool) or int(bad_thr) != bad_thr or not 0 <= bad_thr <= 255:
        raise ValueError(f"bad threshold must be an integer in [0, 255], got {bad_thr!r}")
    if not 0 <= k < W:
        raise ValueError(f"right_shift must lie in [0, W), got {right_shift!r}")
    if k:
        r = C.c_void_p(rg.data_ptr() + k)
        dense = disp16[:, :, :W - k].contiguous()          # held until the launch is enqueued (the allocator is stream-ordered)
        d, ds = _clip(dense, torch.int16, "disp16")
    out, ws = _quality_buffers("quality_reproj_batch", lib().v3d_quality_reproj_ws_bytes(n, W - k, H), n, QUALITY_REPROJ_FIELDS, out, ws, lg.device)
    _call("v3d_quality_reproj_batch", lg.device, l, r, n, W - k, H, W, ls, d, ds, int(bad_thr), _dev(out, torch.int64, "out"),
          _dev(ws, torch.uint8, "ws"))
    return out


def quality_flicker_batch(depth, gray, still, jump16, out=None, ws=None):
    """depth f32 [T,H,W] and left gray u8 [T,H,W] on the device (T >= 2; frames dense, only the frame strides may differ) -> the
    flicker records of the T-1 pairs of consecutive frames, int64 [T-1,4]: luma_sad, n_still, flicker (in 1/16 px), n_jump
    (v3d_quality_flicker_batch; bit-exact contract: tests/quality_ref.py)"""
    d, ds = _clip(depth, torch.float32, "depth")
    g, gs = _clip(gray, torch.uint8, "gray")
    T, H, W = depth.shape
    if tuple(gray.shape) != (T, H, W) or T < 2:
        raise NativeError(f"gray {tuple(gray.shape)} does not match depth {tuple(depth.shape)}, or fewer than two frames")
    for name, v, hi in (("still", still, 255), ("jump16", jump16, 32767)):
        if isinstance(v, bool) or int(v) != v or not 0 <= v <= hi:
            raise ValueError(f"{name} must be an integer in [0, {hi}], got {v!r}")
    out, ws = _quality_buffers("quality_flicker_batch", lib().v3d_quality_flicker_ws_bytes(T, W, H), T - 1, QUALITY_FLICKER_FIELDS, out, ws, depth.device)
    _call("v3d_quality_flicker_batch", depth.device, d, ds, g, gs, T, W, H, int(still), int(jump16), _dev(out, torch.int64, "out"),
          _dev(ws, torch.uint8, "ws"))
    return out


MATCH_FIELDS = 6                                   # V3D_MATCH_FIELDS
MATCH_A_MIN, MATCH_A_MAX, MATCH_B_MAX = 1 << 12, 1 << 20, 1 << 29
MATCH_MAX_CANDIDATES = 65535
WARP_B_MAX = 1 << 40


def plane_profiles_batch(gray):
    """luma planes u8 [n,H,W] on the device (frames dense HxW, only the frame stride may differ) -> (col int32 [n,W], row int32
    [n,H]): the column and row sums as uint32 bit patterns (v3d_plane_profiles_batch; bit-exact contract: tests/register_ref.py)"""
    g, gs = _clip(gray, torch.uint8, "gray")
    n, H, W = gray.shape
    need = lib().v3d_plane_profiles_ws_bytes(n, W, H)
    if not need:
        raise NativeError(f"plane_profiles_batch: {n} planes of {W}x{H} outside the entry's range (at most 65535 of 8192 x 8192)")
    col = torch.empty((n, W), dtype=torch.int32, device=gray.device)
    row = torch.empty((n, H), dtype=torch.int32, device=gray.device)
    ws = _scratch(need, gray.device)
    _call("v3d_plane_profiles_batch", gray.device, g, n, W, H, W, gs, _dev(col, torch.int32, "col"), _dev(row, torch.int32, "row"),
          _dev(ws, torch.uint8, "ws"))
    return col, row


def check_match_candidates(cand):
    """a host-side candidate list -> int64 [C,2]; ValueError outside the entry's domain (the device refuses those in band)"""
    c = np.ascontiguousarray(np.asarray(cand, dtype=np.int64).reshape(-1, 2))
    bad = (c[:, 0] < MATCH_A_MIN) | (c[:, 0] > MATCH_A_MAX) | (np.abs(c[:, 1]) > MATCH_B_MAX)
    if not len(c) or bad.any():
        raise ValueError("no candidates" if not len(c) else
                         f"candidate {c[np.flatnonzero(bad)[0]].tolist()} outside 2^12 <= a <= 2^20, |b| <= 2^29")
    return c


def profile_match_scores(prof_a, prof_b, cand, bins):
    """profiles int32-viewed uint32 [K,na] (source) and [K,nb] (target) on the device, cand (a, b) in Q16: a NumPy int64 [C,2]
    (checked against the domain here, ValueError, then copied) or a device int64 [C,2] tensor -> the records int64 [K,C,6] on the
    device: (n_pairs, sum da, sum db, sum da db, sum da^2, sum db^2) (v3d_profile_match_scores; tests/register_ref.py)"""
    for t, what in ((prof_a, "prof_a"), (prof_b, "prof_b")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise NativeError(f"{what}: expected an int32 [K,n] device tensor")
    (K, na), (Kb, nb) = prof_a.shape, prof_b.shape
    if K != Kb:
        raise NativeError(f"prof_a has {K} frames, prof_b {Kb}")
    if not isinstance(cand, torch.Tensor):
        cand = torch.from_numpy(check_match_candidates(cand)).to(prof_a.device)
    if cand.dim() != 2 or cand.shape[1] != 2:
        raise NativeError(f"cand: expected int64 [C,2], got {tuple(cand.shape)}")
    Cn = cand.shape[0]
    need = lib().v3d_profile_match_ws_bytes(K, na, nb)
    if not need:
        raise NativeError(f"profile_match_scores: {K} frames of {na} and {nb} samples outside the entry's range (4096 frames, 8192 samples)")
    out = torch.empty((K, Cn, MATCH_FIELDS), dtype=torch.int64, device=prof_a.device)
    ws = _scratch(need, prof_a.device)
    _call("v3d_profile_match_scores", prof_a.device, _dev(prof_a, torch.int32, "prof_a"), na, _dev(prof_b, torch.int32, "prof_b"), nb,
          K, _dev(cand, torch.int64, "cand"), Cn, int(bins), _dev(out, torch.int64, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def warp_u16_batch(src, ax, bx, ay, by, Wo, Ho, fill=0, out=None):
    """u16 planes as int16 bit patterns [n,Hs,Ws] on the device (frames dense, only the frame stride may differ) resampled through
    u = ax x + bx, v = ay y + by (Q16 source-index coordinates) -> int16-viewed u16 [n,Ho,Wo]; `fill` outside the source
    (v3d_warp_u16_batch; bit-exact contract: tests/register_ref.py)"""
    s, ss = _clip(src, torch.int16, "src")
    n, Hs, Ws = src.shape
    out = _out(out, (n, int(Ho), int(Wo)), torch.int16, src.device)
    if not 0 <= int(fill) <= 65535:
        raise ValueError(f"fill must lie in [0, 65535], got {fill!r}")
    _call("v3d_warp_u16_batch", src.device, s, n, Ws, Hs, ss, int(ax), int(bx), int(ay), int(by), int(fill),
          _dev(out, torch.int16, "out"), int(Wo), int(Ho))
    return out


def _bgr_frames(t, what):
    """a u8 [n,H,W,3] device tensor of dense BGR triples (the row pitch and the frame stride may differ) -> (pointer, frame stride,
    n, W, H, pitch), strides in bytes"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
        raise NativeError(f"{what}: expected a uint8 [n,H,W,3] device tensor")
    if t.stride(3) != 1 or t.stride(2) != 3:
        raise NativeError(f"{what}: pixels must be dense BGR triples (only the row pitch and the frame stride may differ)")
    n, H, W, _ = t.shape
    pitch = t.stride(1) if H > 1 else 3 * W
    return C.c_void_p(t.data_ptr()), (t.stride(0) if n > 1 else H * pitch), n, W, H, pitch


def _rect(rect, W, H):
    """(x0, y0, x1, y1) or None = the whole image, as four ints (the entry checks them)"""
    return (0, 0, W, H) if rect is None else tuple(int(v) for v in rect)


def bgr_hist_batch(bgr, rect=None, out=None):
    """u8 [n,H,W,3] BGR frames on the device -> int32 [n,3,256] (the bits of uint32 counts): per frame and channel, how often each
    level occurs among the pixels [x0, x1) x [y0, y1) of rect = (x0, y0, x1, y1), None = the whole image (v3d_bgr_hist_batch;
    bit-exact contract: tests/colour_ref.py)"""
    p, fs, n, W, H, pitch = _bgr_frames(bgr, "bgr")
    out = _out(out, (n, 3, 256), torch.int32, bgr.device)
    _call("v3d_bgr_hist_batch", bgr.device, p, fs, n, W, H, pitch, *_rect(rect, W, H), _dev(out, torch.int32, "out"))
    return out


def colour_lut_batch(hist_src, hist_dst, group=1, out=None):
    """two int32 [n,3,256] histogram sets -> u8 [ceil(n/group),3,256]: table j maps the levels of the source frames [j group,
    (j+1) group) onto the target's by histogram matching, exactly and monotonically (v3d_colour_lut_batch)"""
    if not isinstance(hist_src, torch.Tensor) or hist_src.dim() != 3 or tuple(hist_src.shape[1:]) != (3, 256) or hist_src.shape != hist_dst.shape:
        raise NativeError("hist_src / hist_dst: expected two int32 [n,3,256] device tensors of one shape")
    n, group = hist_src.shape[0], int(group)
    if not 1 <= group <= n:
        raise ValueError(f"group must lie in [1, {n}], got {group!r}")
    out = _out(out, ((n + group - 1) // group, 3, 256), torch.uint8, hist_src.device)
    _call("v3d_colour_lut_batch", hist_src.device, _dev(hist_src, torch.int32, "hist_src"), _dev(hist_dst, torch.int32, "hist_dst"),
          n, group, _dev(out, torch.uint8, "out"))
    return out


def bgr_lut_batch(src, lut, rect=None, out=None):
    """out = lut[channel][src] on the pixels of rect (None = the whole image) of u8 [n,H,W,3] BGR frames on the device; lut u8
    [3,256] or [1,3,256] (one table for all frames) or [n,3,256] (one per frame).  out=src works in place; out=None gives a new
    tensor that equals src outside the rectangle (v3d_bgr_lut_batch)"""
    p, fs, n, W, H, pitch = _bgr_frames(src, "src")
    if not isinstance(lut, torch.Tensor) or tuple(lut.shape[-2:]) != (3, 256) or lut.dim() not in (2, 3) or \
            (lut.dim() == 3 and lut.shape[0] not in (1, n)):
        raise NativeError(f"lut: expected a uint8 [3,256] or [1 or {n},3,256] device tensor")
    x0, y0, x1, y1 = _rect(rect, W, H)
    if out is None:
        whole = (x0, y0, x1, y1) == (0, 0, W, H)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=src.device) if whole else src.clone(memory_format=torch.contiguous_format)
    if tuple(out.shape) != tuple(src.shape):
        raise NativeError(f"out: expected shape {tuple(src.shape)}, got {tuple(out.shape)}")
    q, qs, _, _, _, qpitch = _bgr_frames(out, "out")
    _call("v3d_bgr_lut_batch", src.device, p, fs, n, W, H, pitch, x0, y0, x1, y1, _dev(lut, torch.uint8, "lut"),
          768 if lut.dim() == 3 and lut.shape[0] == n and n > 1 else 0, q, qs, qpitch)
    return out


def verify_cell(ax, ay):
    """(cx, cy): the cell of targets that one stored-eye sample spans under the Q16 map scales ax, ay (ceil(65536 / a), 1 .. 16)"""
    return (65536 + int(ax) - 1) // int(ax), (65536 + int(ay) - 1) // int(ay)


def verify_eye_source_batch(eye_bgr, sbs, eye, ax, bx, ay, by, tau, out=None):
    """a rendered eye checked IN PLACE against the stored eye `eye` (0 | 1) of the SBS frames (v3d_verify_eye_source_batch):
    eye_bgr u8 [n,H,W,3] on the device, usually a view of a packed output (the right half of a full-SBS frame, the lower half of a
    full top-bottom one: the row pitch and the frame stride may differ), sbs u8 [n,Hs,Ws,3] as for render_stereo_source_batch.  A
    cell of verify_cell(ax, ay) targets whose channel sums differ from the sampled stored eye's by more than tau per pixel takes
    the sample.  -> int32 [n] (the bits of uint32 counts): replaced cells per frame.  Bit-exact contract: tests/verify_ref.py."""
    p, fs, n, W, H, pitch = _bgr_frames(eye_bgr, "eye_bgr")
    sp, ss, ns, Ws, Hs, spitch = _bgr_frames(sbs, "sbs")
    if ns != n:
        raise NativeError(f"sbs holds {ns} frames, eye_bgr {n}")
    if eye not in (0, 1) or isinstance(eye, bool):
        raise ValueError(f"eye must be 0 (left) or 1 (right), got {eye!r}")
    if isinstance(tau, bool) or not isinstance(tau, (int, np.integer)) or not 0 <= tau <= 765:
        raise ValueError(f"tau must be an integer in [0, 765], got {tau!r}")
    out = _out(out, (n,), torch.int32, eye_bgr.device)
    _call("v3d_verify_eye_source_batch", eye_bgr.device, p, fs, pitch, n, W, H, sp, ss, Ws, Hs, spitch, int(eye), int(ax), int(bx),
          int(ay), int(by), int(tau), _dev(out, torch.int32, "out"))
    return out


FIDELITY_FIELDS = 6                                # V3D_FIDELITY_FIELDS: n_cells, sad, ssd, n_bad, n_win, ssim_q20
FIDELITY_BAD_MAX = 765


def fidelity_grid(W, H, ax, ay):
    """(ncx, ncy, n_win) of v3d_eye_fidelity_batch: the cells of verify_cell(ax, ay) targets over W x H, and the 8 x 8-cell windows
    at stride 4 that fit into them"""
    cx, cy = verify_cell(ax, ay)
    ncx, ncy = -(-int(W) // cx), -(-int(H) // cy)
    nwx, nwy = ((ncx - 8) // 4 + 1 if ncx >= 8 else 0), ((ncy - 8) // 4 + 1 if ncy >= 8 else 0)
    return ncx, ncy, nwx * nwy


def eye_fidelity_batch(eye_bgr, sbs, eye, ax, bx, ay, by, bad_thr, out=None, ws=None):
    """a rendered eye measured against the stored eye `eye` (0 | 1) of the SBS frames (v3d_eye_fidelity_batch): eye_bgr u8
    [n,H,W,3] on the device, usually a view of a packed output, and sbs u8 [n,Hs,Ws,3], both as for verify_eye_source_batch and
    both read only -> int64 [n,6]: n_cells, sad, ssd, n_bad of the cell means (cells of verify_cell(ax, ay) targets; n_bad: those
    whose three channel differences add up to more than bad_thr) and n_win, ssim_q20 of the cells' luma (8 x 8-cell windows at
    stride 4, the sum of their SSIM in Q20).  out / ws: a caller's buffers; None takes them from the caching allocator.
    Bit-exact contract: tests/fidelity_ref.py."""
    p, fs, n, W, H, pitch = _bgr_frames(eye_bgr, "eye_bgr")
    sp, ss, ns, Ws, Hs, spitch = _bgr_frames(sbs, "sbs")
    if ns != n:
        raise NativeError(f"sbs holds {ns} frames, eye_bgr {n}")
    if eye not in (0, 1) or isinstance(eye, bool):
        raise ValueError(f"eye must be 0 (left) or 1 (right), got {eye!r}")
    if isinstance(bad_thr, bool) or not isinstance(bad_thr, (int, np.integer)) or not 0 <= bad_thr <= FIDELITY_BAD_MAX:
        raise ValueError(f"bad_thr must be an integer in [0, {FIDELITY_BAD_MAX}], got {bad_thr!r}")
    need = lib().v3d_eye_fidelity_ws_bytes(n, W, H, int(ax), int(ay))
    if not need:
        raise NativeError(f"eye_fidelity_batch: {n} eyes of {W}x{H} under the scales ({ax}, {ay}) outside the entry's range "
                          f"(W <= 8192, scales in [2^12, 2^20])")
    out = _out(out, (n, FIDELITY_FIELDS), torch.int64, eye_bgr.device)
    if ws is None:
        ws = _scratch(need, eye_bgr.device)
    elif ws.numel() < need:
        raise NativeError(f"ws: {ws.numel()} bytes, eye_fidelity_batch needs {need}")
    _call("v3d_eye_fidelity_batch", eye_bgr.device, p, fs, pitch, n, W, H, sp, ss, Ws, Hs, spitch, int(eye), int(ax), int(bx),
          int(ay), int(by), int(bad_thr), _dev(out, torch.int64, "out"), _dev(ws, torch.uint8, "ws"))
    return out


def to_device(a, device="cuda"):
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:          # e.g. a memory-mapped clip: torch wants a writable buffer
        a = a.copy()
    return torch.from_numpy(a).to(device)


def fuse_eye_source_ws_bytes(n, Ws, Hs):
    """the workspace of fuse_eye_source_batch for n SBS frames of Ws x Hs in bytes (v3d_fuse_eye_source_ws_bytes)"""
    need = lib().v3d_fuse_eye_source_ws_bytes(int(n), int(Ws), int(Hs))
    if not need:
        raise NativeError(f"fuse_eye_source_batch: {n} SBS frames of {Ws}x{Hs} outside the entry's range (Ws even, Ws/2 <= 8192)")
    return need


def fuse_eye_source_batch(eye_bgr, sbs, eye, ax, bx, ay, by, ws=None):
    """a rendered eye fused IN PLACE with the stored eye `eye` (0 | 1) of the SBS frames (v3d_fuse_eye_source_batch): eye_bgr u8
    [n,H,W,3] on the device, usually a view of a packed output, and sbs u8 [n,Hs,Ws,3], both as for verify_eye_source_batch.  The
    eye keeps its detail above the stored eye's resolution and takes everything below it from the stored eye: E - LP(E) + P.  ws:
    a caller's uint8 scratch of v3d_fuse_eye_source_ws_bytes; None takes it from the caching allocator.  -> eye_bgr.
    Bit-exact contract: tests/fuse_ref.py."""
    p, fs, n, W, H, pitch = _bgr_frames(eye_bgr, "eye_bgr")
    sp, ss, ns, Ws, Hs, spitch = _bgr_frames(sbs, "sbs")
    if ns != n:
        raise NativeError(f"sbs: {ns} frames for {n} eye images")
    if eye not in (0, 1):
        raise ValueError(f"eye must be 0 (left) or 1 (right), got {eye!r}")
    need = fuse_eye_source_ws_bytes(n, Ws, Hs)
    if ws is None:
        ws = _scratch(need, eye_bgr.device)
    elif ws.numel() < need:
        raise NativeError(f"ws: {ws.numel()} bytes, fuse_eye_source_batch needs {need}")
    _call("v3d_fuse_eye_source_batch", eye_bgr.device, p, fs, pitch, n, W, H, sp, ss, Ws, Hs, spitch, int(eye), int(ax), int(bx),
          int(ay), int(by), _dev(ws, torch.uint8, "ws"))
    return eye_bgr
