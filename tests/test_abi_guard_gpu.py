"""Memory behaviour of every C-ABI entry that enqueues work (include/v3d_hip.h: every function with a `void* stream`).

The binding (video_3d_pipeline/_native.py) always passes fresh, exactly sized, 512-byte aligned tensors, dense pitches and dense
strides.  Here each entry is called through the raw ctypes functions on buffers of a guard arena (tests/guard_arena.py):
red zones around every buffer, poisoned outputs, workspaces and padding.  Every case runs in these placements:

  aligned    every buffer at 256 k bytes, dense pitch and strides;
  minalign   every pointer at the alignment the header grants and no better: 256 k + one element for typed pointers,
             256 k + 16 for a `void* ws` (256 k + 8 for v3d_temporal_cuts), on widths the vector paths would otherwise take;
  pad16      every pitch / stride argument padded by a multiple of 16 bytes;
  padodd     every pitch padded by 3 (gray) or 5 (BGR) bytes, every frame stride by 7 elements; batches use n = 3;

and `aligned` + `padodd` again with the poison byte 0xFF instead of 0xA5 (test_two_poisons): outputs must not change by a bit.
Every run asserts rc == 0, outputs == expected, and that no byte outside the outputs' and workspaces' payloads changed.

Expected outputs: the entry's own reference (oracle / stereo_ref / temporal_ref / range_ref) for the bit-exact entries; for the
float-toleranced entries (guided filter, correlation lookup, audio) the binding's ordinary call on fresh tensors, bit for bit
(their own test files tie that call to float64 references).  S_out of v3d_sgbm_debug_raw has no reference of its own (the
device keeps the sum of all paths but the last): it is compared with the binding's dense call as well.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import textured_pair
from guard_arena import Arena

PLACEMENTS = ("aligned", "minalign", "pad16", "padodd")
WS_ALIGN = 16                      # what the header grants for a `void* ws` unless the entry says otherwise


class Kit:
    """declares one case's buffers in an arena according to the placement"""

    def __init__(self, place, poison, native=None, oracle=None, device="cuda"):
        self.place, self.native, self.oracle = place, native, oracle
        self.arena = Arena(device, poison)
        self.padded = place in ("pad16", "padodd")
        self.outs = {}

    def _skew(self, itemsize, align):
        return (align or itemsize) if self.place == "minalign" else 0

    def _pitch(self, cols, itemsize, odd):
        if self.place == "pad16":
            return (cols * itemsize // 16 + 2) * 16 // itemsize
        return cols + odd

    def _stride(self, frame_elems, itemsize):
        if self.place == "pad16":
            return (frame_elems * itemsize // 16 + 2) * 16 // itemsize
        return frame_elems + 7

    def inp(self, name, data, pitch=False, stride=False, align=None, odd=3, role="in"):
        a = np.ascontiguousarray(data)
        it = a.dtype.itemsize
        cols = a.shape[-1]
        rows = a.shape[-2] if a.ndim >= 2 else 1
        p = self._pitch(cols, it, odd) if pitch and self.padded else None
        fs = self._stride(rows * (p or cols), it) if stride and self.padded and a.ndim == 3 else None
        return self.arena.buf(name, role, a.dtype, a.shape, align, self._skew(it, align), p, fs).set(a)

    def out(self, name, dtype, shape, align=None):
        it = np.dtype(dtype).itemsize
        b = self.arena.buf(name, "out", dtype, shape, align, self._skew(it, align))
        self.outs[name] = b
        return b

    def inout(self, name, data):
        b = self.inp(name, data, role="inout")
        self.outs[name] = b
        return b

    def ws(self, name, count, dtype=np.uint8, align=None):
        it = np.dtype(dtype).itemsize
        return self.arena.buf(name, "ws", dtype, (max(int(count), 1),), align, self._skew(it, align))


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(b):
    return C.c_void_p(b.ptr)


def _dev(native, a):
    return native.to_device(np.ascontiguousarray(a))


def _bits(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------
# the matcher: a handle per run, routes as handle options
# ------------------------------------------------------------------------------------------------------------------------
SGBM_ROUTES = {"lockstep-march": {"lockstep": 1, "lrm_tiles": 0}, "chains-tiles": {"lockstep": 0, "lrm_tiles": 1}}
_pairs = {}


def _pair(W, H, seed):
    key = (W, H, seed)
    if key not in _pairs:
        _pairs[key] = textured_pair(W, H, seed=seed)
    return _pairs[key]


def _route_dims(variant):
    """'route@WxH' -> (route, W, H)"""
    route, dims = variant.split("@")
    W, H = dims.split("x")
    return route, int(W), int(H)


class _Handle:
    def __init__(self, k, W, H, n, route):
        self.m = k.native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options=SGBM_ROUTES[route])

    def finish(self):
        errs = self.m.sync_errors()
        self.m.close()
        assert errs == 0, f"{errs} lock-step time-outs"


def case_sgbm_compute(k, variant):
    route, W, H = _route_dims(variant)
    L, R = _pair(W, H, 11 * W + H)
    l, r = k.inp("left", L, pitch=True), k.inp("right", R, pitch=True)
    o = k.out("disp16", np.int16, (H, W))
    h = _Handle(k, W, H, 1, route)
    call = lambda lib: lib.v3d_sgbm_compute(h.m._h, _p(l), _p(r), W, H, l.pitch_bytes, _p(o), _stream())
    return call, lambda: {"disp16": k.oracle.sgbm_compute(L, R)}, h.finish


def case_sgbm_compute_batch(k, variant):
    route, W, H = _route_dims(variant)
    n = 3
    pairs = [_pair(W, H, 400 + i) for i in range(n)]
    Ls, Rs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    l, r = k.inp("left", Ls, pitch=True, stride=True), k.inp("right", Rs, pitch=True, stride=True)
    o = k.out("disp16", np.int16, (n, H, W))
    h = _Handle(k, W, H, n, route)
    call = lambda lib: lib.v3d_sgbm_compute_batch(h.m._h, _p(l), _p(r), n, W, H, l.pitch_bytes, l.frame_stride_bytes, _p(o), _stream())
    return call, lambda: {"disp16": np.stack([k.oracle.sgbm_compute(*p) for p in pairs])}, h.finish


def case_sgbm_debug_cost_volume(k, variant):
    route, W, H = _route_dims(variant)
    L, R = _pair(W, H, 7)
    l, r = k.inp("left", L, pitch=True), k.inp("right", R, pitch=True)
    o = k.out("C", np.int16, (H, (W - 64) * 64))
    h = _Handle(k, W, H, 1, route)
    call = lambda lib: lib.v3d_sgbm_debug_cost_volume(h.m._h, _p(l), _p(r), W, H, l.pitch_bytes, _p(o), _stream())
    return call, lambda: {"C": k.oracle.cost_volume(L, R).reshape(H, -1)}, h.finish


def case_sgbm_debug_raw(k, variant):
    variant, want_S = variant.rsplit("-", 1)
    want_S = want_S == "S"
    route, W, H = _route_dims(variant)
    L, R = _pair(W, H, 9)
    l, r = k.inp("left", L, pitch=True), k.inp("right", R, pitch=True)
    o = k.out("disp16", np.int16, (H, W))
    s = k.out("S", np.int16, (H, (W - 64) * 64)) if want_S else None
    h = _Handle(k, W, H, 1, route)
    call = lambda lib: lib.v3d_sgbm_debug_raw(h.m._h, _p(l), _p(r), W, H, l.pitch_bytes, _p(o), _p(s) if want_S else None, _stream())

    def expect():
        want = {"disp16": k.oracle.sgbm_raw(L, R)}
        if want_S:
            m = k.native.StereoSGBM(max_width=W, max_height=H, options=SGBM_ROUTES[route])
            want["S"] = _bits(m.debug_raw(_dev(k.native, L), _dev(k.native, R), want_S=True)[1]).reshape(H, -1)
            m.close()
        return want
    return call, expect, h.finish


def _disparity_image(W, H, seed):
    rng = np.random.default_rng(seed)
    img = (rng.integers(0, 64, (H, W)) * 16).astype(np.int16)
    img[rng.random((H, W)) < 0.3] = -16
    img[H // 4:H // 2, W // 4:W // 2] = 320                # one large component next to the speckles
    return img


def case_median3x3_i16(k, variant):
    W, H = 264, 33                                          # 264 = 8 * 33: vector-friendly, one block and a ragged second one
    img = _disparity_image(W, H, 3)
    s, o = k.inp("src", img), k.out("dst", np.int16, (H, W))
    call = lambda lib: lib.v3d_median3x3_i16(_p(s), W, H, _p(o), _stream())
    return call, lambda: {"dst": k.oracle.median3x3(img)}, None


def case_filter_speckles(k, variant):
    W, H = (int(v) for v in variant.split("x"))           # test_speckle_run_lists_extremes: 640 takes the 8- and 16-byte loads, 516 the 8-byte ones
    img = _disparity_image(W, H, W + H)
    io = k.inout("img", img)
    ws = k.ws("labels_ws", 3 * W * H, np.int32)
    call = lambda lib: lib.v3d_filter_speckles(_p(io), W, H, -16, 100, 512, _p(ws), _stream())
    return call, lambda: {"img": k.oracle.filter_speckles(img)}, None


# ------------------------------------------------------------------------------------------------------------------------
# either side of the matcher
# ------------------------------------------------------------------------------------------------------------------------
def _sbs(n, W, H, seed):
    sbs = np.random.default_rng(seed).integers(0, 256, (n, H, W * 3), dtype=np.uint8)
    sbs[:, :, 60:120] = 255                                 # saturating edges overshoot under Lanczos
    sbs[:, :, 120:180] = 0
    return sbs


def _sbs_dims(variant):
    mode, dims = variant.split("@")
    unsq = mode == "unsqueeze"
    W, H = (int(v) for v in dims.split("x"))                # 1076 * 3 = 3228: a multiple of 4, interior blocks stage dwords
    return unsq, W, H, (W if unsq else W // 2)


def case_sbs_to_gray(k, variant):
    unsq, W, H, ow = _sbs_dims(variant)
    sbs = _sbs(1, W, H, W + H)[0]
    s = k.inp("sbs", sbs, pitch=True, odd=5)
    L, R = k.out("left", np.uint8, (H, ow)), k.out("right", np.uint8, (H, ow))
    call = lambda lib: lib.v3d_sbs_to_gray(_p(s), W, H, s.pitch_bytes, int(unsq), _p(L), _p(R), _stream())
    return call, lambda: dict(zip(("left", "right"), k.oracle.sbs_to_gray(sbs.reshape(H, W, 3), unsq))), None


def case_split_sbs(k, variant):
    unsq, W, H, ow = _sbs_dims(variant)
    sbs = _sbs(1, W, H, W + H + 1)[0]
    s = k.inp("sbs", sbs, pitch=True, odd=5)
    L, R = k.out("left", np.uint8, (H, ow * 3)), k.out("right", np.uint8, (H, ow * 3))
    call = lambda lib: lib.v3d_split_sbs(_p(s), W, H, s.pitch_bytes, int(unsq), _p(L), _p(R), _stream())
    return call, lambda: {n: a.reshape(H, -1) for n, a in zip(("left", "right"), k.oracle.split_sbs(sbs.reshape(H, W, 3), unsq))}, None


def case_sbs_to_gray_batch(k, variant):
    unsq, W, H, ow = _sbs_dims(variant)
    n = 3
    sbs = _sbs(n, W, H, W + H + 2)
    s = k.inp("sbs", sbs, pitch=True, stride=True, odd=5)
    L, R = k.out("left", np.uint8, (n, H, ow)), k.out("right", np.uint8, (n, H, ow))
    call = lambda lib: lib.v3d_sbs_to_gray_batch(_p(s), n, W, H, s.pitch_bytes, s.frame_stride_bytes, int(unsq), _p(L), _p(R), _stream())

    def expect():
        per = [k.oracle.sbs_to_gray(f.reshape(H, W, 3), unsq) for f in sbs]
        return {"left": np.stack([p[0] for p in per]), "right": np.stack([p[1] for p in per])}
    return call, expect, None


def case_bgr_to_gray(k, variant):
    H, W = 33, 71
    img = np.random.default_rng(6).integers(0, 256, (H, W * 3), dtype=np.uint8)
    s, o = k.inp("bgr", img), k.out("gray", np.uint8, (H, W))
    call = lambda lib: lib.v3d_bgr_to_gray(_p(s), H * W, _p(o), _stream())
    return call, lambda: {"gray": k.oracle.bgr_to_gray(img.reshape(H, W, 3))}, None


def _disp(shape, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(-1, 64 * 16, shape).astype(np.int16)
    d[rng.random(shape) < 0.2] = -16
    return d


def _depth(shape, seed):
    return k_oracle_free_disp_to_depth(_disp(shape, seed))


def k_oracle_free_disp_to_depth(d):
    """disparity x16 -> float32 depth, multiples of 1/16, <= 0 -> 0 (input data only: never an expected value)"""
    return np.maximum(d.astype(np.float32) / np.float32(16), np.float32(0))


def case_disp_to_depth(k, variant):
    d = _disp((20, 332), 7)
    s, o = k.inp("disp16", d), k.out("depth", np.float32, d.shape)
    call = lambda lib: lib.v3d_disp_to_depth(_p(s), d.size, _p(o), _stream())
    return call, lambda: {"depth": k.oracle.disp_to_depth(d)}, None


def case_depth_to_u16(k, variant):
    dep = _depth((20, 332), 8)
    s, o, ws = k.inp("depth", dep), k.out("u16", np.uint16, dep.shape), k.ws("minmax_ws", 2, np.float32)
    call = lambda lib: lib.v3d_depth_to_u16(_p(s), dep.size, _p(o), _p(ws), _stream())
    return call, lambda: {"u16": k.oracle.depth_to_u16(dep)}, None


def case_depth_to_u16_batch(k, variant):
    n = 3
    dep = _depth((n, 20, 332), 9) + np.arange(n, dtype=np.float32)[:, None, None]
    s, o, ws = k.inp("depth", dep, stride=True), k.out("u16", np.uint16, dep.shape), k.ws("minmax_ws", 2 * n, np.float32)
    call = lambda lib: lib.v3d_depth_to_u16_batch(_p(s), n, 20 * 332, s.frame_stride, _p(o), _p(ws), _stream())
    return call, lambda: {"u16": np.stack([k.oracle.depth_to_u16(f) for f in dep])}, None


def case_round_to_u16(k, variant):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-50, 70000, 5000), np.arange(0, 300) + 0.5, [-0.5, 65534.5, 65535.5, 1e9, -1e9, np.nan]]).astype(np.float32)
    s, o = k.inp("depth", x), k.out("u16", np.uint16, x.shape)
    call = lambda lib: lib.v3d_round_to_u16(_p(s), x.size, _p(o), _stream())
    return call, lambda: {"u16": np.clip(np.rint(np.nan_to_num(x, nan=0.0)), 0, 65535).astype(np.uint16)}, None


def case_mono_blend(k, variant):
    W, H = 200, 60
    mw, mh = (W, H) if variant == "same-size" else (64, 48)
    d = _disp((H, W), 10)
    mono = (np.random.default_rng(11).random((mh, mw)) * 7 + 1).astype(np.float32)
    s, m, o = k.inp("disp16", d), k.inp("mono", mono), k.out("depth", np.float32, (H, W))
    ws = k.ws("ws", k.native.lib().v3d_mono_blend_ws_bytes(1), align=WS_ALIGN)
    call = lambda lib: lib.v3d_mono_blend(_p(s), W, H, _p(m), mw, mh, 0.7, 0.3, _p(o), _p(ws), _stream())
    return call, lambda: {"depth": k.oracle.mono_blend(d, mono)}, None


def case_mono_blend_batch(k, variant):
    W, H, n = 200, 60, 3
    mw, mh = (W, H) if variant == "same-size" else (64, 48)
    d = _disp((n, H, W), 12)
    mono = (np.random.default_rng(13).random((n, mh, mw)) * 7 + 1).astype(np.float32)
    s, m, o = k.inp("disp16", d), k.inp("mono", mono, stride=True), k.out("depth", np.float32, (n, H, W))
    ws = k.ws("ws", k.native.lib().v3d_mono_blend_ws_bytes(n), align=WS_ALIGN)
    call = lambda lib: lib.v3d_mono_blend_batch(_p(s), n, W, H, _p(m), mw, mh, m.frame_stride, 0.7, 0.3, _p(o), _p(ws), _stream())
    return call, lambda: {"depth": np.stack([k.oracle.mono_blend(d[i], mono[i]) for i in range(n)])}, None


# ------------------------------------------------------------------------------------------------------------------------
# guided filter: three kernel routes (library-wide options, restored after every run)
# ------------------------------------------------------------------------------------------------------------------------
GF_ROUTES = {"fused": {"gf_fused": 1, "gf_tiled": 0}, "sweeps": {"gf_fused": 0, "gf_tiled": 0}, "tiled": {"gf_fused": 1, "gf_tiled": 1}}
CORR_ROUTES = {"fused": {"corr_fused": 1}, "warp-gemm": {"corr_fused": 0}}


class _Options:
    """set library-wide switches, put the old values back"""

    def __init__(self, native, opts):
        self.native, self.opts, self.old = native, opts, {}

    def __enter__(self):
        for key, v in self.opts.items():
            self.old[key] = self.native.get_option(key)
            self.native.set_option(key, v)

    def __exit__(self, *exc):
        for key, v in self.old.items():
            self.native.set_option(key, v)


def _guided_inputs(n, seed):
    Wlo, Hlo, Whi, Hhi = 96, 54, 192, 108                   # exact 2x (the int16 integer first stage), W a multiple of 4
    rng = np.random.default_rng(seed)
    disp = rng.integers(-16, 1000, (n, Hlo, Wlo)).astype(np.int16)
    from scipy.ndimage import gaussian_filter
    guide = np.stack([np.clip(gaussian_filter(rng.integers(0, 256, (Hhi, Whi)).astype(np.float32), 1.5) * 2 - 128, 0, 255) for _ in range(n)]).astype(np.uint8)
    return Wlo, Hlo, Whi, Hhi, disp, guide


def _guided_case(k, route, kind, batch):
    n = 3 if batch else 1
    Wlo, Hlo, Whi, Hhi, disp, guide = _guided_inputs(n, 20 + len(kind))
    N = k.native
    if kind == "f32":
        lo, odt, tdt = k_oracle_free_disp_to_depth(disp), np.float32, None
    elif kind == "disp16":
        lo, odt = disp, np.float32
    else:
        lo, odt = (np.maximum(disp, 0).astype(np.uint16) * 60), np.uint16
    d = k.inp("depth_lo", lo if batch else lo[0], stride=batch)
    g = k.inp("guide", guide if batch else guide[0], stride=batch)
    o = k.out("out", odt, (n, Hhi, Whi))
    ws = k.ws("ws", N.lib().v3d_guided_upscale_ws_bytes(Whi, Hhi) * n, align=WS_ALIGN)
    r, eps = 8, 1e-3
    L = N.lib()
    if not batch:
        fn = lambda lib: lib.v3d_guided_upscale(_p(d), Wlo, Hlo, _p(g), Whi, Hhi, r, eps, _p(o), _p(ws), _stream())
    else:
        entry = {"f32": "v3d_guided_upscale_batch", "disp16": "v3d_guided_upscale_disp16_batch", "u16": "v3d_guided_upscale_u16_batch"}[kind]
        fn = lambda lib: getattr(lib, entry)(_p(d), Wlo, Hlo, d.frame_stride, _p(g), Whi, Hhi, g.frame_stride_bytes, n, r, eps, _p(o), _p(ws), _stream())

    def call(lib):
        with _Options(N, GF_ROUTES[route]):
            return fn(lib)

    def expect():
        import torch
        with _Options(N, GF_ROUTES[route]):
            if kind == "u16":
                got = N.guided_upscale_u16_batch(_dev(N, lo.view(np.int16)), _dev(N, guide), r, eps)
                torch.cuda.synchronize()
                return {"out": _bits(got).view(np.uint16)}
            got = N.guided_upscale_batch(_dev(N, lo), _dev(N, guide), r, eps)
            torch.cuda.synchronize()
            return {"out": _bits(got)}
    return call, expect, None


def case_guided_upscale(k, route):
    return _guided_case(k, route, "f32", False)


def case_guided_upscale_batch(k, route):
    return _guided_case(k, route, "f32", True)


def case_guided_upscale_disp16_batch(k, route):
    return _guided_case(k, route, "disp16", True)


def case_guided_upscale_u16_batch(k, route):
    return _guided_case(k, route, "u16", True)


def case_corr_lookup(k, variant):
    import torch
    route, pattern = variant.rsplit("-p", 1)
    pattern = int(pattern)
    N = k.native
    Cc, h, w, G = 128, 6, 20, 2
    g = torch.Generator().manual_seed(5)
    fl = torch.randn((h, w, Cc), generator=g).bfloat16()
    fr = torch.randn((h, w, Cc), generator=g).bfloat16()
    flow = (torch.rand((2, h, w), generator=g) * 6 - 3).float()
    raw = lambda t: t.view(torch.int16).numpy().view(np.uint16).reshape(h, w * Cc)
    a = k.inp("fl", raw(fl), align=16)                      # the header: fl, fr and ws are read 16 bytes at a time
    b = k.inp("fr", raw(fr), align=16)
    f = k.inp("flow", flow.numpy().reshape(2 * h, w))
    o = k.out("out", np.float32, (G * 9, h * w))
    ws = k.ws("ws", N.lib().v3d_corr_ws_bytes(Cc, h, w), align=WS_ALIGN)

    def call(lib):
        with _Options(N, CORR_ROUTES[route]):
            return lib.v3d_corr_lookup(_p(a), _p(b), _p(f), Cc, h, w, G, pattern, _p(o), _p(ws), _stream())

    def expect():
        with _Options(N, CORR_ROUTES[route]):
            got = N.corr_lookup(fl.cuda(), fr.cuda(), flow.cuda(), G, pattern)
            torch.cuda.synchronize()
            return {"out": _bits(got).reshape(G * 9, h * w)}
    return call, expect, None


def _tracks():
    rng = np.random.default_rng(21)
    n1, n2, lag = 3000, 3500, 137
    base = rng.standard_normal(n2 + 400).astype(np.float32)
    a2 = base[:n2].copy()
    a1 = (base[lag:lag + n1] + 0.05 * rng.standard_normal(n1)).astype(np.float32)
    return a1, a2


def case_xcorr(k, variant):
    N = k.native
    a1, a2 = _tracks()
    x, y = k.inp("a1", a1), k.inp("a2", a2)
    o = k.out("out", np.float32, (a1.size + a2.size - 1,))
    ws = k.ws("ws", N.lib().v3d_xcorr_ws_bytes(a1.size, a2.size), align=WS_ALIGN)
    call = lambda lib: lib.v3d_xcorr(_p(x), a1.size, _p(y), a2.size, _p(o), _p(ws), _stream())
    return call, lambda: {"out": _bits(N.xcorr(_dev(N, a1), _dev(N, a2)))}, None


def case_align_audio(k, variant):
    N = k.native
    a1, a2 = _tracks()
    x, y = k.inp("a1", a1), k.inp("a2", a2)
    o = k.out("result", np.float64, (4,))
    ws = k.ws("ws", N.lib().v3d_xcorr_ws_bytes(a1.size, a2.size), align=WS_ALIGN)
    call = lambda lib: lib.v3d_align_audio(_p(x), a1.size, _p(y), a2.size, _p(o), _p(ws), _stream())
    return call, lambda: {"result": _bits(N.align_audio(_dev(N, a1), _dev(N, a2)))}, None


# ------------------------------------------------------------------------------------------------------------------------
# DIBR, temporal stabilisation, robust range
# ------------------------------------------------------------------------------------------------------------------------
def case_render_stereo_batch(k, variant):
    import stereo_ref as SR
    mode, dims = variant.split("@")
    layout = 0 if mode == "full" else 1
    W, H = (int(v) for v in dims.split("x"))                # test_stereo_gpu's (7, 3), (255, 5), (1000, 4); half SBS needs an even W
    n = 3
    rng = np.random.default_rng(W + layout)
    frames = rng.integers(0, 256, (n, H, W * 3), dtype=np.uint8)
    from scipy.ndimage import gaussian_filter
    depth = np.stack([gaussian_filter(rng.random((H, W)).astype(np.float32), 3.0) for _ in range(n)])
    depth = np.clip((depth - depth.min()) / (depth.max() - depth.min()) * 65535, 0, 65535).astype(np.uint16)
    gl, gr, conv = SR.stereo_gains(24.0, 0.5, 0.5)
    f, d = k.inp("frame_bgr", frames, stride=True), k.inp("depth", depth, stride=True)
    ow = 2 * W if layout == 0 else W
    o = k.out("out_bgr", np.uint8, (n, H, ow * 3))
    call = lambda lib: lib.v3d_render_stereo_batch(_p(f), f.frame_stride_bytes, _p(d), d.frame_stride, n, W, H, gl, gr, conv, layout, _p(o), _stream())
    return call, lambda: {"out_bgr": np.stack([SR.render(frames[i].reshape(H, W, 3), depth[i], gl, gr, conv, layout).reshape(H, -1) for i in range(n)])}, None


def _clip(T, H, W, seed):
    """a small clip with a scene cut in the middle: depth f32 (multiples of 1/16, zeros = invalid) and gray u8"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, W)).astype(np.int64)
    gray = np.stack([np.clip(base + rng.integers(-6, 7, (H, W)), 0, 255) for _ in range(T)])
    gray[T // 2:] = 255 - gray[T // 2:]
    depth = k_oracle_free_disp_to_depth(_disp((T, H, W), seed + 1))
    return depth, gray.astype(np.uint8)


CLIP = (5, 17, 64)                                          # T, H, W: W a multiple of 16, the filter's and the SAD's vector width
CLIP_ODD = (5, 9, 37)


def case_temporal_cuts(k, variant):
    import temporal_ref as TR
    T, H, W = CLIP if variant == "vec" else CLIP_ODD
    _, gray = _clip(T, H, W, 30)
    g = k.inp("gray", gray, stride=True)
    ws = k.ws("ws", 8 * T, align=8)
    o = k.out("cut", np.uint8, (T,))
    call = lambda lib: lib.v3d_temporal_cuts(_p(g), g.frame_stride_bytes, T, W, H, 20, _p(ws), _p(o), _stream())
    return call, lambda: {"cut": TR.cuts(gray, 20)}, None


def case_depth_minmax_batch(k, variant):
    import temporal_ref as TR
    T, H, W = CLIP if variant == "vec" else CLIP_ODD
    depth, _ = _clip(T, H, W, 31)
    d = k.inp("depth", depth, stride=True)
    o = k.out("minmax", np.float32, (T, 2))
    call = lambda lib: lib.v3d_depth_minmax_batch(_p(d), T, H * W, d.frame_stride, _p(o), _stream())
    return call, lambda: {"minmax": TR.minmax(depth)}, None


def case_temporal_range(k, variant):
    import temporal_ref as TR
    T, R, t0, n = 9, 2, 1, 7
    rng = np.random.default_rng(32)
    mm = np.sort(rng.random((T, 2)).astype(np.float32) * 60, axis=1)
    cut = (rng.random(T) < 0.3).astype(np.uint8)
    cut[0] = 0
    m, c = k.inp("minmax", mm), k.inp("cut", cut)
    o = k.out("lohi", np.float32, (n, 2))
    call = lambda lib: lib.v3d_temporal_range(_p(m), _p(c), T, t0, n, R, _p(o), _stream())
    return call, lambda: {"lohi": TR.ranges(mm, cut, R, t0, n)}, None


def case_temporal_filter_batch(k, variant):
    import temporal_ref as TR
    T, H, W = CLIP if variant == "vec" else CLIP_ODD
    depth, gray = _clip(T, H, W, 33)
    cut = TR.cuts(gray, 20)
    R, tau, fill, t0, n = 2, 12, 1, 1, 3
    d, g, c = k.inp("depth", depth, stride=True), k.inp("gray", gray, stride=True), k.inp("cut", cut)
    o = k.out("out", np.float32, (n, H, W))
    call = lambda lib: lib.v3d_temporal_filter_batch(_p(d), d.frame_stride, _p(g), g.frame_stride_bytes, T, W, H, t0, n, R, tau, fill, _p(c), _p(o), _stream())
    return call, lambda: {"out": TR.filter_clip(depth, gray, R, tau, cut, fill, t0, n)}, None


def case_depth_to_u16_range_batch(k, variant):
    import temporal_ref as TR
    n, H, W = CLIP if variant == "vec" else CLIP_ODD
    depth, _ = _clip(n, H, W, 34)
    lohi = TR.minmax(depth)
    lohi[1] = (1.0, 20.0)                                   # a range inside the data: both clamps
    lohi[2] = (5.0, 5.0)                                    # flat
    d, l = k.inp("depth", depth, stride=True), k.inp("lohi", lohi)
    o = k.out("u16", np.uint16, (n, H, W))
    call = lambda lib: lib.v3d_depth_to_u16_range_batch(_p(d), n, H * W, d.frame_stride, _p(l), _p(o), _stream())
    return call, lambda: {"u16": TR.to_u16_range(depth, lohi)}, None


def case_depth_robust_minmax_batch(k, variant):
    import range_ref as RR
    T, H, W = CLIP if variant == "vec" else CLIP_ODD
    depth, _ = _clip(T, H, W, 35)
    depth[0, 0, :5] = 120.0                                 # a handful of outliers above the white point
    d = k.inp("depth", depth, stride=True)
    ws = k.ws("ws", k.native.lib().v3d_depth_robust_minmax_ws_bytes(T), align=16)
    o = k.out("minmax", np.float32, (T, 2))
    call = lambda lib: lib.v3d_depth_robust_minmax_batch(_p(d), T, H * W, d.frame_stride, 9900, _p(ws), _p(o), _stream())
    return call, lambda: {"minmax": RR.robust_minmax(depth, 9900)}, None


# entry -> (case function, variants (one per kernel route / shape class), has a pitch or stride argument)
CASES = {
    # shapes: EDGE_SIZES, the lock-step and the row-march lists of tests/test_sgbm_gpu.py (184 and 192 columns keep the 8-pixel
    # row march and the speckle vector loads in play; 2050 takes 16 pixels per thread)
    "v3d_sgbm_compute": (case_sgbm_compute, ("lockstep-march@184x91", "chains-tiles@184x91", "lockstep-march@253x33", "chains-tiles@505x17",
                                             "lockstep-march@123x181", "lockstep-march@2050x6"), True),
    "v3d_sgbm_compute_batch": (case_sgbm_compute_batch, ("lockstep-march@184x33", "chains-tiles@125x65", "lockstep-march@317x129"), True),
    "v3d_sgbm_debug_cost_volume": (case_sgbm_debug_cost_volume, ("lockstep-march@125x65", "lockstep-march@184x91"), True),
    "v3d_sgbm_debug_raw": (case_sgbm_debug_raw, ("lockstep-march@192x40-noS", "lockstep-march@192x40-S", "chains-tiles@193x33-S"), True),
    "v3d_median3x3_i16": (case_median3x3_i16, ("w264",), False),
    "v3d_filter_speckles": (case_filter_speckles, ("640x33", "300x40", "516x19", "257x1", "1x5"), False),
    # the odd shapes of tests/test_prepost_gpu.py
    "v3d_sbs_to_gray": (case_sbs_to_gray, ("unsqueeze@322x45", "plain@322x45", "unsqueeze@1076x9", "plain@2050x3", "unsqueeze@64x8"), True),
    "v3d_sbs_to_gray_batch": (case_sbs_to_gray_batch, ("unsqueeze@322x45", "plain@1076x9", "unsqueeze@1030x9"), True),
    "v3d_split_sbs": (case_split_sbs, ("unsqueeze@322x45", "plain@322x45", "unsqueeze@1076x9", "plain@1030x9"), True),
    "v3d_bgr_to_gray": (case_bgr_to_gray, ("71x33",), False),
    "v3d_disp_to_depth": (case_disp_to_depth, ("332x20",), False),
    "v3d_depth_to_u16": (case_depth_to_u16, ("332x20",), False),
    "v3d_depth_to_u16_batch": (case_depth_to_u16_batch, ("332x20",), True),
    "v3d_round_to_u16": (case_round_to_u16, ("5306",), False),
    "v3d_mono_blend": (case_mono_blend, ("resize", "same-size"), False),
    "v3d_mono_blend_batch": (case_mono_blend_batch, ("resize", "same-size"), True),
    "v3d_guided_upscale": (case_guided_upscale, tuple(GF_ROUTES), False),
    "v3d_guided_upscale_batch": (case_guided_upscale_batch, tuple(GF_ROUTES), True),
    "v3d_guided_upscale_disp16_batch": (case_guided_upscale_disp16_batch, tuple(GF_ROUTES), True),
    "v3d_guided_upscale_u16_batch": (case_guided_upscale_u16_batch, tuple(GF_ROUTES), True),
    "v3d_corr_lookup": (case_corr_lookup, ("fused-p0", "warp-gemm-p0", "warp-gemm-p1"), False),
    "v3d_xcorr": (case_xcorr, ("3000x3500",), False),
    "v3d_align_audio": (case_align_audio, ("3000x3500",), False),
    "v3d_render_stereo_batch": (case_render_stereo_batch, ("full@255x5", "half@254x5", "full@1000x4", "half@1000x4", "full@7x3"), True),
    "v3d_temporal_cuts": (case_temporal_cuts, ("vec", "odd"), True),
    "v3d_depth_minmax_batch": (case_depth_minmax_batch, ("vec", "odd"), True),
    "v3d_temporal_range": (case_temporal_range, ("t9",), False),
    "v3d_temporal_filter_batch": (case_temporal_filter_batch, ("vec", "odd"), True),
    "v3d_depth_to_u16_range_batch": (case_depth_to_u16_range_batch, ("vec", "odd"), True),
    "v3d_depth_robust_minmax_batch": (case_depth_robust_minmax_batch, ("vec", "odd"), True),
}


def _runs(placements):
    for entry, (_, variants, padded) in CASES.items():
        for v in variants:
            for p in placements:
                if padded or not p.startswith("pad"):
                    yield pytest.param(entry, v, p, id=f"{entry}-{v}-{p}")


_expected = {}


def run_case(native, oracle, entry, variant, place, poison):
    """one guarded call: rc == 0, outputs == expected, nothing else written -> {output name: array}"""
    import torch
    fn = CASES[entry][0]
    k = Kit(place, poison, native, oracle)
    call, expect, finish = fn(k, variant)
    key = (entry, variant)
    if key not in _expected:
        _expected[key] = expect()
    k.arena.fill().snapshot()
    try:
        rc = call(native.lib())
        torch.cuda.synchronize()
    finally:
        if finish is not None:
            finish()
    assert rc == 0, f"{entry} rc={rc}: {native.lib().v3d_last_error().decode()}"
    got = {name: b.get() for name, b in k.outs.items()}
    for name, want in _expected[key].items():
        g, w = got[name], np.asarray(want).reshape(got[name].shape)
        same = g.view(np.uint8) == w.astype(g.dtype, copy=False).view(np.uint8)
        assert w.dtype.itemsize == g.dtype.itemsize and same.all(), \
            f"{entry}[{variant}] {place} poison 0x{poison:02x}: output {name!r} differs in {int((~same).sum())} bytes, first at byte {int(np.flatnonzero(~same.reshape(-1))[0])}"
    k.arena.check()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", list(_runs(PLACEMENTS)))
def test_guarded_call(native, oracle, entry, variant, place):
    run_case(native, oracle, entry, variant, place, 0xA5)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,variant,place", list(_runs(("aligned", "padodd"))))
def test_two_poisons(native, oracle, entry, variant, place):
    """the same call over 0xA5 and over 0xFF (NaN as a float, -1 / 65535 as integers) in the red zones, the padding, the outputs
    and the workspaces: bit-identical outputs, i.e. no unwritten sample, no dependence on workspace content, no read past an input
    that reaches the result"""
    a = run_case(native, oracle, entry, variant, place, 0xA5)
    b = run_case(native, oracle, entry, variant, place, 0xFF)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), f"{entry}[{variant}] {place}: {name!r} depends on the poison"


# ------------------------------------------------------------------------------------------------------------------------
# refusals the header states
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_misaligned_workspaces_are_refused(native):
    """a `void* ws` 8 bytes off a 16-byte boundary (4 off an 8-byte one for v3d_temporal_cuts) and correlation features 2 bytes
    off one: V3D_ERR_ARG before anything is enqueued, outputs untouched"""
    import torch
    L = native.lib()
    k = Kit("aligned", 0xA5, native)
    f32 = k.inp("f32", np.zeros((3, 64, 64), np.float32))
    u8 = k.inp("u8", np.zeros((3, 128, 128), np.uint8))
    i16 = k.inp("i16", np.zeros((3, 64, 64), np.int16))
    bf = k.inp("bf", np.zeros((4, 4 * 64), np.uint16), align=16)
    out = k.out("out", np.float32, (3, 128, 128))
    ws = k.ws("ws", 1 << 20, align=16)
    k.arena.fill().snapshot()
    P, st, bad = C.c_void_p, _stream(), C.c_void_p(ws.ptr + 8)
    calls = {
        "v3d_mono_blend": lambda: L.v3d_mono_blend(P(i16.ptr), 64, 64, P(f32.ptr), 64, 64, 0.7, 0.3, P(out.ptr), bad, st),
        "v3d_mono_blend_batch": lambda: L.v3d_mono_blend_batch(P(i16.ptr), 3, 64, 64, P(f32.ptr), 64, 64, 4096, 0.7, 0.3, P(out.ptr), bad, st),
        "v3d_guided_upscale": lambda: L.v3d_guided_upscale(P(f32.ptr), 64, 64, P(u8.ptr), 128, 128, 8, 1e-3, P(out.ptr), bad, st),
        "v3d_guided_upscale_batch": lambda: L.v3d_guided_upscale_batch(P(f32.ptr), 64, 64, 4096, P(u8.ptr), 128, 128, 16384, 3, 8, 1e-3, P(out.ptr), bad, st),
        "v3d_guided_upscale_disp16_batch": lambda: L.v3d_guided_upscale_disp16_batch(P(i16.ptr), 64, 64, 4096, P(u8.ptr), 128, 128, 16384, 3, 8, 1e-3, P(out.ptr), bad, st),
        "v3d_guided_upscale_u16_batch": lambda: L.v3d_guided_upscale_u16_batch(P(i16.ptr), 64, 64, 4096, P(u8.ptr), 128, 128, 16384, 3, 8, 1e-3, P(out.ptr), bad, st),
        "v3d_corr_lookup ws": lambda: L.v3d_corr_lookup(P(bf.ptr), P(bf.ptr), P(f32.ptr), 64, 2, 2, 1, 0, P(out.ptr), bad, st),
        "v3d_corr_lookup fl": lambda: L.v3d_corr_lookup(P(bf.ptr + 2), P(bf.ptr), P(f32.ptr), 64, 2, 2, 1, 0, P(out.ptr), P(ws.ptr), st),
        "v3d_corr_lookup fr": lambda: L.v3d_corr_lookup(P(bf.ptr), P(bf.ptr + 2), P(f32.ptr), 64, 2, 2, 1, 0, P(out.ptr), P(ws.ptr), st),
        "v3d_xcorr": lambda: L.v3d_xcorr(P(f32.ptr), 1000, P(f32.ptr), 1000, P(out.ptr), bad, st),
        "v3d_align_audio": lambda: L.v3d_align_audio(P(f32.ptr), 1000, P(f32.ptr), 1000, P(out.ptr), bad, st),
        "v3d_temporal_cuts": lambda: L.v3d_temporal_cuts(P(u8.ptr), 16384, 3, 128, 128, 20, P(ws.ptr + 4), P(out.ptr), st),
        "v3d_depth_robust_minmax_batch": lambda: L.v3d_depth_robust_minmax_batch(P(f32.ptr), 3, 4096, 4096, 9900, bad, P(out.ptr), st),
    }
    for name, fn in calls.items():
        assert fn() == -1, f"{name} accepted a misaligned pointer"
        assert b"align" in L.v3d_last_error(), f"{name}: {L.v3d_last_error()}"
    torch.cuda.synchronize()
    assert (out.get().view(np.uint8) == 0xA5).all()
    k.arena.check()


@pytest.mark.gpu
def test_overlapping_frame_strides_are_refused(native):
    """v3d_sgbm_compute_batch and v3d_sbs_to_gray_batch refuse frame_stride < H * pitch when n > 1, like the newer entries;
    n == 1 ignores the stride"""
    import torch
    L = native.lib()
    W, H = 160, 20
    k = Kit("aligned", 0xA5, native)
    g = k.inp("gray", np.zeros((2, H, W + 8), np.uint8))
    s = k.inp("sbs", np.zeros((2, H, W * 3 + 4), np.uint8))
    o = k.out("out", np.int16, (2, H, W))
    k.arena.fill().snapshot()
    P, st = C.c_void_p, _stream()
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2)
    pitch = W + 8
    assert L.v3d_sgbm_compute_batch(m._h, P(g.ptr), P(g.ptr), 2, W, H, pitch, H * pitch - 1, P(o.ptr), st) == -1
    assert b"frame stride" in L.v3d_last_error()
    assert L.v3d_sgbm_compute_batch(m._h, P(g.ptr), P(g.ptr), 2, W, H, pitch, H * W, P(o.ptr), st) == -1
    sp = W * 3 + 4
    assert L.v3d_sbs_to_gray_batch(P(s.ptr), 2, W, H, sp, H * sp - 1, 1, P(o.ptr), P(o.ptr + 2 * H * W), st) == -1
    assert b"frame stride" in L.v3d_last_error()
    torch.cuda.synchronize()
    assert (o.get().view(np.uint8) == 0xA5).all()
    assert L.v3d_sgbm_compute_batch(m._h, P(g.ptr), P(g.ptr), 1, W, H, pitch, 0, P(o.ptr), st) == 0
    assert L.v3d_sbs_to_gray_batch(P(s.ptr), 1, W, H, sp, 0, 1, P(o.ptr), P(o.ptr + H * W), st) == 0
    assert m.sync_errors() == 0
    m.close()
    k.arena.check()


# ------------------------------------------------------------------------------------------------------------------------
# the matcher's own scratch cannot be poisoned from outside: larger-then-smaller geometry on ONE handle instead
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_handle_through_shrinking_and_growing_geometry(native, oracle):
    """one handle (480 x 270 x 3) computes 480x270 n=3, 203x77 n=1, 125x65 n=2, 480x270 n=1, then again after set_lockstep(False)
    and with vdd_dpl 4 and 8: stale rows, strips, run lists and sequence tags of a larger call lie under every smaller one.
    Every frame of every call equals the oracle, no lock-step time-outs."""
    m = native.StereoSGBM(max_width=480, max_height=270, max_batch=3)
    want = {}

    def step(W, H, n, what):
        pairs = [_pair(W, H, 700 + i) for i in range(n)]
        got = _bits(m.compute(_dev(native, np.stack([p[0] for p in pairs])), _dev(native, np.stack([p[1] for p in pairs]))))
        assert m.sync_errors() == 0, what
        for i, p in enumerate(pairs):
            if (W, H, i) not in want:
                want[(W, H, i)] = oracle.sgbm_compute(*p)
            bad = got[i] != want[(W, H, i)]
            assert not bad.any(), f"{what}: {W}x{H} frame {i} of {n}: {int(bad.sum())} px differ, first at {tuple(np.argwhere(bad)[0])}"

    try:
        step(480, 270, 3, "step 1")
        step(203, 77, 1, "step 2")
        step(64 + 61, 65, 2, "step 3")
        step(480, 270, 1, "step 4")
        m.set_lockstep(False)
        step(203, 77, 1, "lockstep off")
        step(480, 270, 3, "lockstep off")
        m.set_lockstep(True)
        m.set_option("vdd_dpl", 4)
        step(64 + 61, 65, 2, "vdd_dpl 4")
        step(480, 270, 1, "vdd_dpl 4")
        m.set_option("vdd_dpl", 8)
        step(203, 77, 1, "vdd_dpl 8")
        step(480, 270, 3, "vdd_dpl 8")
    finally:
        m.close()
