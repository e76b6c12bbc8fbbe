"""v3d_fill_holes_disp16_batch against tests/fill_ref.py, bit for bit, through video_3d_pipeline._native: every size class of the
row kernel (8 / 16 / 32 / 40 pixels per thread, chosen from W + 7), strided, odd-offset and in-place layouts, hole patterns that
cross every thread-run and wave boundary, empty rows, the matcher's own output, and the refusals the header lists."""
import ctypes as C
import os

import numpy as np
import pytest

import fill_ref as FR
import launch_plan as LP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
I = -16

# W x H.  The issue's list, then both sides of every width at which the kernel takes more pixels per thread (W + 7 <= 2048, 4096,
# 8192), then shapes for the empty-row pass: more than one 32-row band, and a source row more than 256 rows away
SIZES = [(1, 1), (7, 1), (63, 5), (64, 3), (65, 3), (257, 33), (1000, 9), (1920, 3), (8192, 2),
         (2041, 2), (2042, 2), (4089, 2), (4090, 2), (8185, 2), (8186, 2), (65, 70), (5, 700)]
LAYOUTS = ("dense", "strided", "odd", "inplace")
RUNS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2049)


def _values(rng, shape):
    d = rng.integers(1, 1024, shape).astype(np.int16)
    d[rng.random(shape) < 0.05] = 0                                   # 0 is a valid disparity
    return d


def _run_pattern(rng, n, H, W):
    """alternating valid and hole runs whose lengths straddle 8, 16, 32 and 40 pixels (a thread's run) and 512 .. 2560 (a wave's)"""
    d = _values(rng, (n, H, W))
    for f in range(n):
        for y in range(H):
            x = int(rng.integers(0, 9))
            while x < W:
                hole = int(rng.choice(RUNS))
                d[f, y, x:x + hole] = rng.choice(np.array([I, -1, -32768], np.int16))
                x += hole + int(rng.choice(RUNS[:12]))
    return d


def patterns(n, H, W, seed):
    rng = np.random.default_rng(seed)
    base = _values(rng, (n, H, W))
    out = {"none": base.copy(), "all": np.full((n, H, W), I, np.int16)}
    p = np.full((n, H, W), I, np.int16); p[:, :, 0] = base[:, :, 0]; out["col0"] = p
    p = np.full((n, H, W), -1, np.int16); p[:, :, -1] = base[:, :, -1]; out["last"] = p
    p = base.copy(); p[:, :, 0::2] = I; out["alt-even"] = p
    p = base.copy(); p[:, :, 1::2] = -32768; out["alt-odd"] = p
    out["runs"] = _run_pattern(rng, n, H, W)
    p = base.copy(); p[:, :, :64] = I; p[rng.random((n, H, W)) < 0.03] = I; out["band+speckle"] = p
    p = base.copy(); p[rng.random((n, H, W)) < 0.5] = I
    p[:, :max(H // 4, 1)] = I                                          # empty rows at the top ...
    p[:, H - max(H // 5, 1):] = -1                                      # ... at the bottom ...
    if H >= 7:
        p[:, H // 2 - 1:H // 2 + 2] = I                                # ... in the middle: 3 rows, the centre one equidistant
    out["empty-rows"] = p
    p = np.full((n, H, W), I, np.int16); p[:, H - 1 - (H - 1) // 8] = base[:, 0]; p[:, H - 1 - (H - 1) // 8, W // 2:] = I
    out["one-row"] = p                                                 # every other row copies it, most from far away
    p = out["band+speckle"].copy(); p[n // 2] = I; out["frame-invalid"] = p
    return out


def run_entry(N, d, layout):
    """d: int16 [n,H,W] host -> the entry's output as a host array; also checks that an out-of-place call left its input alone"""
    import torch
    n, H, W = d.shape
    dev = torch.device("cuda")
    src = torch.from_numpy(d)
    if layout == "dense":
        x = src.to(dev)
        out = N.fill_holes_disp16_batch(x)
    elif layout == "strided":
        stride = H * W + 11
        buf = torch.full((n * stride,), 777, dtype=torch.int16, device=dev)
        x = torch.as_strided(buf, (n, H, W), (stride, W, 1))
        x.copy_(src)
        out = N.fill_holes_disp16_batch(x)
        pad = torch.as_strided(buf, (n, 11), (stride, 1), H * W)
        assert bool((pad == 777).all()), "the padding between the input frames changed"
    elif layout == "odd":
        stride = H * W + 1
        buf = torch.full((1 + n * stride,), 777, dtype=torch.int16, device=dev)
        x = torch.as_strided(buf, (n, H, W), (stride, W, 1), 1)
        x.copy_(src)
        obuf = torch.full((3 + n * H * W + 8,), 555, dtype=torch.int16, device=dev)
        o = obuf[3:3 + n * H * W].view(n, H, W)
        assert x.data_ptr() % 4 == 2 and o.data_ptr() % 4 == 2
        out = N.fill_holes_disp16_batch(x, out=o)
        assert bool((obuf[:3] == 555).all()) and bool((obuf[3 + n * H * W:] == 555).all()), "a store outside the output"
    else:
        x = src.to(dev)
        out = N.fill_holes_disp16_batch(x, out=x)
        assert out.data_ptr() == x.data_ptr()
    got = out.cpu().numpy()
    if layout != "inplace":
        assert np.array_equal(x.cpu().numpy(), d), "an out-of-place call changed its input"
    return got


_cases = {}


def cases(W, H):
    """(n, {pattern: (input, reference)}) of one size: computed once, shared by the four layouts, never written to"""
    if (W, H) not in _cases:
        n = 1 + (W + H) % 3
        _cases[W, H] = n, {name: (d, FR.fill(d)) for name, d in patterns(n, H, W, W * 131 + H).items()}
    return _cases[W, H]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_bit_exact(native, W, H, layout):
    from conftest import mismatch_report
    n, cs = cases(W, H)
    for name, (d, want) in cs.items():
        got = run_entry(native, d, layout)
        assert np.array_equal(got, want), f"{W}x{H} n={n} {layout} {name}: " + mismatch_report(got, want, "filled")


@pytest.mark.parametrize("n,W,H", LP.FILL_BAND_CASES, ids=[f"n{c[0]}" for c in LP.FILL_BAND_CASES])
def test_rows_per_workgroup_above_four(native, n, W, H):
    """k_fill_rows takes clamp(ceil(n H / 2048), 4, 64) rows a workgroup (tests/launch_plan.py): 4 in every sized case above and in
    the 1080p batch; here 5 and 64, over a height that neither divides, so that the last workgroup of a frame has a short band.
    Seven distinct frames repeated in order (frames are independent: the sized cases hold that)"""
    from conftest import mismatch_report
    ps = patterns(7, H, W, n)
    idx = np.arange(n) % 7
    for name in ("runs", "empty-rows", "one-row"):
        want = FR.fill(ps[name])
        assert len({f.tobytes() for f in want}) > 1
        for layout in ("dense", "strided"):
            got = run_entry(native, ps[name][idx], layout)
            assert np.array_equal(got, want[idx]), f"n={n} {layout} {name}: " + mismatch_report(got, want[idx], "filled")


def test_1080p_batch_of_four(native):
    from conftest import mismatch_report
    rng = np.random.default_rng(1080)
    d = _values(rng, (4, 1080, 1920))
    d[:, :, :64] = I
    d[rng.random(d.shape) < 0.04] = I
    for f in range(4):                                                 # occlusion-like bands beside "edges"
        for x0 in rng.integers(64, 1900, 12):
            d[f, int(rng.integers(0, 500)):int(rng.integers(500, 1080)), x0:x0 + int(rng.integers(4, 40))] = I
    d[2, 300:303] = I
    want = FR.fill(d)
    assert (want >= 0).all()
    for layout in ("dense", "inplace"):
        got = run_entry(native, d, layout)
        assert np.array_equal(got, want), layout + ": " + mismatch_report(got, want, "filled")


@pytest.mark.parametrize("golden", ["sgbm_320x180.npz", "prepost_192x64.npz"])
def test_golden_matcher_output(native, golden):
    d = np.ascontiguousarray(np.load(os.path.join(HERE, "golden", golden))["disp"]).astype(np.int16)
    assert d.ndim == 2 and (d < 0).any() and (d >= 0).any()
    want = FR.fill_frame(d)
    for layout in LAYOUTS:
        assert np.array_equal(run_entry(native, d[None], layout)[0], want), layout
    assert (want >= 0).all() and np.array_equal(want[d >= 0], d[d >= 0])


def test_matcher_output_on_the_temporal_clip(native, oracle):
    """the matcher's own frame through the entry; the filled holes right of the 64-column band against the clip's ground truth:
    mean |error| <= 2.0 px and at most 5 % off by more than 2 px (the oracle matcher with the reference gives 1.22 px and 2.5 %;
    the matcher is bit-exact to the oracle, the margin only absorbs a change of the synthetic clip)"""
    from video_3d_pipeline import synthetic as syn
    L, R, G = syn.temporal_clip(480, 270, 2, scene_seed=1)
    m = native.StereoSGBM(480, 270, 1)
    try:
        disp = m.compute(native.to_device(L[1]), native.to_device(R[1]))
        assert m.sync_errors() == 0
        d = disp.cpu().numpy().reshape(270, 480)
        filled = native.fill_holes_disp16_batch(disp.reshape(1, 270, 480)).cpu().numpy()[0]
    finally:
        m.close()
    assert np.array_equal(d, oracle.sgbm_compute(L[1], R[1]))
    assert np.array_equal(filled, FR.fill_frame(d))
    holes = d < 0
    holes[:, :64] = False
    err = np.abs(filled[holes].astype(np.float64) / 16.0 - G[1][holes])
    print(f"{int(holes.sum())} holes at x >= 64: mean |error| {err.mean():.3f} px, {100 * (err > 2).mean():.2f} % off by more than 2 px")
    assert holes.sum() > 1000
    assert err.mean() <= 2.0
    assert (err > 2).mean() <= 0.05


def test_idempotent_on_the_device(native):
    d = patterns(2, 33, 257, 5)["empty-rows"]
    once = run_entry(native, d, "dense")
    assert np.array_equal(run_entry(native, once, "inplace"), once)


# ---------------------------------------------------------------- refusals

ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_refusals(native):
    import torch
    lib = native.lib()
    W, H, n = 40, 6, 2
    buf = torch.full((n * (W * H + 8) + 16,), 99, dtype=torch.int16, device="cuda")
    out = torch.full((n * W * H,), 99, dtype=torch.int16, device="cuda")
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, w = buf.data_ptr(), out.data_ptr(), ws.data_ptr()
    assert w % 16 == 0

    def call(disp=p, stride=W * H, n_=n, W_=W, H_=H, out_=o, ws_=w):
        return lib.v3d_fill_holes_disp16_batch(C.c_void_p(disp), stride, n_, W_, H_, C.c_void_p(out_), C.c_void_p(ws_), stream)

    assert call() == 0
    assert call(stride=W * H + 8) == 0
    assert call(disp=p, out_=p) == 0                                           # in place, dense batch
    assert call(disp=p, out_=p, n_=1, stride=7) == 0                           # in place, one frame: the stride is ignored
    arg = dict(null_in=dict(disp=None), null_out=dict(out_=None), null_ws=dict(ws_=None), n0=dict(n_=0), n_neg=dict(n_=-1),
               n_big=dict(n_=65536), w0=dict(W_=0), h0=dict(H_=0), w_neg=dict(W_=-3), h_neg=dict(H_=-3),
               short_stride=dict(stride=W * H - 1), ws_misaligned=dict(ws_=w + 8), ws_misaligned2=dict(ws_=w + 2),
               inplace_strided=dict(out_=p, stride=W * H + 8))
    for name, kw in arg.items():
        assert call(**kw) == ERR_ARG, name
        assert lib.v3d_last_error()
    assert call(n_=1, stride=0) == 0                                           # one frame ignores the stride
    for name, kw in dict(wide=dict(W_=8193, n_=1), tall=dict(H_=65536, n_=1)).items():
        assert call(**kw) == ERR_UNSUPPORTED, name
    assert call(W_=8193, n_=0) == ERR_ARG                                      # an argument error comes first
    torch.cuda.synchronize()
    assert bool((buf[n * (W * H + 8):] == 99).all())
    # the workspace size: 0 for what the entry refuses, else one flag per row rounded up to 16 bytes
    wsb = lib.v3d_fill_holes_ws_bytes
    assert wsb(1, 1) == 16 and wsb(2, 1080) == 2160 and wsb(3, 11) == 48 and wsb(65535, 65535) == (65535 * 65535 + 15) // 16 * 16
    for n_, H_ in ((0, 5), (-1, 5), (65536, 5), (1, 0), (1, -2), (1, 65536)):
        assert wsb(n_, H_) == 0, (n_, H_)
    # the binding refuses what the entry would misread
    with pytest.raises(native.NativeError):
        native.fill_holes_disp16_batch(torch.zeros((1, 4, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(native.NativeError):
        native.fill_holes_disp16_batch(torch.zeros((1, 4, 4), dtype=torch.int16, device="cuda"), out=torch.zeros((1, 4, 5), dtype=torch.int16, device="cuda"))
    with pytest.raises(native.NativeError):
        native.fill_holes_disp16_batch(torch.zeros((2, 40, 4), dtype=torch.int16, device="cuda"), ws=torch.zeros(16, dtype=torch.uint8, device="cuda"))
