"""`--temporal-motion` on the MI355X: the block-matching fields, the compensated residual and cuts, the compensated filter, the
streaming driver and the one-pass pipeline against the NumPy contract (tests/temporal_mc_ref.py), bit for bit."""
import json

import numpy as np
import pytest
import torch

import stereo_ref as SR
import temporal_mc_ref as MR
import temporal_ref as TR
from conftest import mismatch_report

pytestmark = pytest.mark.gpu


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _strided(a, pad):
    """[T,H,W] array -> device tensor whose frames lie `pad` elements further apart than their size"""
    T, H, W = a.shape
    buf = torch.zeros((T, H * W + pad), dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
    buf[:, :H * W] = _dev(a.reshape(T, H * W))
    return buf[:, :H * W].view(T, H, W)


def _moving_gray(rng, T, H, W, shift=(2, -1), noise=5):
    """a smooth texture that moves by `shift` pixels per frame, plus noise: motion a search can find"""
    m = 2 + max(abs(shift[0]), abs(shift[1])) * T
    big = rng.integers(0, 256, (H + 2 * m, W + 2 * m)).astype(np.int64)
    big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, (1, 1), (0, 1))) // 4
    g = np.stack([big[m + shift[1] * t:m + shift[1] * t + H, m + shift[0] * t:m + shift[0] * t + W] for t in range(T)])
    return np.clip(g + rng.integers(-noise, noise + 1, g.shape), 0, 255).astype(np.uint8)


def _depth_clip(rng, T, H, W):
    d = (rng.integers(1, 1024, (T, H, W)) / 16.0).astype(np.float32)
    d[rng.random((T, H, W)) < 0.2] = 0.0
    return d


def _check_motion(native, gray, S, c=20, dev=None, what=""):
    fwd, bwd, resid, cut = native.temporal_motion(_dev(gray) if dev is None else dev, S, c)
    F, Bk, want_resid = MR.fields(gray, S)
    assert not mismatch_report(fwd.cpu().numpy(), F, f"forward field {what}")
    assert not mismatch_report(bwd.cpu().numpy(), Bk, f"backward field {what}")
    assert np.array_equal(resid.cpu().numpy().astype(np.uint64), want_resid), what
    assert np.array_equal(cut.cpu().numpy(), MR.cuts(want_resid, c, gray.shape[2], gray.shape[1])), what
    return F, Bk, want_resid


# ---------------------------------------------------------------- the fields, the residual, the cuts

@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17), (33, 19)])
def test_motion_small_sizes(native, size):
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    for S in (1, 2, 5):
        _check_motion(native, _moving_gray(rng, 3, H, W), S, what=f"{W}x{H} S={S}")
    _check_motion(native, rng.integers(0, 256, (3, H, W), dtype=np.uint8), 3, what=f"{W}x{H} white noise")


@pytest.mark.parametrize("S", [1, 32])
def test_motion_search_radius_limits(native, S):
    rng = np.random.default_rng(S)
    shift = (1, 0) if S == 1 else (-27, 13)
    g = _moving_gray(rng, 3, 48, 80, shift=shift)
    F, Bk, _ = _check_motion(native, g, S, what=f"80x48 S={S}")
    assert tuple(F[0, 1, 2]) == (-shift[0], -shift[1]) and tuple(Bk[1, 1, 2]) == shift      # a block whose match lies inside the frame
    # black against white: the largest SAD a block has, every candidate tied on it
    g = np.zeros((2, 16, 32), np.uint8)
    g[1] = 255
    _, _, resid = _check_motion(native, g, S, c=255, what="black / white")
    assert resid[1] == 2 * 65280


def test_motion_odd_width_strides_and_unaligned_views(native):
    rng = np.random.default_rng(5)
    T, H, W, S = 4, 20, 70, 4                                 # W no multiple of 4: rows start at every alignment
    g = _moving_gray(rng, T, H, W)
    g[3] = 255 - g[3]                                         # a scene change the matcher cannot explain
    F, Bk, resid = _check_motion(native, g, S, what="70x20")
    assert list(MR.cuts(resid, 20, W, H)) == [0, 0, 0, 1]
    for pad in (1, 7, 16):
        _check_motion(native, g, S, dev=_strided(g, pad), what=f"frame stride + {pad}")
    buf = torch.zeros(T * H * W + 3, dtype=torch.uint8, device="cuda")
    for off in (1, 2, 3):
        buf[off:off + T * H * W] = _dev(g.reshape(-1))
        _check_motion(native, g, S, dev=buf[off:off + T * H * W].view(T, H, W), what=f"view at byte {off}")
    # thresholds around the residual: resid == c*W*H is no cut, one level less is
    g2 = np.zeros((2, 4, 5), np.uint8)
    g2[1] = 20
    for c in (19, 20, 21):
        _, _, cut = native.temporal_motion(_dev(g2), 2, c)[1:]
        assert list(cut.cpu().numpy()) == [0, int(c < 20)]


def test_motion_single_frame(native):
    g = np.random.default_rng(6).integers(0, 256, (1, 19, 33), dtype=np.uint8)
    fwd, bwd, resid, cut = native.temporal_motion(_dev(g), 8)
    assert not fwd.any() and not bwd.any() and not resid.any() and not cut.any()
    _check_motion(native, g, 8, what="T=1")


_pan = {}


def _pan_clip():
    """320x120x9 under a pan of 5 px per frame with a scene change at frame 5, and the contract's fields at S = 16 (once)"""
    if not _pan:
        from video_3d_pipeline import synthetic as syn
        L, Rr, _ = syn.temporal_pan_clip(320, 120, 9, 5, cut_at=5)
        F, Bk, resid = MR.fields(L, 16)
        _pan.update(L=L, R=Rr, F=F, Bk=Bk, resid=resid, cut=MR.cuts(resid, 20, 320, 120))
    return _pan


def test_motion_on_the_panning_clip(native):
    p = _pan_clip()
    fwd, bwd, resid, cut = native.temporal_motion(_dev(p["L"]), 16, 20)
    assert not mismatch_report(fwd.cpu().numpy(), p["F"], "forward field") and not mismatch_report(bwd.cpu().numpy(), p["Bk"], "backward field")
    assert np.array_equal(resid.cpu().numpy().astype(np.uint64), p["resid"])
    assert list(cut.cpu().numpy()) == list(p["cut"]) == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert list(native.temporal_cuts(_dev(p["L"]), 20).cpu().numpy()) == [0] + [1] * 8      # what the uncompensated rule makes of a pan
    inner = p["F"][:4, 1:-1, 2:-2]
    assert (inner[..., 0] == -5).mean() > 0.8 and (inner[..., 1] == 0).mean() > 0.9          # the pan itself


def test_motion_refusals(native):
    g = _dev(np.zeros((2, 8, 8), np.uint8))
    for S in (0, 33, 1.5, True):
        with pytest.raises(ValueError):
            native.temporal_motion(g, S)
    with pytest.raises(ValueError):
        native.temporal_motion(g, 4, 257)
    L, P = native.lib(), lambda t: t.data_ptr()
    mv, resid, cut = torch.zeros(8, dtype=torch.int16, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.uint8, device="cuda")
    assert L.v3d_temporal_motion(P(g), 64, 2, 8, 8, 0, 20, P(mv), P(mv), P(resid), P(cut), None) == -1
    assert L.v3d_temporal_motion(P(g), 64, 2, 8, 8, 33, 20, P(mv), P(mv), P(resid), P(cut), None) == -1
    assert L.v3d_temporal_motion(P(g), 63, 2, 8, 8, 4, 20, P(mv), P(mv), P(resid), P(cut), None) == -1
    assert L.v3d_temporal_motion(P(g), 64, 2, 8, 8, 4, 20, P(mv), P(mv), P(resid) + 4, P(cut), None) == -1
    assert L.v3d_temporal_motion(P(g), 64, 2, 8, 8, 4, 20, None, P(mv), P(resid), P(cut), None) == -1
    torch.cuda.synchronize()
    assert not mv.any() and not resid.any() and not cut.any()


# ---------------------------------------------------------------- the compensated filter

def _check_filter(native, depth, gray, R, tau, cut, F, Bk, fill, t0=0, n=None, pad=(0, 0), what=""):
    d = _strided(depth, pad[0]) if pad[0] else _dev(depth)
    g = _strided(gray, pad[1]) if pad[1] else _dev(gray)
    got = native.temporal_filter_mc_batch(d, g, R, tau, _dev(cut), _dev(F), _dev(Bk), fill, t0, n).cpu().numpy()
    want = MR.filter_clip(depth, gray, R, tau, cut, F, Bk, fill, t0, n)
    rep = mismatch_report((got * 16).astype(np.int64), (want * 16).astype(np.int64), what)
    assert not rep and np.array_equal(got, want), rep


@pytest.mark.parametrize("size", [(64, 20), (260, 33), (37, 9), (1, 1), (70, 17)])
def test_filter_both_routes(native, size):
    """widths the vector route takes (a multiple of 4, aligned frames) and widths it cannot; the matcher's own fields and random
    ones, which send taps outside the frame on every side; fill on and off; a cut inside the window; odd frame strides"""
    W, H = size
    rng = np.random.default_rng(W * 7 + H)
    T, S = 6, 4
    gray, depth = _moving_gray(rng, T, H, W), _depth_clip(rng, T, H, W)
    F, Bk, _ = MR.fields(gray, S)
    Fr, Br = rng.integers(-S, S + 1, F.shape).astype(np.int16), rng.integers(-S, S + 1, F.shape).astype(np.int16)
    none, cut = np.zeros(T, np.uint8), np.zeros(T, np.uint8)
    cut[3] = 1
    _check_filter(native, depth, gray, 2, 12, none, F, Bk, 1, what=f"{W}x{H} matcher fields")
    _check_filter(native, depth, gray, 2, 12, cut, F, Bk, 0, what=f"{W}x{H} matcher fields, a cut, no fill")
    _check_filter(native, depth, gray, 2, 255, none, Fr, Br, 1, what=f"{W}x{H} random fields")
    _check_filter(native, depth, gray, 1, 1, cut, Fr, Br, 0, 1, 4, what=f"{W}x{H} random fields, targets 1..4")
    for pad in ((4, 4), (1, 3), (0, 5)):
        _check_filter(native, depth, gray, 2, 12, cut, Fr, Br, 1, 2, 3, pad, what=f"{W}x{H} pad {pad}")


def test_filter_radius_eight_and_the_largest_vectors(native):
    rng = np.random.default_rng(9)
    T, H, W = 12, 40, 300
    gray, depth = _moving_gray(rng, T, H, W, shift=(3, 1)), _depth_clip(rng, T, H, W)
    F, Bk, _ = MR.fields(gray, 4)
    cut = np.zeros(T, np.uint8)
    cut[9] = 1
    _check_filter(native, depth, gray, 8, 12, cut, F, Bk, 1, what="R=8 matcher fields")
    big = np.zeros_like(F)
    big[..., 0], big[..., 1] = 32, -32                       # |m| reaches R*S = 256: far outside a 40-row frame
    _check_filter(native, depth, gray, 8, 12, np.zeros(T, np.uint8), big, -big, 1, what="R=8, S=32 everywhere")


def test_filter_pan_32_on_a_64_wide_clip(native):
    """half the frame leaves per step: two steps away every tap lies outside and has weight 0"""
    from video_3d_pipeline import synthetic as syn
    L, _, _ = syn.temporal_pan_clip(64, 32, 5, 32, sigma=2.0)
    depth = _depth_clip(np.random.default_rng(10), 5, 32, 64)
    F, Bk, resid = _check_motion(native, L, 32, what="64x32 pan 32")
    assert (F[:4, :, 2:, 0] == -32).mean() > 0.7              # the right half of frame t is the left half of frame t+1
    cut = MR.cuts(resid, 20, 64, 32)
    for fill in (0, 1):
        _check_filter(native, depth, L, 2, 12, cut, F, Bk, fill, what=f"pan 32 fill={fill}")
        _check_filter(native, depth, L, 2, 12, np.zeros(5, np.uint8), F, Bk, fill, what=f"pan 32 without cuts fill={fill}")


def test_zero_fields_equal_the_uncompensated_entry(native):
    rng = np.random.default_rng(12)
    for (T, H, W, R, fill) in ((5, 33, 256, 2, 1), (4, 9, 37, 1, 0), (10, 20, 64, 8, 1)):
        gray, depth = _moving_gray(rng, T, H, W), _depth_clip(rng, T, H, W)
        cut = np.zeros(T, np.uint8)
        cut[T // 2] = 1
        z = torch.zeros((T, -(-H // 16), -(-W // 16), 2), dtype=torch.int16, device="cuda")
        d, g, c = _dev(depth), _dev(gray), _dev(cut)
        got = native.temporal_filter_mc_batch(d, g, R, 12, c, z, z, fill)
        assert torch.equal(got, native.temporal_filter_batch(d, g, R, 12, c, fill)), (T, H, W, R)


def test_both_filter_entries_refuse_the_same_arguments_alike(native):
    """one table of bad arguments: v3d_temporal_filter_batch and v3d_temporal_filter_mc_batch return the same code, leave the
    same v3d_last_error text and write nothing; the compensated entry also refuses null and odd-address fields"""
    L, P = native.lib(), lambda t: t.data_ptr()
    T, H, W = 2, 8, 8
    depth = torch.ones((T, H, W), dtype=torch.float32, device="cuda")
    gray = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
    cut = torch.zeros(T, dtype=torch.uint8, device="cuda")
    mv = torch.zeros((T, 1, 1, 2), dtype=torch.int16, device="cuda")
    out = torch.full((T, H, W), -7.5, dtype=torch.float32, device="cuda")
    good = dict(depth=P(depth), ds=H * W, gray=P(gray), gs=H * W, T=T, W=W, H=H, t0=0, n=T, R=1, tau=12, fill=1, cut=P(cut), out=P(out))

    def plain(a):
        rc = L.v3d_temporal_filter_batch(a["depth"], a["ds"], a["gray"], a["gs"], a["T"], a["W"], a["H"], a["t0"], a["n"], a["R"],
                                         a["tau"], a["fill"], a["cut"], a["out"], None)
        return rc, L.v3d_last_error()

    def comp(a, fwd=P(mv), bwd=P(mv)):
        rc = L.v3d_temporal_filter_mc_batch(a["depth"], a["ds"], a["gray"], a["gs"], a["T"], a["W"], a["H"], a["t0"], a["n"], a["R"],
                                            a["tau"], a["fill"], a["cut"], fwd, bwd, a["out"], None)
        return rc, L.v3d_last_error()

    table = [(dict(depth=None), b"null pointer"), (dict(gray=None), b"null pointer"), (dict(cut=None), b"null pointer"),
             (dict(out=None), b"null pointer"), (dict(T=0), b"bad targets"), (dict(n=T + 1), b"bad targets"),
             (dict(t0=1), b"bad targets"), (dict(R=9), b"radius 9"), (dict(tau=0), b"tau 0"), (dict(tau=256), b"tau 256"),
             (dict(fill=2), b"fill must be 0 or 1"), (dict(ds=H * W - 1), b"frame stride"), (dict(gs=H * W - 1), b"frame stride")]
    for bad, text in table:
        a = dict(good, **bad)
        got_plain, got_comp = plain(a), comp(a)
        assert got_plain == got_comp and got_plain[0] == -1 and text in got_plain[1], (bad, got_plain, got_comp)
    for kw, text in ((dict(fwd=None), b"null pointer"), (dict(bwd=None), b"null pointer"), (dict(fwd=P(mv) + 1), b"2-byte aligned"),
                     (dict(bwd=P(mv) + 1), b"2-byte aligned")):
        rc, err = comp(good, **kw)
        assert rc == -1 and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert (out == -7.5).all()


def test_filter_on_the_panning_clip(native):
    p = _pan_clip()
    m = native.StereoSGBM(320, 120, 9)
    depth = native.disp_to_depth(m.compute(_dev(p["L"]), _dev(p["R"]))).cpu().numpy()
    m.close()
    assert (depth > 0).mean() > 0.5
    _check_filter(native, depth, p["L"], 2, 12, p["cut"], p["F"], p["Bk"], 1, what="pan 5, R=2")


# ---------------------------------------------------------------- the streaming driver and the pipeline

def test_streaming_driver_equals_one_whole_clip_call(native):
    from video_3d_pipeline.depth import HipStereoBackend
    from video_3d_pipeline.temporal import TemporalStabilizer
    be = HipStereoBackend()
    rng = np.random.default_rng(13)
    T, H, W, S = 9, 40, 96, 6
    gray, depth = _moving_gray(rng, T, H, W, shift=(4, 1)), _depth_clip(rng, T, H, W)
    gray[5:] = 255 - gray[5:]
    dd, gd = _dev(depth), _dev(gray)
    for R in (1, 2):
        want = MR.stabilize(depth, gray, R, S)
        assert (want != TR.stabilize(depth, gray, R)).any()
        whole = _u16(be.temporal_stabilize(dd, gd, 0, T, R, 12, 20, True, motion_search=S))
        assert not mismatch_report(whole, want, f"whole clip R={R}")
        assert np.array_equal(_u16(be.temporal_stabilize(dd, gd, 0, T, R, 12, 20, True)), TR.stabilize(depth, gray, R))
        for step in (1, 2, 3, 5):
            st = TemporalStabilizer(be, R, motion_search=S)
            parts = []
            for i in range(0, T, step):
                out = st.push(dd[i:i + step].clone(), gd[i:i + step].clone())
                if out is not None:
                    parts.append(_u16(out))
            out = st.finish()
            if out is not None:
                parts.append(_u16(out))
            assert np.array_equal(np.concatenate(parts), want), (R, step)


def test_pipeline_with_temporal_motion_and_stereo_output(native, tmp_path):
    """one-pass pipeline, --temporal-radius 2 --temporal-motion 16 --stereo-output on a panning clip: the 1080p-side u16 maps
    equal the NumPy contract on the backend's own per-frame depth and left gray, the 4K maps the guided entry on those samples,
    the 3D frames tests/stereo_ref.py on the 4K frames and maps"""
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.pipeline import HipPipelineBackend, SbsTo4kDepthPipeline
    from video_3d_pipeline.utils import iter_frames, read_png16
    SW, SH, T = 320, 64, 7
    sbs = syn.temporal_pan_sbs_clip(SW, SH, T, 6, cut_at=4)
    v4k = np.random.default_rng(4).integers(0, 256, (T, 2 * SH, 2 * SW, 3), dtype=np.uint8)
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)

    be = HipPipelineBackend()
    depth = be.sbs_to_disparity(list(sbs), True).cpu().numpy()
    gray = be.left_gray(T).cpu().numpy()
    want_lo = MR.stabilize(depth, gray, 2, 16)
    assert list(MR.cuts(MR.fields(gray, 16)[2], 20, SW, SH)) == [0, 0, 0, 0, 1, 0, 0]
    luma = be.guide_luma(list(v4k), 2 * SH, 2 * SW, T)
    want_hi = _u16(native.guided_upscale_u16_batch(_dev(want_lo.view(np.int16)), luma, 8, 1e-3))
    gains = SR.stereo_gains()

    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / "w"), batch_size=3, stereo_only=True, guide_batch=3, temporal_radius=2,
                                temporal_motion=16)
    out = pipe.run(str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"), output_path=str(tmp_path / "d.json"), keep_depth_maps=True,
                   stereo_output=str(tmp_path / "s.json"))
    man = json.loads(open(out).read())
    assert man["count"] == T and man["temporal"] == {"radius": 2, "tau": 12, "cut_threshold": 20, "fill": True, "motion_search": 16}
    cache = pipe.extractor.get_cache_path(str(tmp_path / "sbs.npy"), 0, T)
    sman = json.loads((tmp_path / "s.json").read_text())
    got3d = list(iter_frames(sman["frames_dir"]))
    assert sman["count"] == T == len(got3d)
    for i in range(T):
        assert not mismatch_report(read_png16(cache / f"depth_{i:06d}.png"), want_lo[i], f"1080p-side map {i}")
        assert not mismatch_report(read_png16(f"{man['frames_dir']}/depth4k_{i:06d}.png"), want_hi[i], f"4K map {i}")
        assert np.array_equal(got3d[i], SR.render(v4k[i], want_hi[i], *gains, SR.FULL_SBS)), i
    assert (want_lo != TR.stabilize(depth, gray, 2)).any()
