"""GPU parity of the SGBM hot path (depth.py:315-341) against the CPU oracle, stage by stage.
Bar: bit-exact int16 (SURVEY.md 8d asks +-1 level; the integer pipeline is reproduced exactly)."""
import numpy as np
import pytest

from conftest import mismatch_report, textured_pair

pytestmark = pytest.mark.gpu

SIZES = [(160, 96), (320, 180), (203, 77), (480, 270), (960, 540)]      # (960, 540) = BASELINE configs[0] geometry


def _dev(native, a):
    return native.to_device(a)


@pytest.fixture(scope="module")
def matcher(native):
    m = native.StereoSGBM(max_width=1920, max_height=1080, max_batch=2)
    yield m
    m.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_cost_volume_bit_exact(native, oracle, matcher, W, H):
    L, R = textured_pair(W, H, seed=W + H)
    want = oracle.cost_volume(L, R)
    got = matcher.debug_cost_volume(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert not mismatch_report(got, want, "C"), mismatch_report(got, want, "C")


@pytest.mark.parametrize("W,H", SIZES)
def test_raw_disparity_bit_exact(native, oracle, matcher, W, H):
    L, R = textured_pair(W, H, seed=7 * W + H)
    want = oracle.sgbm_raw(L, R)
    got = matcher.debug_raw(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert not mismatch_report(got, want, "raw disp"), mismatch_report(got, want, "raw disp")


@pytest.mark.parametrize("W,H", SIZES)
def test_full_compute_bit_exact(native, oracle, matcher, W, H):
    L, R = textured_pair(W, H, seed=3 * W + H)
    want = oracle.sgbm_compute(L, R)
    got = matcher.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert not mismatch_report(got, want, "disp16"), mismatch_report(got, want, "disp16")
    assert (got[:, :64] == -16).all()


# sizes that sit on the kernels' tile edges: k_cost strips of 60 cost columns x 90-row bands, k_prefilter 252 columns x
# 64-row bands, lrcheck/median 64 x 16 tiles, the speckle filter's 16-row merge bands, k_vdd/k_hfused row groups
EDGE_SIZES = [(64 + 120, 91), (64 + 61, 65), (253, 33), (505, 17), (64 + 59, 181), (317, 129)]


@pytest.mark.parametrize("W,H", EDGE_SIZES)
def test_tile_edge_sizes_bit_exact(native, oracle, W, H):
    L, R = textured_pair(W, H, seed=11 * W + H)
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2)
    want = oracle.sgbm_compute(L, R)
    got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    cv = m.debug_cost_volume(_dev(native, L), _dev(native, R)).cpu().numpy()
    m.close()
    assert np.array_equal(cv, oracle.cost_volume(L, R))
    assert not mismatch_report(got, want, "disp16"), mismatch_report(got, want, "disp16")


def test_mode_hh_8_paths(native, oracle):
    W, H = 240, 100
    L, R = textured_pair(W, H, seed=5)
    m = native.StereoSGBM(max_width=W, max_height=H, mode=1)
    want = oracle.sgbm_compute(L, R, oracle.default_params(mode=1))
    got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    m.close()
    assert not mismatch_report(got, want, "disp16 HH"), mismatch_report(got, want, "disp16 HH")


def test_hh_saturation_large_p2(native, oracle):
    """8 paths with a huge P2 drive S into int16 saturation (SURVEY 8c known-answer 6)"""
    W, H = 200, 60
    L, R = textured_pair(W, H, seed=11)
    kw = dict(mode=1, P1=3000, P2=12000)
    m = native.StereoSGBM(max_width=W, max_height=H, **kw)
    want = oracle.sgbm_compute(L, R, oracle.default_params(**kw))
    got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    m.close()
    assert not mismatch_report(got, want, "disp16 sat"), mismatch_report(got, want, "disp16 sat")


def test_known_answers(native, matcher):
    """shifted texture -> k; identical -> 0; constant -> 0; first 64 columns invalid"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(0)
    H, W, k = 48, 200, 7
    T = gaussian_filter(rng.integers(0, 256, (H, W + 64)).astype(np.float32), 1.2)
    T = np.clip((T - 127) * 3 + 127, 0, 255).astype(np.uint8)
    L = np.ascontiguousarray(T[:, 32:32 + W])
    R = np.ascontiguousarray(T[:, 32 + k:32 + k + W])
    d = matcher.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    inter = d[8:-8, 64 + 16:-16]
    assert (inter >= 0).all() and (((inter + 8) >> 4) == k).all() and (np.abs(inter - 16 * k) <= 8).all()
    assert (d[:, :64] == -16).all()
    d0 = matcher.compute(_dev(native, L), _dev(native, L)).cpu().numpy()
    assert (d0[:, 64:] == 0).all()
    c = np.full((H, W), 100, np.uint8)
    dc = matcher.compute(_dev(native, c), _dev(native, c)).cpu().numpy()
    assert (dc[:, 64:] == 0).all() and (dc[:, :64] == -16).all()


def test_batch_equals_single(native, matcher):
    W, H = 320, 180
    pairs = [textured_pair(W, H, seed=s) for s in (21, 22)]
    Ls = _dev(native, np.stack([p[0] for p in pairs]))
    Rs = _dev(native, np.stack([p[1] for p in pairs]))
    both = matcher.compute(Ls, Rs).cpu().numpy()
    for i in range(2):
        one = matcher.compute(Ls[i].contiguous(), Rs[i].contiguous()).cpu().numpy()
        assert not mismatch_report(both[i], one, f"batch[{i}]"), mismatch_report(both[i], one, f"batch[{i}]")


def test_chain_lane_mappings_agree(native, oracle):
    """both k_chain lane mappings (8 and 4 disparities per lane) give the oracle's bits"""
    W, H = 230, 90
    L, R = textured_pair(W, H, seed=31)
    want = oracle.sgbm_compute(L, R)
    for dpl in (8, 4):
        m = native.StereoSGBM(max_width=W, max_height=H, options={"lockstep": 0, "chain_dpl": dpl})   # the per-direction k_chain launches
        got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
        m.close()
        assert not mismatch_report(got, want, f"dpl={dpl}"), mismatch_report(got, want, f"dpl={dpl}")


def test_median_and_speckle_stages(native, oracle):
    rng = np.random.default_rng(3)
    H, W = 120, 260
    img = (rng.integers(0, 64, (H, W)) * 16).astype(np.int16)
    img[rng.random((H, W)) < 0.3] = -16
    got = native.median3x3(_dev(native, img)).cpu().numpy()
    assert not mismatch_report(got, oracle.median3x3(img), "median")
    # blobs around the 100-pixel threshold: 10x10 removed, 101 px kept (SURVEY 8c known-answer 9)
    sp = np.full((H, W), -16, np.int16)
    sp[5:15, 5:15] = 160
    sp[30:40, 30:40] = 320
    sp[40, 30] = 320                                   # 101 px
    sp[60:100, 100:200] = (rng.integers(0, 40, (40, 100)) * 16).astype(np.int16)
    sp[70:75, 120:180] = 3000                          # a plateau cut off by > 512 steps
    got = native.filter_speckles(_dev(native, sp)).cpu().numpy()
    want = oracle.filter_speckles(sp)
    assert not mismatch_report(got, want, "speckle")
    assert (got[5:15, 5:15] == -16).all() and (got[30:40, 30:40] == 320).all()
    noisy = native.filter_speckles(_dev(native, img)).cpu().numpy()
    assert not mismatch_report(noisy, oracle.filter_speckles(img), "speckle noisy")


def test_rejects_bad_arguments(native):
    with pytest.raises(native.NativeError):
        native.StereoSGBM(max_width=640, max_height=480, numDisparities=128)
    with pytest.raises(native.NativeError):
        native.StereoSGBM(max_width=640, max_height=480, P2=20000)   # beyond the packed int16 recurrence
    m = native.StereoSGBM(max_width=320, max_height=100)
    big = native.to_device(np.zeros((200, 320), np.uint8))
    with pytest.raises(native.NativeError):
        m.compute(big, big)
    narrow = native.to_device(np.zeros((50, 60), np.uint8))
    with pytest.raises(native.NativeError):
        m.compute(narrow, narrow)
    m.close()


def test_full_size_1080p_properties(native, oracle, matcher):
    """BASELINE size: bit-exact on a band the oracle finishes quickly is covered above; at full
    1920x1080 check size-independent properties + a row band against the oracle."""
    from video_3d_pipeline import synthetic as syn
    L, R = syn.gray_pair(1920, 1080, 0)
    d = matcher.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert d.shape == (1080, 1920) and (d[:, :64] == -16).all()
    valid = d >= 0
    assert valid.mean() > 0.5
    assert ((d == -16) | ((d >= 0) & (d <= 63 * 16))).all()
    gt = syn.gt_disparity(1920, 1080)
    err = np.abs(d / 16.0 - gt)[valid]
    assert np.median(err) < 1.0
    # determinism
    d2 = matcher.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert (d == d2).all()
    want = oracle.sgbm_compute(L, R)
    assert not mismatch_report(d, want, "1080p disp16"), mismatch_report(d, want, "1080p disp16")


@pytest.mark.parametrize("dpl", [4, 8])
@pytest.mark.parametrize("W,H,n", [(160, 96, 1), (203, 77, 2), (320, 180, 3), (64 + 128, 40, 1), (64 + 129, 33, 2), (64 + 256, 21, 1)])
def test_lockstep_top_down_kernel(native, oracle, W, H, n, dpl):
    """r1 + r2 + r3 in one lock-step pass (k_vdd) instead of three k_chain launches, both strip mappings.
    Covers strips that end mid-image, exact multiples of the strip width, multi-frame launches."""
    pairs = [textured_pair(W, H, seed=50 + i) for i in range(n)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"lockstep": 1, "vdd_dpl": dpl})
    Ls = _dev(native, np.stack([p[0] for p in pairs]))
    Rs = _dev(native, np.stack([p[1] for p in pairs]))
    for rep in range(2):                                    # second call: fresh sequence tag over stale granules
        got = m.compute(Ls, Rs).cpu().numpy()
        assert m.sync_errors() == 0
        for i in range(n):
            want = oracle.sgbm_compute(*pairs[i])
            assert not mismatch_report(got[i], want, f"vdd frame {i} rep {rep}"), mismatch_report(got[i], want, f"vdd frame {i} rep {rep}")
    m.close()


PARAM_SETS = [
    dict(uniquenessRatio=0),
    dict(uniquenessRatio=100),
    dict(uniquenessRatio=35, disp12MaxDiff=3),
    dict(speckleWindowSize=0),
    dict(speckleWindowSize=400, speckleRange=1),
    dict(preFilterCap=31, P1=200, P2=900),
    dict(P1=8, P2=32),
    dict(P1=1500, P2=9000, mode=1),
    dict(disp12MaxDiff=10, uniquenessRatio=5, speckleWindowSize=30, speckleRange=4, mode=1),
]


@pytest.mark.parametrize("kw", PARAM_SETS, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("vdd", [1, 0])
def test_parameter_sweep(native, oracle, kw, vdd):
    """every StereoSGBM_create keyword the build accepts, away from depth.py's values, through both the
    lock-step (k_vdd + k_hfused) and the per-direction (k_chain) code paths"""
    W, H = 250, 64
    L, R = textured_pair(W, H, seed=sum(kw.values()) + 3)
    want = oracle.sgbm_compute(L, R, oracle.default_params(**kw))
    # vdd = 0 also takes the round-2 forms of the small kernels: L-R check + median as tiles, k_hfused one wave per row group
    m = native.StereoSGBM(max_width=W, max_height=H, options={"lockstep": vdd, "hfused": vdd, "lrm_tiles": 1 - vdd, "hf_persist": vdd}, **kw)
    got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert m.sync_errors() == 0
    m.close()
    assert not mismatch_report(got, want, str(kw)), mismatch_report(got, want, str(kw))


def test_noise_and_flat_inputs(native, oracle, matcher):
    """no structure at all (pure noise: most pixels rejected) and piecewise-flat input (massive cost ties)"""
    rng = np.random.default_rng(77)
    W, H = 300, 70
    L = rng.integers(0, 256, (H, W), dtype=np.uint8)
    R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    got = matcher.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert not mismatch_report(got, oracle.sgbm_compute(L, R), "noise")
    flat = np.repeat(np.repeat(rng.integers(0, 256, (H // 10, W // 20), dtype=np.uint8), 10, axis=0), 20, axis=1)
    flatR = np.roll(flat, -6, axis=1)
    got = matcher.compute(_dev(native, flat), _dev(native, flatR)).cpu().numpy()
    assert not mismatch_report(got, oracle.sgbm_compute(flat, flatR), "flat")
    sat = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)          # saturated gradients everywhere
    got = matcher.compute(_dev(native, sat), _dev(native, np.roll(sat, -11, axis=1))).cpu().numpy()
    assert not mismatch_report(got, oracle.sgbm_compute(sat, np.roll(sat, -11, axis=1)), "binary")


def _fuzz_case(seed):
    """random geometry, parameters and image content, all derived from the seed"""
    rng = np.random.default_rng(1000 + seed)
    W = int(rng.integers(70, 420)); H = int(rng.integers(1, 150))
    if seed % 7 == 0: H = int(rng.integers(1, 4))                 # one to three rows
    if seed % 5 == 0: W = 69 + seed % 3                           # a handful of cost columns
    kind = seed % 4
    if kind == 0:
        L, R = textured_pair(W, H, seed=seed)
    elif kind == 1:                                               # unrelated noise: every check fails somewhere
        L = rng.integers(0, 256, (H, W), dtype=np.uint8); R = rng.integers(0, 256, (H, W), dtype=np.uint8)
    elif kind == 2:                                               # hard edges and saturated patches
        L = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)
        L = np.repeat(np.repeat(L[::4, ::4], 4, axis=0), 4, axis=1)[:H, :W] if H >= 4 and W >= 4 else L
        R = np.roll(L, -int(rng.integers(0, 40)), axis=1)
    else:                                                         # smooth ramps: long runs of equal costs (tie-breaks)
        x = np.linspace(0, 255, W)[None, :] * np.ones((H, 1)); L = x.astype(np.uint8); R = np.roll(L, -7, axis=1)
    P1 = int(rng.integers(1, 900)); P2 = int(rng.integers(P1 + 1, 6000))
    kw = dict(P1=P1, P2=P2, uniquenessRatio=int(rng.integers(0, 60)), disp12MaxDiff=int(rng.integers(1, 8)),
              speckleWindowSize=int(rng.choice([0, 20, 100, 300])), speckleRange=int(rng.integers(1, 40)),
              preFilterCap=int(rng.choice([0, 15, 31])), mode=int(rng.integers(0, 2)))
    return W, H, np.ascontiguousarray(L), np.ascontiguousarray(R), kw


@pytest.mark.parametrize("seed", range(28))
def test_fuzz_geometry_parameters_content(native, oracle, seed):
    """seeded fuzz over sizes (down to one row / five cost columns), every accepted parameter and four kinds of image
    content; final disparity bit-exact against the oracle, no lock-step time-outs"""
    W, H, L, R, kw = _fuzz_case(seed)
    want = oracle.sgbm_compute(L, R, oracle.default_params(**kw))
    m = native.StereoSGBM(max_width=W, max_height=H, **kw)
    got = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    errs = m.sync_errors()
    m.close()
    assert errs == 0
    assert not mismatch_report(got, want, f"seed {seed} {W}x{H} {kw}"), mismatch_report(got, want, f"seed {seed} {W}x{H} {kw}")


def test_lockstep_runtime_switch(native, oracle):
    """v3d_sgbm_set_lockstep: the per-direction launches and the lock-step pass give the same bits on one handle"""
    W, H = 300, 90
    L, R = textured_pair(W, H, seed=77)
    want = oracle.sgbm_compute(L, R)
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=2)
    a = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    m.set_lockstep(False)
    b = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert m.sync_errors() == 0
    m.set_lockstep(True)
    c = m.compute(_dev(native, L), _dev(native, R)).cpu().numpy()
    assert m.sync_errors() == 0
    m.close()
    assert np.array_equal(a, want) and np.array_equal(b, want) and np.array_equal(c, want)


def test_benchmarked_configuration_bit_exact(native, oracle):
    """a BELOW-capacity 1080p launch: 30 frames per call on a max_batch=30 handle, then 16 on the same handle -- k_vdd<8>
    (128-column strips, the last one ragged: 1856 = 14 x 128 + 64) with fewer co-resident lock-step workgroups than a full
    launch, the XCD tile order of k_cost over 30 frames, batch-wide CCL.  Five distinct frames, cycled; EVERY frame of the
    batch must equal the oracle's bits.  bench.py's own batch (one FULL launch, vdd_frames_per_launch_dpl8 frames) and the
    product's launch splits are tested frame by frame in tests/test_bench_config_gpu.py."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from video_3d_pipeline import synthetic as syn
    W, H, n, nd = 1920, 1080, 30, 5
    pairs = [syn.gray_pair(W, H, 100 + i) for i in range(nd)]
    with ThreadPoolExecutor(nd) as ex:                       # ctypes releases the GIL inside liboracle.so
        want = list(ex.map(lambda p: oracle.sgbm_compute(*p), pairs))
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n)
    assert n > m.get_option("vdd_frames_per_launch_dpl4"), "batch must be large enough to select the 8-disparities-per-lane strips"
    assert m.get_option("vdd_frames_per_launch_dpl8") >= 1 and m.get_option("lockstep") == 1
    Ls = _dev(native, np.stack([pairs[i % nd][0] for i in range(n)]))
    Rs = _dev(native, np.stack([pairs[i % nd][1] for i in range(n)]))
    wd = [_dev(native, w) for w in want]
    for rep in range(2):
        got = m.compute(Ls, Rs)
        assert m.sync_errors() == 0
        for i in range(n):
            if not torch.equal(got[i], wd[i % nd]):
                g = got[i].cpu().numpy()
                raise AssertionError(mismatch_report(g, want[i % nd], f"batch-30 frame {i} rep {rep}"))
    # batch 16 on the same handle: still above the 4-per-lane bound, one launch of 16 x 15 strips
    got = m.compute(Ls[:16].contiguous(), Rs[:16].contiguous())
    assert m.sync_errors() == 0
    for i in range(16):
        assert torch.equal(got[i], wd[i % nd]), f"batch-16 frame {i}"
    m.close()


def test_lockstep_timeout_is_never_silent(native, oracle):
    """a timed-out lock-step pass must not hand out disparities.  vdd_spin_limit = -1 makes every workgroup
    report a time-out: the call's output is invalidated on the device, the next call raises, set_lockstep() recovers."""
    W, H, n = 64 + 256, 120, 2
    pairs = [textured_pair(W, H, seed=90 + i) for i in range(n)]
    want = [oracle.sgbm_compute(*p) for p in pairs]
    Ls = _dev(native, np.stack([p[0] for p in pairs])); Rs = _dev(native, np.stack([p[1] for p in pairs]))
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"vdd_spin_limit": -1})
    got = m.compute(Ls, Rs).cpu().numpy()
    assert m.poll_errors() > 0 and m.sync_errors() > 0
    assert (got == -16).all(), "a timed-out pass must leave no disparity behind"
    with pytest.raises(native.LockstepTimeout):
        m.compute(Ls, Rs)
    m.set_lockstep(False)                                    # what depth.py does: per-direction launches, same bits
    got = m.compute(Ls, Rs).cpu().numpy()
    assert m.sync_errors() == 0 and m.get_option("lockstep") == 0
    for i in range(n):
        assert not mismatch_report(got[i], want[i], f"fallback frame {i}")
    m.set_option("vdd_spin_limit", 0)
    m.set_lockstep(True)
    got = m.compute(Ls, Rs).cpu().numpy()
    assert m.sync_errors() == 0 and m.poll_errors() == 0
    for i in range(n):
        assert not mismatch_report(got[i], want[i], f"lock-step frame {i}")
    with pytest.raises(native.NativeError):
        m.set_option("no_such_option", 1)
    m.close()


def test_handle_options_round_trip(native):
    """every key of v3d_sgbm_set_option / _get_option: its default, a good value reads back, a bad one raises and leaves the
    setting alone, the read-only keys refuse a set.  No compute call: a tiny handle, milliseconds."""
    import torch
    m = native.StereoSGBM(max_width=96, max_height=8, max_batch=1)
    ncu = torch.cuda.get_device_properties(m.device).multi_processor_count
    onoff = lambda default: (default, (1 - default, default), (2,))
    table = {                                                 # key: (default, good values, bad values)
        "lockstep": onoff(1), "hfused": onoff(1), "chain_dpl": (4, (8, 4), (6,)), "hsplit": onoff(0),
        "vdd_dpl": (0, (4, 8, 0), (2,)), "cost_band": (90, (8, 65536, 90), (7, 65537)), "cost_xcd": onoff(1),
        "vdd_xcd": onoff(0), "hf_xcd": onoff(0), "hf_persist": onoff(1), "lrm_tiles": onoff(0),
        "reserve_cus": (0, (2, ncu, 0), (-1, ncu + 1)), "vdd_spin_limit": (0, (-1, 100, 0), (-2,)),
        "vdd_launch_frames": (0, (3, 0), (-1,)), "vdd_seq": (1, (0xFFFFF, 1), (0, 0x100000)),
    }
    for key, (default, _, _) in table.items():
        assert m.get_option(key) == default, f"default of {key}"
    for key, (default, good, bad) in table.items():
        for g in good:                                        # the last good value is the default: reserve_cus is back at 0
            m.set_option(key, g)                              # before "lockstep" could be read again
            assert m.get_option(key) == g, f"{key} = {g} does not read back"
            for b in bad:
                with pytest.raises(native.NativeError, match=f"option {key}: value {b} out of range"):
                    m.set_option(key, b)
                assert m.get_option(key) == g, f"refused {key} = {b} changed the setting"
        assert m.get_option(key) == default
    for key in ("vdd_frames_per_launch_dpl4", "vdd_frames_per_launch_dpl8"):
        assert m.get_option(key) >= 1
        with pytest.raises(native.NativeError, match=f"unknown option {key}"):
            m.set_option(key, 1)
    with pytest.raises(native.NativeError, match="unknown option no_such_option"):
        m.get_option("no_such_option")
    m.close()


def test_reserved_cus_shrink_the_lockstep_launch(native, oracle):
    """reserve_cus (CUs a concurrent collective keeps busy) lowers the frames per lock-step launch; a batch then takes
    several launches and still gives the oracle's bits"""
    W, H, n = 64 + 300, 60, 3
    pairs = [textured_pair(W, H, seed=120 + i) for i in range(n)]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n)
    full = m.get_option("vdd_frames_per_launch_dpl4")
    ncu_res = 0
    while m.get_option("vdd_frames_per_launch_dpl4") > 1 and ncu_res < 250:     # shrink until one frame per launch
        ncu_res += 2
        m.set_option("reserve_cus", ncu_res)
    assert 1 <= m.get_option("vdd_frames_per_launch_dpl4") < full
    m.set_option("vdd_dpl", 4)
    got = m.compute(_dev(native, np.stack([p[0] for p in pairs])), _dev(native, np.stack([p[1] for p in pairs]))).cpu().numpy()
    assert m.sync_errors() == 0
    m.close()
    for i in range(n):
        assert not mismatch_report(got[i], oracle.sgbm_compute(*pairs[i]), f"frame {i}")


def test_oversized_lockstep_launch_waits_instead_of_deadlocking(native, oracle):
    """only the strips of ONE frame must be co-resident, and workgroups are dispatched in blockIdx order: a launch with
    more workgroups than the chip holds (here 96 frames x 8 strips = 768 > 2 x 256 slots, forced with vdd_launch_frames)
    runs whole frames first and the rest as slots free up: no time-out, the oracle's bits.  (Rounds 1-2 sized every
    launch 10 % below the occupancy bound and never let one exceed it.)"""
    import torch
    W, H, n, nd = 64 + 1000, 48, 96, 3
    pairs = [textured_pair(W, H, seed=300 + i) for i in range(nd)]
    want = [oracle.sgbm_compute(*p) for p in pairs]
    m = native.StereoSGBM(max_width=W, max_height=H, max_batch=n, options={"vdd_dpl": 8, "vdd_launch_frames": n})
    assert m.get_option("vdd_frames_per_launch_dpl8") < n, "the launch must exceed the co-residency bound"
    Ls = _dev(native, np.stack([pairs[i % nd][0] for i in range(n)]))
    Rs = _dev(native, np.stack([pairs[i % nd][1] for i in range(n)]))
    for rep in range(2):
        got = m.compute(Ls, Rs)
        assert m.sync_errors() == 0
        for i in range(n):
            assert torch.equal(got[i].cpu(), torch.from_numpy(want[i % nd])), f"frame {i} rep {rep}"
    m.close()


@pytest.mark.parametrize("W,H", [(300, 40), (64, 9), (1, 5), (257, 1), (640, 33), (516, 19), (1920, 17)])
def test_speckle_run_lists_extremes(native, oracle, W, H):
    """the run-list CCL at its corners: every pixel its own run (a full run list without end marker, > 64 runs per row
    -> several steps of the per-row walkers), one run per row, single-column / single-row images, runs of exactly the
    threshold length, and random mixtures with a tight maxDiff"""
    rng = np.random.default_rng(W * 31 + H)
    yy, xx = np.mgrid[0:H, 0:W]
    cases = {
        "checkerboard": np.where((yy + xx) % 2 == 0, 0, 8000).astype(np.int16),            # no two neighbours connect: all size 1
        "rows": (yy * 16).astype(np.int16) * np.ones((1, W), np.int16),                    # one run per row, all joined vertically
        "columns": np.where(xx % 2 == 0, 160, 9000).astype(np.int16),                      # W runs per row, joined vertically: size H each
        "random": (rng.integers(0, 6, (H, W)) * 700).astype(np.int16),
        "sparse": np.where(rng.random((H, W)) < 0.6, -16, (rng.integers(0, 4, (H, W)) * 300)).astype(np.int16),
    }
    for name, img in cases.items():
        for max_size, max_diff in ((100, 512), (H, 100), (3, 1)):
            got = native.filter_speckles(_dev(native, img), -16, max_size, max_diff).cpu().numpy()
            want = oracle.filter_speckles(img, -16, max_size, max_diff)
            assert not mismatch_report(got, want, f"{name} {W}x{H} size<={max_size} diff<={max_diff}"), \
                mismatch_report(got, want, f"{name} {W}x{H} size<={max_size} diff<={max_diff}")


@pytest.mark.parametrize("W,H", [(70, 5), (257, 33), (300, 31), (1920, 64), (2048, 8), (2050, 6), (2500, 40), (4000, 12), (4096, 4), (4100, 3)])
def test_lrcheck_median_row_march_equals_tiles_and_oracle(native, oracle, W, H):
    """the L-R check + 3x3 median as a row march over full-width bands (default; 8 or 16 pixels per thread and row) against
    the 128 x 16 tile form and the oracle: band edges (30-row bands), image borders, widths that end mid-thread-stride, the raw
    (no median) export too"""
    import torch
    L, R = textured_pair(W, H, seed=W + H)
    want = oracle.sgbm_compute(L, R)
    outs = {}
    for tiles in (0, 1):
        m = native.StereoSGBM(max_width=W, max_height=H, options={"lrm_tiles": tiles})
        outs[tiles] = (m.compute(_dev(native, L), _dev(native, R)), m.debug_raw(_dev(native, L), _dev(native, R)))
        assert m.sync_errors() == 0
        m.close()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not mismatch_report(outs[0][0].cpu().numpy(), want, f"{W}x{H}")


@pytest.mark.parametrize("W,H", [(640, 48), (516, 35), (1920, 33)])
def test_speckle_merge_shapes(native, oracle, W, H):
    """the lock-free union-find where many roots merge at once (tests/speckle_shapes.py: combs, a spiral, a serpentine, a
    staircase, components of exactly the threshold size spread over both merge levels, plateaus at the maxDiff edge, full run
    lists): the emulated test runs these one fiber at a time, a race shows only here.  Every parameter set runs twice and both
    outputs must be the oracle's.  No surface hands a given plane to a StereoSGBM handle's speckle stage (the handle takes
    images), so the batched stage is run on these planes by tests/test_speckle_emulated.py alone"""
    import torch
    import speckle_shapes as SS
    for max_size, max_diff in ((100, 512), (3, 1)):
        planes = SS.shapes(W, H, max_size, max_diff)
        assert {"comb-bottom", "comb-top", "spiral", "serpentine", "staircase", "plateaus", "full-lists"} <= set(planes)
        assert ("exact" in planes) == (H >= 34 and max_size >= SS.EXACT_MIN)
        for name, img in planes.items():
            want = oracle.filter_speckles(img, -16, max_size, max_diff)
            dev = _dev(native, img)
            first = native.filter_speckles(dev, -16, max_size, max_diff)
            second = native.filter_speckles(dev, -16, max_size, max_diff)
            tag = f"{name} {W}x{H} size<={max_size} diff<={max_diff}"
            assert torch.equal(first, second), tag + ": two runs differ"
            assert not mismatch_report(first.cpu().numpy(), want, tag), mismatch_report(first.cpu().numpy(), want, tag)
