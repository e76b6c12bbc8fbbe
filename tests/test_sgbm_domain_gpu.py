"""The SGBM kernels at the edges of the domain v3d_sgbm_create and run_sgbm accept: the int16 headroom of the packed
recurrence (largest accepted P2 per preFilterCap, on content that uses the headroom; inputs pinned in
test_sgbm_domain_host.py), the acceptance line itself, parameter normalisation, uniquenessRatio at and above 100, speckle
parameters beyond their ordinary range, the row limit of the lock-step pass and the smallest accepted frame.
Every comparison is bit-exact int16 against the oracle; every test ends with sync_errors() == 0."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sgbm_domain as sd
from conftest import mismatch_report, textured_pair

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -3

ROUTES = [
    ("default", {}),                                             # lock-step k_vdd + persistent k_hfused
    ("chain4", {"lockstep": 0, "chain_dpl": 4}),
    ("chain8", {"lockstep": 0, "chain_dpl": 8}),
    ("vdd4", {"lockstep": 1, "vdd_dpl": 4}),
    ("vdd8", {"lockstep": 1, "vdd_dpl": 8}),
    ("hfused0", {"hfused": 0}),
    ("hsplit", {"hsplit": 1}),
    ("waves+tiles", {"hf_persist": 0, "lrm_tiles": 1}),
]
CHAIN_WTA = ("chain+wta", {"lockstep": 0, "hfused": 0})           # the WTA tail on k_chain MODE 2


def _ids(kw):
    return ",".join(f"{a}={b}" for a, b in kw.items())


def _run(native, oracle, L, R, kw, routes, stages=("compute", "raw"), cv_routes=()):
    """every route in `routes` on one pair: final disparity and raw disparity (and the cost volume on `cv_routes`) against
    the oracle, no lock-step time-outs; returns the list of mismatch reports"""
    H, W = L.shape
    p = oracle.default_params(**kw)
    want = {"compute": oracle.sgbm_compute(L, R, p), "raw": oracle.sgbm_raw(L, R, p)}
    want_cv = oracle.cost_volume(L, R, p) if cv_routes else None
    dl, dr = native.to_device(L), native.to_device(R)
    bad = []
    for name, options in routes:
        m = native.StereoSGBM(max_width=W, max_height=H, options=options, **kw)
        got = {"compute": m.compute(dl, dr).cpu().numpy()}
        if "raw" in stages:
            got["raw"] = m.debug_raw(dl, dr).cpu().numpy()
        if name in cv_routes:
            bad.append(mismatch_report(m.debug_cost_volume(dl, dr).cpu().numpy(), want_cv, f"{name} C {W}x{H} {kw}"))
        errs = m.sync_errors()
        m.close()
        assert errs == 0, f"{name}: {errs} lock-step time-outs"
        bad += [mismatch_report(g, want[s], f"{name} {s} {W}x{H} {kw}") for s, g in got.items()]
    return [b for b in bad if b]


# ---------------------------------------------------------------------------------------------------------------------
# headroom boundary, every route
# ---------------------------------------------------------------------------------------------------------------------
CAPS, SIZES = sd.CAPS, sd.HEADROOM_SIZES


def _content(name, W, H, ftzero):
    if name == "ceiling":
        return sd.ceiling_pair(W, H, ftzero)
    if name == "binary":
        return sd.binary_inverse_pair(W, H, seed=W + H)
    return textured_pair(W, H, seed=W + H)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("p1", ["P2-1", "1"])
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("content", ["ceiling", "binary", "textured"])
def test_largest_accepted_p2_every_route(native, oracle, content, cap, p1, mode):
    """P2 = the largest value the headroom rule accepts for this preFilterCap: delta = min L + P2 and C = P2 + box sum come
    within two of 32767 on the ceiling content, S saturates in both modes.  All eight routes; the cost volume (12-bit
    C - P2 storage near its design limit) on the default and one k_chain route."""
    ft = sd.ftzero_of(cap)
    P2 = sd.p2max(ft)
    W, H = SIZES[cap]
    L, R = _content(content, W, H, ft)
    kw = dict(preFilterCap=cap, P2=P2, P1=P2 - 1 if p1 == "P2-1" else 1, mode=mode)
    bad = _run(native, oracle, L, R, kw, ROUTES, cv_routes=("default", "chain8"))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the acceptance line
# ---------------------------------------------------------------------------------------------------------------------
def _create_rc(native, W=64 + 70, H=40, **kw):
    """v3d_sgbm_create through the C ABI: (return code, handle or None)"""
    import torch
    h = C.c_void_p()
    p = native.default_params(**kw)
    rc = native.lib().v3d_sgbm_create(C.byref(p), torch.cuda.current_device(), W, H, 1, C.byref(h))
    return rc, h


@pytest.mark.parametrize("cap", CAPS + [14, 30])
def test_acceptance_line_of_p2(native, cap):
    P2 = sd.p2max(sd.ftzero_of(cap))
    assert sd.accepted(P2, cap) and not sd.accepted(P2 + 1, cap)
    m = native.StereoSGBM(max_width=64 + 70, max_height=40, preFilterCap=cap, P2=P2)
    assert m.sync_errors() == 0
    m.close()
    with pytest.raises(native.NativeError, match="int16 range"):
        native.StereoSGBM(max_width=64 + 70, max_height=40, preFilterCap=cap, P2=P2 + 1)
    rc, h = _create_rc(native, preFilterCap=cap, P2=P2 + 1)
    assert rc == ERR_UNSUPPORTED and not h.value
    # P2 is judged after normalisation: P1 lifts a small P2 over the line
    rc, h = _create_rc(native, preFilterCap=cap, P1=P2 + 1, P2=100)
    assert rc == ERR_UNSUPPORTED and not h.value
    rc, h = _create_rc(native, preFilterCap=cap, P1=P2 - 1, P2=100)
    assert rc == 0 and h.value
    assert native.lib().v3d_sgbm_sync_errors(h) == 0
    native.lib().v3d_sgbm_destroy(h)


@pytest.mark.parametrize("cap", [32, 63])
def test_prefilter_cap_above_31_is_refused(native, cap):
    with pytest.raises(native.NativeError):
        native.StereoSGBM(max_width=64 + 70, max_height=40, preFilterCap=cap)
    rc, h = _create_rc(native, preFilterCap=cap, P1=1, P2=2)       # not for P2's sake: refused at the smallest P2 as well
    assert rc == ERR_UNSUPPORTED and not h.value


# ---------------------------------------------------------------------------------------------------------------------
# normalisation on the device
# ---------------------------------------------------------------------------------------------------------------------
RAW_VALUES = [
    dict(P1=0), dict(P1=-5), dict(P2=0), dict(P2=0, P1=3), dict(P1=600, P2=600), dict(P1=900, P2=100),
    dict(uniquenessRatio=-1), dict(disp12MaxDiff=0), dict(disp12MaxDiff=-1), dict(disp12MaxDiff=64),
    dict(preFilterCap=14), dict(preFilterCap=16), dict(preFilterCap=30),
]


@pytest.mark.parametrize("kw", RAW_VALUES, ids=_ids)
def test_parameter_normalisation_on_the_device(native, oracle, kw):
    """values create rewrites (and their neighbours that it must not): the oracle is given the same raw values"""
    routes = [ROUTES[0], ("chain+wta+tiles", {"lockstep": 0, "hfused": 0, "lrm_tiles": 1})]
    bad = []
    for L, R in (sd.patchy_pair(64 + 136, 60, 17), textured_pair(64 + 75, 44, seed=23)):
        bad += _run(native, oracle, L, R, kw, routes, cv_routes=("default",))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# uniquenessRatio 100 and above
# ---------------------------------------------------------------------------------------------------------------------
def _uniq_pairs():
    W, H = 64 + 136, 40
    same = sd.same_view_noise(W, H, 3)
    L, R = textured_pair(W, H, seed=41)
    R = R.copy()
    R[:, :W // 2] = L[:, :W // 2]                                # min S == 0 on the left half, ordinary matching on the right
    return [same, (L, R)]


def test_uniqueness_ratio_100_parity(native, oracle):
    """100 - uniquenessRatio == 0: a pixel is rejected iff min S > 0.  Both WTA tails (k_hfused, k_chain MODE 2)."""
    bad = []
    for L, R in _uniq_pairs():
        bad += _run(native, oracle, L, R, dict(uniquenessRatio=100), [ROUTES[0], CHAIN_WTA])
    assert not bad, "\n".join(bad)
    L, R = _uniq_pairs()[0]
    assert (oracle.sgbm_raw(L, R, oracle.default_params(uniquenessRatio=100))[:, sd.D:] >= 0).all()


@pytest.mark.parametrize("uniq", [101, 150])
def test_uniqueness_ratio_above_100_is_refused(native, uniq):
    """OpenCV's literal S[d] * (100 - uniq) < minS * 100 with a negative factor rejects a pixel with min S == 0 as soon as
    a far S[d] > 0 (test_sgbm_domain_host.py); the kernels' threshold form keeps it.  Create refuses the value."""
    with pytest.raises(native.NativeError, match="uniquenessRatio"):
        native.StereoSGBM(max_width=64 + 136, max_height=40, uniquenessRatio=uniq)
    rc, h = _create_rc(native, uniquenessRatio=uniq)
    assert rc == ERR_UNSUPPORTED and not h.value
    m = native.StereoSGBM(max_width=64 + 136, max_height=40, uniquenessRatio=100)      # the last accepted value
    assert m.sync_errors() == 0
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# speckle parameters through the handle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(speckleRange=0), dict(speckleRange=2048), dict(speckleRange=5000),
                                dict(speckleWindowSize=1), dict(speckleWindowSize="W*H+1"), dict(speckleWindowSize=-1),
                                dict(speckleWindowSize="W*H+1", speckleRange=5000)], ids=_ids)
def test_speckle_parameters_beyond_the_ordinary_range(native, oracle, kw):
    """16 * speckleRange past int16 (every pair of valid neighbours joins), 0 (only equal values join), a window of one
    pixel, a window larger than the image (nothing survives) and -1 (filter off), on pairs with components of every size"""
    bad = []
    for L, R in sd.speckle_pairs():
        H, W = L.shape
        k = {a: (W * H + 1 if b == "W*H+1" else b) for a, b in kw.items()}
        bad += _run(native, oracle, L, R, k, [ROUTES[0]], stages=("compute",))
        if kw.get("speckleWindowSize") == "W*H+1":
            assert (oracle.sgbm_compute(L, R, oracle.default_params(**k)) == -16).all()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the row limit of the lock-step pass
# ---------------------------------------------------------------------------------------------------------------------
ROWS_W = 64 + 136


@pytest.fixture(scope="module")
def tall(oracle):
    """one 200 x 4096 textured pair and its crops; expected outputs computed once, in parallel (ctypes releases the GIL)"""
    L, R = textured_pair(ROWS_W, 4096, seed=4096)
    small = [textured_pair(ROWS_W, 60, seed=60 + i) for i in range(2)]
    crop = lambda w, h: (np.ascontiguousarray(L[:h, :w]), np.ascontiguousarray(R[:h, :w]))
    jobs = {("m0", ROWS_W, 4096): (crop(ROWS_W, 4096), 0), ("m0", ROWS_W, 4094): (crop(ROWS_W, 4094), 0),
            ("m0", 64 + 19, 4095): (crop(64 + 19, 4095), 0), ("m0", "small0"): (small[0], 0), ("m0", "small1"): (small[1], 0),
            ("m1", ROWS_W, 4094): (crop(ROWS_W, 4094), 1), ("m1", ROWS_W, 4096): (crop(ROWS_W, 4096), 1)}
    with ThreadPoolExecutor(len(jobs)) as ex:
        want = dict(zip(jobs, ex.map(lambda j: oracle.sgbm_compute(*j[0], oracle.default_params(mode=j[1])), jobs.values())))
    return {"pair": {k: j[0] for k, j in jobs.items()}, "want": want}


def _tall_call(native, m, tall, key):
    L, R = tall["pair"][key]
    got = m.compute(native.to_device(L), native.to_device(R)).cpu().numpy()
    assert m.sync_errors() == 0, f"{key}: lock-step time-outs"
    rep = mismatch_report(got, tall["want"][key], str(key))
    assert not rep, rep


def test_row_limit_one_handle_switches_routes(native, tall):
    """H < 4095 takes the lock-step pass (granule tag = (seq << 12) | (y + 1), 4094 rows end at tag 0xFFE), H >= 4095 the
    per-direction k_chain launches.  One handle, call by call: 4096 (k_chain), 4094 (the last lock-step height), 4095 on a
    narrow frame (k_chain), a batch of two short frames (lock-step: fresh tags over the stale ones of the tall call),
    4094 again.  Also the row-march L-R check, the median and the CCL merge bands at 4000+ rows."""
    m = native.StereoSGBM(max_width=ROWS_W, max_height=4096, max_batch=2)
    assert m.get_option("lockstep") == 1
    _tall_call(native, m, tall, ("m0", ROWS_W, 4096))
    _tall_call(native, m, tall, ("m0", ROWS_W, 4094))
    _tall_call(native, m, tall, ("m0", 64 + 19, 4095))
    pairs = [tall["pair"][("m0", "small0")], tall["pair"][("m0", "small1")]]
    got = m.compute(native.to_device(np.stack([p[0] for p in pairs])), native.to_device(np.stack([p[1] for p in pairs]))).cpu().numpy()
    assert m.sync_errors() == 0
    for i in range(2):
        rep = mismatch_report(got[i], tall["want"][("m0", f"small{i}")], f"batch frame {i} after the tall calls")
        assert not rep, rep
    _tall_call(native, m, tall, ("m0", ROWS_W, 4094))
    m.close()


def test_row_limit_eight_paths(native, tall):
    """the bottom-up lock-step pass at 4094 rows and the three bottom-up k_chain launches at 4096"""
    m = native.StereoSGBM(max_width=ROWS_W, max_height=4096, mode=1)
    _tall_call(native, m, tall, ("m1", ROWS_W, 4094))
    _tall_call(native, m, tall, ("m1", ROWS_W, 4096))
    m.close()


# ---------------------------------------------------------------------------------------------------------------------
# the smallest accepted geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cap", [0, 31])
def test_smallest_frame_at_the_headroom_boundary(native, oracle, cap, mode):
    """W = 69 (five cost columns), H = 1, ceiling content, the largest accepted P2"""
    ft = sd.ftzero_of(cap)
    P2 = sd.p2max(ft)
    L, R = sd.ceiling_pair(69, 1, ft)
    bad = []
    for P1 in (P2 - 1, 1):
        bad += _run(native, oracle, L, R, dict(preFilterCap=cap, P2=P2, P1=P1, mode=mode), [ROUTES[0], ROUTES[1], CHAIN_WTA],
                    cv_routes=("default", "chain4"))
    assert not bad, "\n".join(bad)


def test_width_68_is_refused(native):
    with pytest.raises(native.NativeError):
        native.StereoSGBM(max_width=68, max_height=1)
    rc, h = _create_rc(native, W=68, H=1)
    assert rc == ERR_ARG and not h.value
    m = native.StereoSGBM(max_width=69, max_height=1)
    z = native.to_device(np.zeros((1, 68), np.uint8))
    with pytest.raises(native.NativeError):
        m.compute(z, z)
    assert m.sync_errors() == 0
    m.close()
