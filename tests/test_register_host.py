"""Host side of the spatial registration on the CPU: the decision rule on hand-made tables, the search on synthetic clips with a
NumPy stand-in for the device (tests/register_ref.py), the rounding of the conversions to Q16, the alignment file's block and its
refusals, and the upscale / pipeline drivers: with no block, --no-spatial or the identity they make the calls, keys and bytes
they made before; with a map the low-res depth passes through the warp right before the guided filter."""
import json

import numpy as np
import pytest

import register_ref as RR
from test_host import OracleUpscaleBackend
from test_pipeline_host import OraclePipelineBackend, SH, SW, _pngs

Q = RR.Q
EYE, GUIDE = (256, 144), (512, 288)
MAPS = {                                                   # (Ax, Bx, Ay, By), bars in the eye
    "letterbox": ((1.0, 0.0, 0.875, 0.0625), True),        # bars over 12.5 % of the eye's height, the guide shows the picture alone
    "crop": ((0.9, 0.05, 0.9, 0.05), False),               # the guide is the centred 90 % of the eye
    "anamorphic": ((1.03, 5 / 256 - 0.015, 1.0, 0.0), False),   # 3 % horizontal stretch about the centre, shifted by 5 eye pixels
    "parallax": ((1.0, 6 / 256, 1.0, 0.0), False),         # the 2D master is the other eye: 6 eye pixels to the side
    "identity": ((1.0, 0.0, 1.0, 0.0), False),
}


class RefRegisterBackend:
    """test-only stand-in for estimate()'s backend: the left eye of an SBS frame is its left half (gray in all channels)"""

    def sbs_left_profiles(self, frames, unsqueeze):
        assert not unsqueeze
        return RR.profiles(np.stack([f[:, :f.shape[1] // 2, 0] for f in frames]))

    def guide_profiles(self, frames, height, width):
        assert all(f.shape[:2] == (height, width) for f in frames)
        return RR.profiles(np.stack([f[..., 0] for f in frames]))

    def match_scores(self, prof_a, prof_b, cand, bins):
        return RR.match_scores(prof_a, prof_b, cand, bins)


def _clip_pair(d, name, amap, bars, n=3, flat=()):
    from video_3d_pipeline import synthetic as syn
    pairs = [syn.registered_pair(EYE, GUIDE, amap, i, bars) for i in range(n)]
    eye, guide = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    for i in flat:
        eye[i], guide[i] = 16, 16
    np.save(d / f"{name}_sbs.npy", np.repeat(np.concatenate([eye, eye], axis=2)[..., None], 3, axis=3))
    np.save(d / f"{name}_g.npy", np.repeat(guide[..., None], 3, axis=3))
    return str(d / f"{name}_sbs.npy"), str(d / f"{name}_g.npy")


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("reg")
    return {name: _clip_pair(d, name, m, bars) for name, (m, bars) in MAPS.items()}


# ---------------------------------------------------------------- conversions
def test_host_conversions_are_the_restatements():
    from video_3d_pipeline import register as R
    rng = np.random.default_rng(0)
    for _ in range(200):
        A, B = float(rng.uniform(0.7, 1.4)), float(rng.uniform(-0.3, 0.3))
        Ws, Wo = int(rng.integers(1, 4000)), int(rng.integers(1, 4000))
        assert R.map_to_q16(A, B, Ws, Wo) == RR.map_to_q16(A, B, Ws, Wo)
        p0, p1, nb = int(rng.integers(-Q * 500, Q * 500)), int(rng.integers(Q * 600, Q * 3000)), int(rng.integers(8, 8192))
        assert R.candidate(p0, p1, nb) == RR.candidate(p0, p1, nb)
        pairs, cand = R.to_candidates(np.array([[p0, p1]], dtype=np.int64), nb)            # the search's vectorised form
        assert cand.tolist() == [list(RR.candidate(p0, p1, nb))] or not len(cand)
        a, b = RR.candidate(p0, p1, nb)
        assert R.normalised(a, b, 1920, nb) == RR.normalised(a, b, 1920, nb)
    assert R.map_to_q16(1.0, 0.0, 1920, 1920) == (Q, 0) and R.rhu(-0.5) == 0 and R.rhu(0.5) == 1 and R.rhu(-1.5) == -1
    # a map written to JSON and read back gives the same integers
    m = [0.1 + 0.2, 1e-3, 0.875, 0.0625]
    back = json.loads(json.dumps(m))
    assert R.warp_q16(back, (1920, 1080), (3840, 2160)) == R.warp_q16(m, (1920, 1080), (3840, 2160))
    assert R.warp_q16(R.IDENTITY, (1920, 1080), (3840, 2160)) == dict(q=(Q, 0, Q, 0), size=(1920, 1080))
    assert R.warp_q16(R.IDENTITY, (960, 1080), (3841, 2161))["size"] == (1921, 1081)
    with pytest.raises(ValueError, match="warp's range"):
        R.warp_q16((40.0, 0.0, 1.0, 0.0), (1920, 1080), (3840, 2160))


def test_search_levels_end_at_an_eighth_of_a_source_sample():
    from video_3d_pipeline import register as R
    for na, nb, bins in ((256, 512, 512), (144, 288, 512), (1920, 3840, 512), (1080, 1600, 512), (8192, 8192, 1024), (40, 23, 512), (9, 9, 8)):
        levels = R.search_levels(na, nb, bins)
        assert [b for b, _, _ in levels] == sorted(b for b, _, _ in levels) and levels[-1][0] <= min(bins, nb) and levels[0][0] >= 8
        assert levels[-1][1] <= Q // 8 and all(s >= 1 for _, s, _ in levels)
        assert levels[1][1] * levels[1][2] >= levels[0][1] and levels[2][1] * levels[2][2] >= levels[1][1]      # a refinement reaches the step before
        grid = R.first_grid(na, nb, levels[0][1])
        span = grid[:, 1] - grid[:, 0]
        assert span.min() >= 0.8 * na * Q - 1 and span.max() <= 1.25 * na * Q + 1 and np.abs(grid[:, 0]).max() <= na * Q // 4
        assert span.min() < 0.8 * na * Q + levels[0][1] and span.max() > 1.25 * na * Q - levels[0][1]
        assert [0, na * Q] in grid.tolist()                                                                     # the nominal map is on the grid
        assert len(R.to_candidates(grid, nb)[1]) <= 4 * R.MAX_CANDIDATES


# ---------------------------------------------------------------- decision rule
def _p(a, b, z):
    return dict(a=a, b=b, z=z)


def test_decision_rule():
    from video_3d_pipeline import register as R
    nom_x, nom_y = 32768, 32768                                       # 256 -> 512 and 144 -> 288
    ok = R.decide([_p(nom_x, Q, 0.9), _p(nom_x, Q + 100, 0.8), _p(nom_x + 1, Q - 100, 0.7)], [_p(nom_y, 0, 0.9)] * 3, EYE, GUIDE, 0.5)
    assert ok["status"] == "registered" and ok["map_q16"] == [[nom_x, Q], [nom_y, 0]] and ok["score"] == [0.8, 0.9]
    assert ok["map"] == (1.0, 1 / 256, 1.0, 0.0)
    # an even count: the floor of the middle values' mean; probes without a Z do not vote
    even = R.decide([_p(nom_x, 10, 0.9), None, _p(nom_x, 13, 0.7), _p(nom_x, 0, float("nan"))], [_p(nom_y, 0, 0.6), _p(nom_y, 0, 0.8), None, None], EYE, GUIDE)
    assert even["status"] == "registered" and even["map_q16"][0] == [nom_x, 11] and even["score"] == [pytest.approx(0.8), pytest.approx(0.7)]
    # the median's score below the threshold: undetermined, the identity
    low = R.decide([_p(nom_x, Q, 0.9), _p(nom_x, Q, 0.4), _p(nom_x, Q, 0.3)], [_p(nom_y, 0, 0.9)] * 3, EYE, GUIDE, 0.5)
    assert (low["status"], low["map"]) == ("undetermined", R.IDENTITY) and low["score"][0] == 0.4
    assert R.decide([_p(nom_x, Q, 0.4)], [_p(nom_y, 0, 0.9)], EYE, GUIDE, 0.4)["status"] == "registered"      # >= min_score
    # one probe more than a source pixel off at the far end only (its scale differs): inconsistent
    far = nom_x + (Q + 600) // 512 + 1
    bad = R.decide([_p(nom_x, 0, 0.9), _p(nom_x, 0, 0.9), _p(far, 0, 0.9)], [_p(nom_y, 0, 0.9)] * 3, EYE, GUIDE)
    assert (bad["status"], bad["map"]) == ("inconsistent", R.IDENTITY)
    edge = R.decide([_p(nom_x, 0, 0.9), _p(nom_x, 0, 0.9), _p(nom_x, Q, 0.9)], [_p(nom_y, 0, 0.9)] * 3, EYE, GUIDE)
    assert edge["status"] == "registered"                                                                    # exactly one pixel agrees
    over = R.decide([_p(nom_x, 0, 0.9), _p(nom_x, 0, 0.9), _p(nom_x, Q + 1, 0.9)], [_p(nom_y, 0, 0.9)] * 3, EYE, GUIDE)
    assert over["status"] == "inconsistent"
    # nothing defined on an axis: undetermined
    for px, py in (([None, None], [_p(nom_y, 0, 0.9)] * 2), ([_p(nom_x, 0, 0.9)], [None]), ([], [])):
        res = R.decide(px, py, EYE, GUIDE)
        assert (res["status"], res["map"], res["map_q16"]) == ("undetermined", R.IDENTITY, None)


def test_ties_go_to_the_candidate_nearest_the_nominal_map():
    from video_3d_pipeline import register as R
    pairs = np.array([[-Q, 256 * Q], [0, 257 * Q], [0, 256 * Q + 5], [Q, 256 * Q], [0, 256 * Q + 5]], dtype=np.int64)
    assert R.pick(np.array([0.7, 0.7, 0.7, 0.7, 0.7]), pairs, 256) == 2
    assert R.pick(np.array([0.7, 0.9, np.nan, 0.9, 0.2]), pairs, 256) == 1
    assert R.pick(np.array([np.nan] * 5), pairs, 256) is None and R.pick(np.array([]), pairs[:0], 256) is None
    # zncc: the restatement's, NaN below bins / 2 pairs, for a zero variance and for the in-band refusal
    rec = np.array([[5, 16, 33, 209, 174, 711], [5, 10, 3, 6, 20, 9], [-1, 0, 0, 0, 0, 0]])
    assert np.allclose(R.zncc(rec, 8), RR.zncc(rec, 8), rtol=0, atol=1e-15, equal_nan=True) and np.isnan(R.zncc(rec, 8)[1:]).all()
    assert np.isnan(R.zncc(rec, 12)).all()


# ---------------------------------------------------------------- recovery
def _residual(res, amap):
    """the largest distance, in source pixels, between where the estimate and the truth put a source sample: an affine map's is at
    an end of the axis"""
    (Ax, Bx, Ay, By), (ex, bx, ey, by) = amap, res["map"]
    return max(abs(bx - Bx) * EYE[0], abs(ex + bx - Ax - Bx) * EYE[0], abs(by - By) * EYE[1], abs(ey + by - Ay - By) * EYE[1])


@pytest.mark.parametrize("name", list(MAPS))
def test_estimate_recovers_the_map(clips, name):
    """Every map within 1.0 source pixel at both ends of both axes (the registered / agree criterion, half the guided filter's
    default reach at low resolution).  What tests/register_ref.py alone achieves on these clips on the CPU, the largest residual
    in source pixels: letterbox 0.000, crop 0.090, anamorphic 0.111, parallax 0.111, identity 0.110."""
    from video_3d_pipeline import register as R
    amap, _ = MAPS[name]
    res = R.estimate(*clips[name], 0, probes=3, unsqueeze=False, backend=RefRegisterBackend())
    r = _residual(res, amap)
    print(f"{name}: {res['status']} map {res['map']} scores {res['score']} residual {r:.3f} px")
    assert res["status"] == "registered" and res["probe_frames"] == [0, 1, 2] and min(res["score"]) >= 0.5
    assert r <= 1.0
    assert (res["eye_size"], res["guide_size"], res["unsqueeze"]) == (list(EYE), list(GUIDE), False)


def test_flat_probes_do_not_vote_and_all_flat_is_undetermined(tmp_path):
    from video_3d_pipeline import register as R
    amap, bars = MAPS["crop"]
    one = R.estimate(*_clip_pair(tmp_path, "oneflat", amap, bars, flat=(1,)), 0, probes=3, unsqueeze=False, backend=RefRegisterBackend())
    assert one["status"] == "registered" and one["probes_x"][1] is None and one["probes_y"][1] is None and _residual(one, amap) <= 1.0
    flat = R.estimate(*_clip_pair(tmp_path, "flat", amap, bars, flat=(0, 1, 2)), 0, probes=3, unsqueeze=False, backend=RefRegisterBackend())
    assert (flat["status"], flat["map"]) == ("undetermined", R.IDENTITY)


def test_a_clip_that_switches_framing_is_inconsistent(tmp_path):
    from video_3d_pipeline import register as R
    a, b = _clip_pair(tmp_path, "a", *MAPS["letterbox"]), _clip_pair(tmp_path, "b", *MAPS["identity"])
    sbs, g = np.load(a[0]), np.load(a[1])
    sbs[2], g[2] = np.load(b[0])[2], np.load(b[1])[2]
    np.save(tmp_path / "mix_sbs.npy", sbs)
    np.save(tmp_path / "mix_g.npy", g)
    res = R.estimate(str(tmp_path / "mix_sbs.npy"), str(tmp_path / "mix_g.npy"), 0, probes=3, unsqueeze=False, backend=RefRegisterBackend())
    assert (res["status"], res["map"]) == ("inconsistent", R.IDENTITY)


def test_estimate_refuses_bad_input(clips, tmp_path):
    from video_3d_pipeline import register as R
    for kw in (dict(probes=0), dict(probes=65), dict(bins=7), dict(bins=1025), dict(min_score=float("nan"))):
        with pytest.raises(ValueError):
            R.estimate(*clips["crop"], 0, backend=RefRegisterBackend(), **kw)
    with pytest.raises(ValueError, match="Could not read video info"):
        R.estimate(str(tmp_path / "none.npy"), clips["crop"][1], 0, backend=RefRegisterBackend())
    for text in ("1,0,1", "1,0,x,0", "0,0,1,0", "1,0,-1,0", "1,0,1,inf"):
        with pytest.raises(ValueError, match="--spatial-map"):
            R.parse_map(text)


# ---------------------------------------------------------------- alignment file
TEN = ("video1_path", "video2_path", "time_offset_seconds", "offset_frames", "correlation_strength", "frame_duration", "video1_fps",
       "video2_fps", "sample_rate", "audio_length_analyzed")


class AlignBackend(RefRegisterBackend):
    """the refinement's stand-in of tests/test_framematch_host.py and the registration's in one"""

    def __init__(self):
        from test_framematch_host import RefMatchBackend
        m = RefMatchBackend()
        self.sbs_left_signatures, self.guide_signatures, self.signature_scores, self.read_scores = \
            m.sbs_left_signatures, m.guide_signatures, m.signature_scores, m.read_scores


def _align(clips, name, tmp_path, *extra):
    from video_3d_pipeline import align
    rc = align.main([*clips[name], "--work-dir", str(tmp_path), "--no-unsqueeze", *extra], backend=AlignBackend())
    f = tmp_path / "alignment_data.json"
    return rc, (json.loads(f.read_text()) if f.exists() else None), str(f)


def test_align_cli_writes_the_block_and_it_round_trips(clips, tmp_path, capsys):
    from video_3d_pipeline import register as R
    rc, plain, _ = _align(clips, "letterbox", tmp_path / "plain", "--video-only", "--refine-window", "2", "--refine-probes", "1")
    assert rc == 0 and "spatial" not in plain
    rc, data, path = _align(clips, "letterbox", tmp_path / "reg", "--video-only", "--refine-window", "2", "--refine-probes", "1", "--register-spatial")
    assert rc == 0 and list(data)[:10] == list(TEN) and {k: v for k, v in data.items() if k != "spatial"} == plain
    sp = data["spatial"]
    assert set(sp) >= {"status", "map", "map_q16", "score", "probe_frames", "probes_x", "probes_y", "eye_size", "guide_size", "unsqueeze", "parameters"}
    assert (sp["status"], sp["eye_size"], sp["guide_size"], sp["unsqueeze"]) == ("registered", list(EYE), list(GUIDE), False)
    assert sp["parameters"]["bins"] == 512 and sp["parameters"]["probes"] == 3 and sp["parameters"]["min_score"] == 0.5
    assert len(sp["probes_x"]) == 3 and set(sp["probes_x"][0]) == {"a", "b", "A", "B", "score"}
    assert "Spatial registration: registered" in capsys.readouterr().out
    want = R.estimate(*clips["letterbox"], data["guide_start_frame"], unsqueeze=False, backend=RefRegisterBackend())
    assert tuple(sp["map"]) == want["map"] and sp["map_q16"] == want["map_q16"]
    # the map of the file is the map of the estimate, bit for bit, and so are the warp's integers
    got = R.resolve(path, eye_size=EYE, guide_size=GUIDE, unsqueeze=False)
    assert got["map"] == want["map"] and got["source"] == path
    assert R.warp_q16(got["map"], EYE, GUIDE) == R.warp_q16(want["map"], EYE, GUIDE)
    assert R.normalised(*sp["map_q16"][1], EYE[1], GUIDE[1]) == tuple(sp["map"][2:])
    # flags reach the estimate
    rc, data, _ = _align(clips, "crop", tmp_path / "flags", "--video-only", "--refine-window", "2", "--refine-probes", "1", "--register-spatial",
                         "--register-probes", "2", "--register-bins", "128", "--register-min-score", "0.99")
    assert rc == 0 and data["spatial"]["parameters"]["probes"] == 2 and data["spatial"]["parameters"]["bins"] == 128
    assert data["spatial"]["status"] == "undetermined" and data["spatial"]["map"] == [1.0, 0.0, 1.0, 0.0] and len(data["spatial"]["probes_x"]) == 2


def _block_file(tmp_path, name="a.json", **over):
    block = dict(status="registered", map=[1.0, 0.0, 0.875, 0.0625], eye_size=[SW, SH], guide_size=[2 * SW, 2 * SH], unsqueeze=True)
    block.update(over)
    f = tmp_path / name
    f.write_text(json.dumps({"time_offset_seconds": 0.0, "guide_start_frame": 0, "spatial": block}))
    return str(f)


def test_resolve_and_its_refusals(tmp_path):
    from video_3d_pipeline import register as R
    sizes = dict(eye_size=(SW, SH), guide_size=(2 * SW, 2 * SH), unsqueeze=True)
    f = _block_file(tmp_path)
    assert R.resolve(f, **sizes)["map"] == (1.0, 0.0, 0.875, 0.0625)
    assert R.resolve(f, no_spatial=True, **sizes) is None and R.resolve(None, **sizes) is None
    assert R.resolve(f, spatial_map="0.9,0.05,0.9,0.05", **sizes) == dict(map=(0.9, 0.05, 0.9, 0.05), source="--spatial-map", eye_size=None)
    assert R.resolve(None, spatial_map="1,0,1,0") is None                                               # the identity applies nothing
    assert R.resolve(_block_file(tmp_path, "i.json", map=[1.0, 0.0, 1.0, 0.0]), **sizes) is None
    for status in ("undetermined", "inconsistent"):
        assert R.resolve(_block_file(tmp_path, "u.json", status=status), **sizes) is None
    nob = tmp_path / "nob.json"
    nob.write_text(json.dumps({"time_offset_seconds": 0.0}))
    assert R.resolve(str(nob), **sizes) is None
    with pytest.raises(ValueError, match="unsqueeze=False"):
        R.resolve(_block_file(tmp_path, "s.json", unsqueeze=False), **sizes)
    with pytest.raises(ValueError, match="left-eye plane of 96x48"):
        R.resolve(_block_file(tmp_path, "e.json", eye_size=[96, 48]), **sizes)
    with pytest.raises(ValueError, match="4K frame of 400x96"):
        R.resolve(_block_file(tmp_path, "g.json", guide_size=[400, 96]), **sizes)
    assert R.manifest_entries(None) == {} and R.manifest_entries(R.resolve(f, **sizes)) == \
        {"spatial_map": [1.0, 0.0, 0.875, 0.0625], "spatial_map_source": f}


# ---------------------------------------------------------------- drivers
class WarpPipelineBackend(OraclePipelineBackend):
    """records every call the driver makes after the u16 samples; the warp is the restatement's"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def guide_luma(self, frames, height, width, capacity):
        self.calls.append(("guide_luma", len(frames)))
        return super().guide_luma(frames, height, width, capacity)

    def warp_u16(self, u16, q, size):
        self.calls.append(("warp_u16", tuple(q), tuple(size), np.asarray(u16).shape))
        return RR.warp(np.asarray(u16).view(np.uint16), *q, 0, *size)

    def guided_upscale_u16(self, u16, luma, r, eps):
        self.calls.append(("guided_upscale_u16", np.asarray(u16).shape, np.asarray(u16).tobytes()))
        return super().guided_upscale_u16(u16, luma, r, eps)


class WarpUpscaleBackend(OracleUpscaleBackend):
    def __init__(self):
        self.calls = []

    def warp_u16(self, depth_u16, q, size):
        self.calls.append(("warp_u16", tuple(q), tuple(size), depth_u16.shape, depth_u16.dtype))
        return RR.warp(depth_u16[None], *q, 0, *size)[0].astype(np.float32)

    def upscale_u16(self, depth_lo, guide, r, eps):
        self.calls.append(("upscale_u16", depth_lo.shape, depth_lo.dtype, depth_lo.tobytes()))
        return super().upscale_u16(depth_lo, guide, r, eps)


@pytest.fixture()
def run_clips(tmp_path):
    from video_3d_pipeline import synthetic as syn
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(3)])
    guides = np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(3)])
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", guides)
    return str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy")


def _pipe(tmp_path, run_clips, tag, spatial):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    be = WarpPipelineBackend()
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"w_{tag}"), batch_size=2, stereo_only=True, guide_batch=2, backend=be)
    out = pipe.run(*run_clips, output_path=str(tmp_path / f"{tag}.json"), keep_depth_maps=True, spatial=spatial)
    man = json.loads(open(out).read())
    cache = pipe.extractor.get_cache_path(run_clips[0], 0, 3)
    man.pop("frames_dir")
    return be.calls, man, _pngs(str(tmp_path / f"{tag}_frames")), cache.name, _pngs(cache)


class _Args:
    def __init__(self, video, video_4k, **kw):
        self.video, self.video_4k, self.alignment_file, self.no_spatial, self.spatial_map, self.no_unsqueeze = video, video_4k, None, False, None, False
        self.__dict__.update(kw)


def test_pipeline_without_a_map_is_unchanged_and_with_one_warps_before_the_filter(tmp_path, run_clips):
    from video_3d_pipeline import register as R
    from video_3d_pipeline.pipeline import _resolve_spatial
    plain = _pipe(tmp_path, run_clips, "plain", None)
    assert not any(c[0] == "warp_u16" for c in plain[0]) and "spatial_map" not in plain[1]
    f = _block_file(tmp_path)
    cases = {"no file": _Args(*run_clips), "no-spatial": _Args(*run_clips, alignment_file=f, no_spatial=True),
             "identity": _Args(*run_clips, spatial_map="1,0,1,0"),
             "identity block": _Args(*run_clips, alignment_file=_block_file(tmp_path, "i.json", map=[1.0, 0.0, 1.0, 0.0])),
             "not registered": _Args(*run_clips, alignment_file=_block_file(tmp_path, "u.json", status="inconsistent"))}
    for tag, args in cases.items():
        spatial = _resolve_spatial(args, R.resolve)
        assert spatial is None, tag
    assert _pipe(tmp_path, run_clips, "none", None) == plain                       # calls, manifest, 4K bytes, cache key, depth maps
    # a block estimated with another setting is refused before anything runs
    with pytest.raises(ValueError, match="unsqueeze"):
        _resolve_spatial(_Args(*run_clips, alignment_file=f, no_unsqueeze=True), R.resolve)
    with pytest.raises(ValueError, match="left-eye plane"):
        _resolve_spatial(_Args(*run_clips, alignment_file=_block_file(tmp_path, "e.json", eye_size=[SW // 2, SH])), R.resolve)
    spatial = _resolve_spatial(_Args(*run_clips, alignment_file=f), R.resolve)
    calls, man, pngs, key, depth = _pipe(tmp_path, run_clips, "map", spatial)
    w = R.warp_q16(spatial["map"], (SW, SH), (2 * SW, 2 * SH))
    assert [c[0] for c in calls] == ["guide_luma", "warp_u16", "guided_upscale_u16"] * 2
    assert [c[1:] for c in calls if c[0] == "warp_u16"] == [(w["q"], (SW, SH), (2, SH, SW)), (w["q"], (SW, SH), (1, SH, SW))]
    assert (key, depth) == (plain[3], plain[4])                                    # the depth cache: same key, same bytes
    assert pngs != plain[2] and list(pngs) == list(plain[2])
    assert man["spatial_map"] == [1.0, 0.0, 0.875, 0.0625] and man["spatial_map_source"] == f
    assert {k: v for k, v in man.items() if not k.startswith("spatial_")} == plain[1]
    # the filter saw the restatement's warp of the very planes the plain run filtered
    for got, before in zip([c for c in calls if c[0] == "guided_upscale_u16"], [c for c in plain[0] if c[0] == "guided_upscale_u16"]):
        lo = np.frombuffer(before[2], np.uint16).reshape(before[1])
        assert got[1] == before[1] and got[2] == RR.warp(lo, *w["q"], 0, *w["size"]).tobytes()


def _upscale_cli(tmp_path, run_clips, ddir, tag, *extra):
    from video_3d_pipeline import upscale
    be = WarpUpscaleBackend()
    out = tmp_path / f"up_{tag}.json"
    rc = upscale.main([str(ddir), run_clips[1], "--output", str(out), *extra], backend=be)
    man = json.loads(out.read_text()) if out.exists() else None
    pngs = _pngs(man.pop("frames_dir")) if man else None
    return rc, be.calls, man, pngs


def test_upscale_cli_without_a_map_is_unchanged_and_with_one_warps_the_u16_samples(tmp_path, run_clips, capsys):
    from video_3d_pipeline import register as R
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    from video_3d_pipeline.utils import read_png16
    from test_host import OracleStereoBackend
    work = str(tmp_path / "d")
    ddir = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=2, stereo_only=True, backend=OracleStereoBackend()).process_video_sbs(run_clips[0])
    rc, plain_calls, plain_man, plain = _upscale_cli(tmp_path, run_clips, ddir, "plain")
    assert rc == 0 and [c[0] for c in plain_calls] == ["upscale_u16"] * 3 and all(c[2] == np.float32 for c in plain_calls)
    f = _block_file(tmp_path)
    for tag, extra in (("nofile", ()), ("nospatial", ("--alignment-file", f, "--no-spatial")), ("ident", ("--spatial-map", "1,0,1,0")),
                       ("undet", ("--alignment-file", _block_file(tmp_path, "u.json", status="undetermined")))):
        rc, calls, man, pngs = _upscale_cli(tmp_path, run_clips, ddir, tag, *extra)
        assert rc == 0 and calls == plain_calls and pngs == plain and man == plain_man, tag
    rc, calls, man, pngs = _upscale_cli(tmp_path, run_clips, ddir, "map", "--alignment-file", f)
    w = R.warp_q16((1.0, 0.0, 0.875, 0.0625), (SW, SH), (2 * SW, 2 * SH))
    assert rc == 0 and [c[0] for c in calls] == ["warp_u16", "upscale_u16"] * 3
    assert all(c[1:] == (w["q"], (SW, SH), (SH, SW), np.uint16) for c in calls if c[0] == "warp_u16")
    assert man["spatial_map"] == [1.0, 0.0, 0.875, 0.0625] and man["spatial_map_source"] == f
    assert {k: v for k, v in man.items() if not k.startswith("spatial_")} == plain_man and pngs != plain
    # the composition of the stages: the stand-in's filter on the restatement's warp of the depth map's samples
    d0 = read_png16(sorted(ddir.glob("depth_*.png"))[0])
    be = OracleUpscaleBackend()
    want = be.upscale_u16(RR.warp(d0[None], *w["q"], 0, *w["size"])[0].astype(np.float32), np.load(run_clips[1])[0], 8, 1e-3)
    (tmp_path / "got.png").write_bytes(pngs["depth4k_000000.png"])
    got = read_png16(str(tmp_path / "got.png"))
    assert np.array_equal(got, want)
    # --spatial-map without a file; a block of another size is refused with a message
    rc, calls, man, _ = _upscale_cli(tmp_path, run_clips, ddir, "hand", "--spatial-map", "1,0,0.875,0.0625")
    assert rc == 0 and man["spatial_map_source"] == "--spatial-map" and [c[1] for c in calls if c[0] == "warp_u16"] == [w["q"]] * 3
    capsys.readouterr()
    rc, _, man, _ = _upscale_cli(tmp_path, run_clips, ddir, "size", "--alignment-file", _block_file(tmp_path, "e.json", eye_size=[SW // 2, SH]))
    assert rc == 1 and "left-eye plane of 96x48" in capsys.readouterr().out
    rc, _, man, _ = _upscale_cli(tmp_path, run_clips, ddir, "gsize", "--alignment-file", _block_file(tmp_path, "g.json", guide_size=[400, 96]))
    assert rc == 1 and "4K frame of 400x96" in capsys.readouterr().out
