"""--min-disparity on the host, without a GPU: the option and its refusals, the cache key, the manifests, the rebias inside
HipStereoBackend, the cropped reprojection call of the binding, `auto`, and -- with the flag off -- that every call, key and byte
is the parent's.  Stand-in backends as in test_quality_host.py; the stand-in matcher at a window m is the C oracle on the shifted
left view (sgbm_mind_ref.from_oracle)."""
import contextlib
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import quality_ref as QR
import sgbm_mind_ref as MR
from oracle import oracle as O
from test_fill_host import _FakeNative, _hip_backend
from test_quality_host import QualityPipelineBackend, QualityStereoBackend
from test_temporal_host import _pngs

W, H, NF = 320, 120, 4


def disp_at(l, r, m):
    """the stand-in matcher: int16 disparity of the window [m, m + 64), true values, invalid = 16 (m - 1)"""
    if m == 0:
        return O.sgbm_compute(l, r)
    return MR.finish(MR.from_oracle(O.sgbm_raw, l, r, m), m, O)


def rebiased(l, r, m):
    return (disp_at(l, r, m) - 16 * m).astype(np.int16)


def cropped_reproj(L, R, rel, m, bad=16):
    k = -m
    w = L.shape[2] - k
    return QR.reproj(np.ascontiguousarray(L[:, :, :w]), np.ascontiguousarray(R[:, :, k:]), np.ascontiguousarray(rel[:, :, :w]), bad)


class _MindMethods:
    """what HipStereoBackend widens for the flag, NumPy"""

    def sbs_to_disparity(self, frames, unsqueeze, mono_provider=None, fill_holes=False, min_disparity=0):
        self.__dict__.setdefault("calls", []).append(("sbs", len(frames), min_disparity))
        pairs = [O.sbs_to_gray(f, unsqueeze) for f in frames]
        self._lg, self._rg = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        self._disp = np.stack([rebiased(l, r, min_disparity) for l, r in pairs])
        return np.stack([O.disp_to_depth(d) for d in self._disp])

    def quality_reproj(self, n, bad_thr, min_disparity=0):
        self.__dict__.setdefault("calls", []).append(("reproj", n, min_disparity))
        return cropped_reproj(self._lg[:n], self._rg[:n], self._disp[:n], min_disparity, bad_thr)

    def min_disparity_score(self, frames, unsqueeze, min_disparity):
        self.__dict__.setdefault("calls", []).append(("score", len(frames), min_disparity))
        pairs = [O.sbs_to_gray(f, unsqueeze) for f in frames]
        L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        rec = cropped_reproj(L, R, np.stack([rebiased(l, r, min_disparity) for l, r in pairs]), min_disparity)
        return int((rec[:, 1] - rec[:, 4]).sum())


class MindStereoBackend(_MindMethods, QualityStereoBackend):
    pass


class MindPipelineBackend(_MindMethods, QualityPipelineBackend):
    pass


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """a four-frame side-by-side clip whose scene lies behind the screen (the left view of temporal_clip moved 24 columns), a
    random 4K clip, and the gray planes"""
    from video_3d_pipeline import synthetic as syn
    L, R, _ = syn.temporal_clip(W + 24, H, NF)
    L, R = np.ascontiguousarray(L[:, :, 24:]), np.ascontiguousarray(R[:, :, :W])
    d = tmp_path_factory.mktemp("mclips")
    np.save(d / "sbs.npy", np.repeat(np.concatenate([L, R], axis=2)[..., None], 3, axis=3))
    np.save(d / "v4k.npy", np.random.default_rng(4).integers(0, 256, (NF, 2 * H, 2 * W, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy"), L, R


def _depth_cli(tmp_path, sbs, tag, backend, **kw):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    work = str(tmp_path / f"cli_{tag}")
    ex = HybridStereoDepthExtractor(work_dir=work, cache_dir=work, batch_size=3, stereo_only=True, unsqueeze_sbs=False, backend=backend, **kw)
    return ex, ex.process_video_sbs(sbs)


def _pipeline(tmp_path, sbs, v4k, tag, backend, run_kw=None, **kw):
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"pipe_{tag}"), batch_size=3, stereo_only=True, unsqueeze_sbs=False, guide_batch=2,
                                backend=backend, **kw)
    out = pipe.run(sbs, v4k, output_path=str(tmp_path / f"pipe_{tag}.json"), **(run_kw or {}))
    return pipe, json.loads(open(out).read())


def _maps(d, n=NF):
    from video_3d_pipeline.utils import read_png16
    return np.stack([read_png16(os.path.join(str(d), f"depth_{i:06d}.png")) for i in range(n)])


# ---------------------------------------------------------------- the option itself

def test_option_values_and_refusals():
    from video_3d_pipeline.depth import (HybridStereoDepthExtractor, calibration_frames, check_min_disparity, min_disparity_argument,
                                         min_disparity_suffix)
    import argparse
    assert [check_min_disparity(v) for v in (0, -1, -64, np.int64(-32), "auto")] == [0, -1, -64, -32, "auto"]
    for bad in (1, -65, True, -1.0, "-32", "Auto", None):
        with pytest.raises(ValueError):
            check_min_disparity(bad)
        with pytest.raises(ValueError):
            HybridStereoDepthExtractor(work_dir="unused", backend=QualityStereoBackend(), min_disparity=bad)
    with pytest.raises(ValueError):
        check_min_disparity("auto", allow_auto=False)
    assert min_disparity_argument("-32") == -32 and min_disparity_argument("auto") == "auto" and min_disparity_argument("0") == 0
    for bad in ("1", "-65", "x"):
        with pytest.raises(argparse.ArgumentTypeError):
            min_disparity_argument(bad)
    assert min_disparity_suffix(0) == "" and min_disparity_suffix(-32) == "_mind-32"
    assert calibration_frames(10, 100) == [10 + 6 + 12 * j for j in range(8)] and calibration_frames(5, 3) == [5, 6, 7]
    assert calibration_frames(0, 8) == list(range(8)) and calibration_frames(0, 17) == [1 + 2 * j for j in range(8)]


def test_process_frame_batch_takes_an_integer_only():
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.depth import HybridStereoDepthExtractor
    pairs = [O.split_sbs(syn.sbs_frame(192, 48, 0), True)]
    with pytest.raises(ValueError, match="auto"):
        HybridStereoDepthExtractor(work_dir="unused", stereo_only=True, backend=QualityStereoBackend(), min_disparity="auto").process_frame_batch(pairs)

    class Pairs:
        def pairs_to_disparity(self, pairs, monos=None, fill_holes=False, **kw):
            self.kw = kw
            return [np.zeros((2, 2), np.float32) for _ in pairs]

    for m, want in ((0, {}), (-16, {"min_disparity": -16})):
        be = Pairs()
        HybridStereoDepthExtractor(work_dir="unused", stereo_only=True, backend=be, min_disparity=m).process_frame_batch(pairs)
        assert be.kw == want


def test_cache_key(tmp_path):
    from video_3d_pipeline.depth import HybridStereoDepthExtractor

    def name(**kw):
        ex = HybridStereoDepthExtractor(work_dir=str(tmp_path), cache_dir=str(tmp_path), backend=QualityStereoBackend(), **kw)
        return ex.get_cache_path("clip.npy", 3, 40).name

    md5 = lambda suffix: "depth_" + hashlib.md5(f"clip.npy_3_40_Intel/dpt-large_True{suffix}".encode()).hexdigest()[:16]
    assert name() == name(min_disparity=0) == md5("")
    assert name(min_disparity=-32) == md5("_mind-32") and name(min_disparity=-32, fill_holes=True) == md5("_fill1_mind-32")
    with pytest.raises(ValueError, match="auto"):
        name(min_disparity="auto")


def test_command_lines_reach_the_constructors(clip):
    from video_3d_pipeline import depth as depth_mod, pipeline as pipe_mod
    sbs, v4k = clip[:2]
    for mod, name, argv in ((depth_mod, "HybridStereoDepthExtractor", [sbs]), (pipe_mod, "SbsTo4kDepthPipeline", [sbs, v4k])):
        seen = {}
        orig = getattr(mod, name)

        class Spy(orig):
            def __init__(self, **kw):
                seen.update(kw)
                raise RuntimeError("stop here")

        setattr(mod, name, Spy)
        try:
            assert mod.main(argv + ["--min-disparity", "-32"]) == 1 and seen["min_disparity"] == -32
            seen.clear()
            assert mod.main(argv + ["--min-disparity", "auto"]) == 1 and seen["min_disparity"] == "auto"
            seen.clear()
            assert mod.main(argv) == 1 and seen and "min_disparity" not in seen          # off: the parent's constructor call
            seen.clear()
            assert mod.main(argv + ["--min-disparity", "0"]) == 1 and seen and "min_disparity" not in seen
            for bad in ("1", "-65"):
                with pytest.raises(SystemExit):
                    mod.main(argv + ["--min-disparity", bad])
        finally:
            setattr(mod, name, orig)


# ---------------------------------------------------------------- flag off: nothing changes

def test_flag_off_changes_nothing(tmp_path, clip):
    """the parent's stand-ins (no `min_disparity` keyword anywhere: passing one raises) with the flag spelt out as 0"""
    sbs, v4k = clip[:2]
    ex0, plain_dir = _depth_cli(tmp_path, sbs, "plain", QualityStereoBackend(), quality_report=True)
    ex1, off_dir = _depth_cli(tmp_path, sbs, "off", QualityStereoBackend(), quality_report=True, min_disparity=0)
    assert off_dir.name == plain_dir.name and sorted(os.listdir(off_dir)) == sorted(os.listdir(plain_dir))
    assert _pngs(off_dir) == _pngs(plain_dir) and (off_dir / "quality.json").read_text() == (plain_dir / "quality.json").read_text()
    assert "baseline_disparity" not in json.loads((off_dir / "quality.json").read_text()) and not (off_dir / "min_disparity.json").exists()
    assert ex1.manifest_extra().keys() == ex0.manifest_extra().keys() == {"quality"}
    _, plain = _pipeline(tmp_path, sbs, v4k, "plain", QualityPipelineBackend(), run_kw=dict(keep_depth_maps=True))
    pipe, off = _pipeline(tmp_path, sbs, v4k, "off", QualityPipelineBackend(), run_kw=dict(keep_depth_maps=True), min_disparity=0)
    assert set(off) == set(plain) and "min_disparity" not in off and "min_disparity_scores" not in off
    assert _pngs(off["frames_dir"]) == _pngs(plain["frames_dir"]) and len(_pngs(off["frames_dir"])) == NF


# ---------------------------------------------------------------- flag on

def test_depth_cli_and_pipeline_with_a_window(tmp_path, clip, capsys):
    sbs, v4k, L, R = clip
    m = -32
    rel = np.stack([rebiased(l, r, m) for l, r in zip(L, R)])
    assert rel.min() == -16 and (rel[rel != -16] >= 0).all() and rel.max() <= 1023
    assert (rel[:, :, :64 + m] == -16).all() and (rel[:, :, W + m:] == -16).all() and (rel >= 16).mean() > 0.5
    be = MindStereoBackend()
    ex, ddir = _depth_cli(tmp_path, sbs, "on", be, min_disparity=m, quality_report=True)
    _, plain_dir = _depth_cli(tmp_path, sbs, "plain", QualityStereoBackend())
    assert ddir.name != plain_dir.name
    assert ddir.name == "depth_" + hashlib.md5(f"{sbs}_0_{NF}_Intel/dpt-large_False_mind-32".encode()).hexdigest()[:16]
    assert [c for c in be.calls if c[0] == "sbs"] == [("sbs", 3, m), ("sbs", 1, m)] and [c for c in be.calls if c[0] == "reproj"] == [("reproj", 3, m), ("reproj", 1, m)]
    assert np.array_equal(_maps(ddir), np.stack([O.depth_to_u16(O.disp_to_depth(d)) for d in rel]))
    assert json.loads((ddir / "min_disparity.json").read_text()) == {"min_disparity": m}
    rep = json.loads((ddir / "quality.json").read_text())
    assert rep["baseline_disparity"] == m and ex.manifest_extra()["min_disparity"] == m and ex.manifest_extra()["quality"]["baseline_disparity"] == m
    assert [[f[k] for k in QR.REPROJ_FIELDS] for f in rep["frames"]] == cropped_reproj(L, R, rel, m).tolist()
    tot = rep["reproj"]["totals"]
    assert tot["sad"] < tot["sad0"] / 2                        # the true disparity explains the left view; the baseline d = m does not
    out = capsys.readouterr().out
    assert f"baseline_disparity" in out and f"[{m}, {m + 64})" in out
    # the one-pass pipeline: the same depth maps, the key in the manifest
    pipe, man = _pipeline(tmp_path, sbs, v4k, "on", MindPipelineBackend(), run_kw=dict(keep_depth_maps=True), min_disparity=m)
    assert man["min_disparity"] == m and "min_disparity_scores" not in man
    cache = pipe.extractor.get_cache_path(sbs, 0, NF)
    assert cache.name == ddir.name and _pngs(cache) == _pngs(ddir)


def test_auto_scores_the_candidates_and_shares_the_cache_of_its_choice(tmp_path, clip, capsys):
    from video_3d_pipeline.depth import MIN_DISPARITY_CANDIDATES, choose_min_disparity
    sbs, v4k, L, R = clip
    scores = {}
    for m in MIN_DISPARITY_CANDIDATES:
        rec = cropped_reproj(L, R, np.stack([rebiased(l, r, m) for l, r in zip(L, R)]), m)
        scores[m] = int((rec[:, 1] - rec[:, 4]).sum())
    want = choose_min_disparity(scores)
    print("scores", scores, "->", want)
    assert want != 0                                           # the clip lies behind the screen: the window has to move
    be = MindStereoBackend()
    ex, ddir = _depth_cli(tmp_path, sbs, "auto", be, min_disparity="auto")
    assert ex.min_disparity == want and ex.min_disparity_scores == {str(m): s for m, s in scores.items()}
    assert [c for c in be.calls if c[0] == "score"] == [("score", NF, m) for m in MIN_DISPARITY_CANDIDATES]
    assert all(c[2] == want for c in be.calls if c[0] == "sbs")
    out = capsys.readouterr().out
    assert "--min-disparity auto" in out and all(f"m={m}: {s}" in out for m, s in scores.items())
    _, explicit = _depth_cli(tmp_path, sbs, "explicit", MindStereoBackend(), min_disparity=want)
    assert explicit.name == ddir.name and _pngs(explicit) == _pngs(ddir)
    assert json.loads((ddir / "min_disparity.json").read_text()) == {"min_disparity": want, "min_disparity_scores": {str(m): s for m, s in scores.items()}}
    _, man = _pipeline(tmp_path, sbs, v4k, "auto", MindPipelineBackend(), min_disparity="auto")
    assert man["min_disparity"] == want and man["min_disparity_scores"] == {str(m): s for m, s in scores.items()}


# ---------------------------------------------------------------- HipStereoBackend and the binding

def test_hip_backend_rebiases_right_after_the_matcher(capsys):
    import torch
    frames = [np.zeros((4, 16, 3), np.uint8)] * 2
    made = []

    class Native(_FakeNative):
        def __init__(self, timeouts=0):
            super().__init__(timeouts)
            outer, Base = self, self.StereoSGBM

            class StereoSGBM(Base):
                def __init__(self, W, H, n, device=None, **params):
                    made.append(params)
                    self.m = params.get("minDisparity", 0)

                def compute(self, lg, rg, out=None):
                    outer.log.append("compute")
                    out.fill_(16 * (self.m - 1))                           # the matcher's INVALID at this window
                    out[:, :, 1] = 16 * self.m + 5
                    return out

            self.StereoSGBM = StereoSGBM

        def fill_holes_disp16_batch(self, disp, out=None, ws=None):
            assert disp.min() == -16 and disp[0, 0, 1] == 5                # the stage after the matcher reads rebiased values
            return super().fill_holes_disp16_batch(disp, out, ws)

        def disp_to_depth(self, disp, out=None):
            self.seen = disp.clone()
            return super().disp_to_depth(disp, out)

    nat = Native()
    _hip_backend(nat).sbs_to_disparity(frames, True)
    assert made == [{}] and nat.log == ["gray", "compute", "depth"]        # flag off: today's create and today's sequence
    for timeouts, log in ((0, ["gray", "compute", "fill", "depth"]), (1, ["gray", "compute", "lockstep-off", "compute", "fill", "depth"])):
        made.clear()
        nat = Native(timeouts)
        be = _hip_backend(nat)
        be.sbs_to_disparity(frames, True, fill_holes=True, min_disparity=-32)
        assert made == [{"minDisparity": -32}] and nat.log == log           # one rebias, behind the lock-step recompute
        assert (nat.seen[:, :, 1] == 5).all() and (nat.seen[:, :, 0] == -16).all()
        be.sbs_to_disparity(frames, True, min_disparity=-32)
        assert len(made) == 1                                               # the matcher is kept between passes
        be.sbs_to_disparity(frames, True, min_disparity=-16)
        assert made[-1] == {"minDisparity": -16} and len(made) == 2         # and made again for another window
    capsys.readouterr()


def test_binding_crops_the_reprojection_call(monkeypatch):
    """quality_reproj_batch(right_shift=k): left pointer unchanged, right pointer + k bytes, width W - k at the pitch W, the
    disparity dense at W - k -- a fake entry that reads exactly those bytes gives quality_ref on the cropped arrays"""
    import torch
    from video_3d_pipeline import _native as N
    n, h, w, k = 2, 6, 40, 17
    rng = np.random.default_rng(3)
    L, R = rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    rel = rng.integers(-16, 300, (n, h, w)).astype(np.int16)
    tl, tr, td = torch.from_numpy(L), torch.from_numpy(R), torch.from_numpy(rel)
    calls = []

    def read(ptr, count, dtype):
        return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype).copy()

    class Lib:
        def v3d_quality_reproj_ws_bytes(self, n_, W_, H_):
            return 64

        def v3d_quality_reproj_batch(self, l, r, n_, W_, H_, pitch, fs, d, ds, bad, out, ws, stream):
            calls.append((l.value, r.value, n_, W_, H_, pitch, fs, ds, bad))
            rows = lambda p: np.stack([[read(p + f * fs + y * pitch, W_, np.uint8) for y in range(H_)] for f in range(n_)])
            disp = np.stack([read(d.value + 2 * f * ds, W_ * H_, np.int16).reshape(H_, W_) for f in range(n_)])
            out[:] = torch.from_numpy(QR.reproj(rows(l.value), rows(r.value), disp, bad).astype(np.int64))
            return 0

    def clip(t, dtype, what):
        assert t.dtype == dtype and t.is_contiguous()
        return C.c_void_p(t.data_ptr()), t.stride(0)

    monkeypatch.setattr(N, "lib", lambda: Lib())
    monkeypatch.setattr(N, "_clip", clip)
    monkeypatch.setattr(N, "_dev", lambda t, dtype, what: t)
    monkeypatch.setattr(N, "_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", contextlib.nullcontext)
    got = N.quality_reproj_batch(tl, tr, td, 16, right_shift=k).numpy()
    assert calls == [(tl.data_ptr(), tr.data_ptr() + k, n, w - k, h, w, h * w, h * (w - k), 16)]
    assert np.array_equal(got, QR.reproj(L[:, :, :w - k], R[:, :, k:], rel[:, :, :w - k], 16))
    calls.clear()
    got0 = N.quality_reproj_batch(tl, tr, td, 16).numpy()                     # off: the parent's call
    assert calls == [(tl.data_ptr(), tr.data_ptr(), n, w, h, w, h * w, h * w, 16)] and np.array_equal(got0, QR.reproj(L, R, rel, 16))
    with pytest.raises(ValueError):
        N.quality_reproj_batch(tl, tr, td, 16, right_shift=w)
