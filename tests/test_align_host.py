"""Audio alignment on the host: load_audio on every container, the aligner's refusals (all before any GPU call), the
quality grades, the CLI, and --alignment-file on the upscale and pipeline CLIs.  No GPU needed."""
import ctypes
import json
import os
import re
import wave

import numpy as np
import pytest

from conftest import ROOT


def _write_wav(path, samples_i16, rate):
    a = np.asarray(samples_i16, dtype=np.int16)
    ch = 1 if a.ndim == 1 else a.shape[1]
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ch)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(a.astype("<i2").tobytes())


def _frames(n=2, H=8, W=12):
    return np.zeros((n, H, W, 3), np.uint8)


def _i16(n, ch, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-30000, 30000, (n, ch) if ch > 1 else n).astype(np.int16)


# ---------------------------------------------------------------- load_audio

@pytest.mark.parametrize("ch", [1, 2])
def test_load_audio_npz_int16(tmp_path, ch):
    from video_3d_pipeline.utils import load_audio
    a = _i16(1000, ch, ch)
    p = tmp_path / "clip.npz"
    np.savez(p, frames=_frames(), fps=24.0, audio=a, audio_rate=np.int32(8000))
    got, rate = load_audio(str(p))
    want = a.astype(np.float32) / 32768.0
    if ch > 1:
        want = want.mean(axis=1, dtype=np.float32)
    assert rate == 8000 and got.dtype == np.float32 and got.shape == (1000,)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("ch", [1, 2])
def test_load_audio_npz_float32(tmp_path, ch):
    from video_3d_pipeline.utils import load_audio
    rng = np.random.default_rng(5)
    a = rng.standard_normal((700, ch) if ch > 1 else 700).astype(np.float32)
    p = tmp_path / "clip.npz"
    np.savez(p, frames=_frames(), audio=a, audio_rate=22050)
    got, rate = load_audio(str(p))
    assert rate == 22050 and got.dtype == np.float32
    assert np.array_equal(got, a.mean(axis=1, dtype=np.float32) if ch > 1 else a)


@pytest.mark.parametrize("ch", [1, 2])
def test_load_audio_sidecar_wavs(tmp_path, ch):
    from video_3d_pipeline.utils import load_audio
    a = _i16(1234, ch, 10 + ch)
    want = a.astype(np.float32) / 32768.0
    if ch > 1:
        want = want.mean(axis=1, dtype=np.float32)
    np.save(tmp_path / "clip.npy", _frames())                       # .npy stack + clip.wav
    _write_wav(tmp_path / "clip.wav", a, 16000)
    d = tmp_path / "frames"                                          # PNG frame directory + audio.wav
    d.mkdir()
    from PIL import Image
    Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(d / "frame_000000.png")
    _write_wav(d / "audio.wav", a, 16000)
    for path in (tmp_path / "clip.npy", d, tmp_path / "clip.wav"):
        got, rate = load_audio(str(path))
        assert rate == 16000 and np.array_equal(got, want), path


def test_load_audio_truncates_to_max_seconds(tmp_path):
    from video_3d_pipeline.utils import load_audio
    a = _i16(10000, 2, 1)
    np.savez(tmp_path / "c.npz", frames=_frames(), audio=a, audio_rate=1000)
    got, rate = load_audio(str(tmp_path / "c.npz"), max_seconds=2.5)
    assert rate == 1000 and got.shape == (2500,)
    assert np.array_equal(got, (a[:2500].astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float32))
    _write_wav(tmp_path / "c.wav", a[:, 0], 1000)
    got, _ = load_audio(str(tmp_path / "c.wav"), max_seconds=0.0015)     # int(1.5) samples: no resampling, no rounding up
    assert got.shape == (1,)
    got, _ = load_audio(str(tmp_path / "c.wav"), max_seconds=300)
    assert got.shape == (10000,)


def test_load_audio_missing_pieces(tmp_path, monkeypatch):
    from video_3d_pipeline import utils
    with pytest.raises(FileNotFoundError):
        utils.load_audio(str(tmp_path / "nope.npz"))
    np.savez(tmp_path / "silent_film.npz", frames=_frames())
    with pytest.raises(LookupError):
        utils.load_audio(str(tmp_path / "silent_film.npz"))
    np.save(tmp_path / "nowav.npy", _frames())
    with pytest.raises(LookupError):
        utils.load_audio(str(tmp_path / "nowav.npy"))
    (tmp_path / "movie.mkv").write_bytes(b"\0" * 64)
    monkeypatch.setattr(utils.shutil, "which", lambda name: None)
    with pytest.raises(RuntimeError, match="ffmpeg"):
        utils.load_audio(str(tmp_path / "movie.mkv"))
    with wave.open(str(tmp_path / "u8.wav"), "wb") as w:            # 8-bit PCM: refused, not misread
        w.setnchannels(1); w.setsampwidth(1); w.setframerate(8000); w.writeframes(b"\x80" * 100)
    with pytest.raises(ValueError, match="16-bit"):
        utils.load_audio(str(tmp_path / "u8.wav"))


def test_load_audio_is_exported_through_utils_only():
    import video_3d_pipeline
    from video_3d_pipeline import utils
    assert callable(utils.load_audio)
    assert "load_audio" not in video_3d_pipeline.__all__


# ---------------------------------------------------------------- VideoAligner refusals

@pytest.fixture
def no_gpu(monkeypatch):
    """every refusal must come before the first GPU call"""
    from video_3d_pipeline import _native

    def boom(*a, **k):
        raise AssertionError("GPU call before the host checks")
    monkeypatch.setattr(_native, "align_audio", boom)
    monkeypatch.setattr(_native, "to_device", boom)


def _clip(path, audio=None, rate=22050, fps=24.0):
    kw = {} if audio is None else {"audio": audio, "audio_rate": rate}
    np.savez(path, frames=_frames(), fps=fps, **kw)
    return str(path)


def test_constructor_touches_nothing(tmp_path, no_gpu):
    from video_3d_pipeline.align import VideoAligner
    wd = tmp_path / "wd"
    VideoAligner(str(tmp_path / "a.npz"), str(tmp_path / "b.npz"), str(wd))
    assert not wd.exists()
    monkeypatch_cwd = os.getcwd()
    try:
        os.chdir(tmp_path)
        VideoAligner("a", "b")                                   # the default work_dir "temp_alignment"
        assert os.listdir(tmp_path) == []
    finally:
        os.chdir(monkeypatch_cwd)


def test_aligner_refusals_name_skip_alignment(tmp_path, monkeypatch, no_gpu):
    from video_3d_pipeline import utils
    from video_3d_pipeline.align import VideoAligner
    rng = np.random.default_rng(0)
    good = _clip(tmp_path / "good.npz", rng.integers(-999, 999, 5000).astype(np.int16))
    cases = {
        "missing": (str(tmp_path / "missing.npz"), good),
        "no audio": (_clip(tmp_path / "mute.npz"), good),
        "silent": (good, _clip(tmp_path / "silent.npz", np.full(5000, 17, np.int16))),
        "zeros": (_clip(tmp_path / "zeros.npz", np.zeros(5000, np.float32)), good),
        "rates": (good, _clip(tmp_path / "r44.npz", rng.integers(-999, 999, 5000).astype(np.int16), rate=44100)),
    }
    (tmp_path / "film.mkv").write_bytes(b"\0" * 64)
    for what, (v1, v2) in cases.items():
        wd = tmp_path / f"wd_{what.replace(' ', '_')}"
        with pytest.raises(RuntimeError, match="skip-alignment"):
            VideoAligner(v1, v2, str(wd)).find_alignment(300)
        assert not wd.exists(), what
    monkeypatch.setattr(utils.shutil, "which", lambda name: None)          # no decoder
    with pytest.raises(RuntimeError, match="skip-alignment"):
        VideoAligner(str(tmp_path / "film.mkv"), good, str(tmp_path / "wd_dec")).find_alignment(300)
    with pytest.raises(RuntimeError, match="skip-alignment"):
        VideoAligner("a", "b").find_alignment(300)


# ---------------------------------------------------------------- quality grades

def test_quality_grades_at_each_threshold():
    from video_3d_pipeline.align import VideoAligner, assess_alignment_quality
    fd = 1 / 25.0

    def grade(off, corr, tol=2.0):
        d = {"time_offset_seconds": off, "correlation_strength": corr, "frame_duration": fd}
        g = assess_alignment_quality(d, tol)
        assert VideoAligner("a", "b").assess_alignment_quality(d, tol) == g
        return g
    assert grade(0.0, 0.0) == "EXCELLENT"
    assert grade(-0.0799, 0.1) == "EXCELLENT"              # |offset| < 2 frames
    assert grade(2 * fd, 0.99) == "GOOD"                   # == the limit is not within it
    assert grade(0.5, 0.8000001) == "GOOD"
    assert grade(0.5, 0.8) == "MODERATE"
    assert grade(-3.0, 0.6000001) == "MODERATE"
    assert grade(-3.0, 0.6) == "POOR"
    assert grade(0.5, 0.0) == "POOR"
    assert grade(0.1, 0.0, tol=3.0) == "EXCELLENT"


def test_alignment_file_helpers(tmp_path):
    from video_3d_pipeline.align import apply_offset_to_pipeline, load_alignment_data
    f = tmp_path / "alignment_data.json"
    f.write_text(json.dumps({"video1_path": "s.npz", "video2_path": "k.npz", "time_offset_seconds": -0.5}))
    assert load_alignment_data(str(f))["time_offset_seconds"] == -0.5
    assert apply_offset_to_pipeline(str(f), "s.npz", "o", 2.0) == 2.0
    assert apply_offset_to_pipeline(str(f), "k.npz", "o", 2.0) == 1.5
    assert apply_offset_to_pipeline(str(f), "k.npz", "o", 0.25) == 0          # clamped, as in the reference
    with pytest.raises(ValueError):
        apply_offset_to_pipeline(str(f), "other", "o")
    with pytest.raises(FileNotFoundError):
        load_alignment_data(str(tmp_path / "none.json"))


# ---------------------------------------------------------------- align CLI

def _fake_find(corr, calls):
    def find_alignment(self, max_audio_length=300):
        calls.append(max_audio_length)
        return {"time_offset_seconds": 1.0, "correlation_strength": corr, "frame_duration": 0.04}
    return find_alignment


def test_align_main_asks_below_min_correlation(monkeypatch, tmp_path):
    from video_3d_pipeline import align
    calls = []
    monkeypatch.setattr(align.VideoAligner, "find_alignment", _fake_find(0.3, calls))

    def eof(prompt=""):
        raise EOFError
    monkeypatch.setattr("builtins.input", eof)
    assert align.main(["a", "b", "--work-dir", str(tmp_path), "--max-audio", "12"]) == 1      # EOF = "no"
    monkeypatch.setattr("builtins.input", lambda prompt="": "y")
    assert align.main(["a", "b", "--work-dir", str(tmp_path)]) == 0
    monkeypatch.setattr("builtins.input", lambda prompt="": "n")
    assert align.main(["a", "b", "--work-dir", str(tmp_path)]) == 1
    assert align.main(["a", "b", "--min-correlation", "0.2"]) == 0                              # above: no question
    assert calls == [12.0, 300.0, 300.0, 300.0]
    monkeypatch.undo()
    assert align.main([str(tmp_path / "missing_a.npz"), "b", "--work-dir", str(tmp_path / "y")]) == 1


# ---------------------------------------------------------------- --alignment-file on the CLIs

@pytest.fixture
def k4(tmp_path):
    np.savez(tmp_path / "k4.npz", frames=_frames(3), fps=25.0)
    return str(tmp_path / "k4.npz")


def _align_json(tmp_path, offset, fps1=24.0):
    f = tmp_path / f"al_{offset}.json"
    f.write_text(json.dumps({"video1_path": "s", "video2_path": "k", "time_offset_seconds": offset, "video1_fps": fps1}))
    return str(f)


def _stub_pipeline(monkeypatch):
    from video_3d_pipeline import pipeline
    seen = {}

    class Stub:
        def __init__(self, **kw):
            pass

        def run(self, video, video_4k, **kw):
            seen.update(kw)
            return "out.json"
    monkeypatch.setattr(pipeline, "SbsTo4kDepthPipeline", Stub)
    return pipeline, seen


def _stub_upscale(monkeypatch):
    from video_3d_pipeline import upscale
    seen = {}

    class Stub:
        def __init__(self, **kw):
            pass

        def process_depth_upscaling(self, **kw):
            seen.update(kw)
            return "out.json"
    monkeypatch.setattr(upscale, "SimpleDepthUpscaler", Stub)
    return upscale, seen


@pytest.mark.parametrize("which", ["pipeline", "upscale"])
def test_alignment_file_sets_guide_start_frame(tmp_path, monkeypatch, k4, which, capsys):
    mod, seen = (_stub_pipeline if which == "pipeline" else _stub_upscale)(monkeypatch)
    first = ["sbs.npy"] if which == "pipeline" else [str(tmp_path)]
    for offset, want in ((1.23, 31), (0.0, 0), (0.02, 0), (0.021, 1), (4.0, 100)):     # round(offset * 25 fps of the 4K clip)
        seen.clear()
        assert mod.main(first + [k4, "--alignment-file", _align_json(tmp_path, offset)]) == 0
        assert seen["guide_start_frame"] == want, offset
    seen.clear()
    assert mod.main(first + [k4]) == 0 and seen["guide_start_frame"] == 0               # without the flag: unchanged
    assert mod.main(first + [k4, "--guide-start-frame", "7"]) == 0 and seen["guide_start_frame"] == 7
    with pytest.raises(SystemExit) as e:                                                   # both: argparse error
        mod.main(first + [k4, "--guide-start-frame", "3", "--alignment-file", _align_json(tmp_path, 1.0)])
    assert e.value.code == 2
    seen.clear()
    capsys.readouterr()
    assert mod.main(first + [k4, "--alignment-file", _align_json(tmp_path, -0.5, fps1=24.0)]) == 1    # not clamped
    assert not seen
    assert re.search(r"--start-frame 12\b", capsys.readouterr().out)                      # round(0.5 s * 24 fps on the SBS side)
    assert mod.main(first + [k4, "--alignment-file", str(tmp_path / "absent.json")]) == 1


# ---------------------------------------------------------------- ABI

def test_align_symbols_are_exported():
    from video_3d_pipeline import _native
    header = open(os.path.join(ROOT, "include", "v3d_hip.h")).read()
    lib = ctypes.CDLL(_native.lib_path())
    for s in ("v3d_xcorr_ws_bytes", "v3d_xcorr", "v3d_align_audio"):
        assert s in _native.EXPORTS and re.search(rf"\b{s}\(", header) and hasattr(lib, s), s
    L = _native.lib()
    assert L.v3d_xcorr_ws_bytes(1, 2 ** 26) > 8 * 2 ** 26                 # N = 2^26, the largest size
    assert L.v3d_xcorr_ws_bytes(2, 2 ** 26) == 0                          # N = 2^27: unsupported
    assert L.v3d_xcorr_ws_bytes(0, 5) == 0 and L.v3d_xcorr_ws_bytes(5, -1) == 0
    assert 8 * 1024 <= L.v3d_xcorr_ws_bytes(1, 1) < 8 * 2048 + 2 ** 20     # N never below 2^10
    assert L.v3d_xcorr(None, 1, None, 1, None, None, None) == -1          # null pointers refused before any launch
    assert L.v3d_align_audio(None, 3, None, 3, None, None, None) == -1
    assert b"null" in L.v3d_last_error()
