"""Audio alignment on the MI355X: v3d_xcorr against a float64 NumPy correlation at every FFT size, v3d_align_audio against a
float64 find_audio_offset, and the reference's run_pipeline.py step 1 end to end, feeding --alignment-file."""
import json
import os

import numpy as np
import pytest
import torch

from align_ref import RATE, _direct, _norm64, _oracle_align, _ref_corr, _tracks, spectral_error, white
from test_align_edges_gpu import K

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


# ---------------------------------------------------------------- v3d_xcorr

def _xcorr_cases(m):
    N = 1 << m
    need = N - 37 if m > 10 else N - 5                       # n1 + n2 - 1 in (N/2, N]
    n1 = (need * 3 // 5) | 1                                 # odd, unequal
    n2 = need + 1 - n1
    cases = [(n1, n2), (n2, n1), (1, N if m > 10 else 700)]
    if m == 10:
        cases += [(1, 1), (3, 2), (1000, 25)]
    return cases


@pytest.mark.timeout(600)
@pytest.mark.parametrize("m", list(range(10, 25)))
def test_xcorr_every_fft_size(native, m):
    rng = np.random.default_rng(m)
    for n1, n2 in _xcorr_cases(m):
        a1 = (rng.standard_normal(n1) * 3 + 0.5).astype(np.float32)
        a2 = (rng.standard_normal(n2) - 0.25).astype(np.float32)
        got = native.xcorr(_dev(a1), _dev(a2)).cpu().numpy().astype(np.float64)
        want = _ref_corr(a1, a2)
        assert got.shape == (n1 + n2 - 1,)
        tol = 1e-5 * np.linalg.norm(a1.astype(np.float64)) * np.linalg.norm(a2.astype(np.float64))
        err = np.abs(got - want).max()
        assert err <= tol, (m, n1, n2, err, tol)
    # a second, zero-mean white input held per spectrum bin (tests/align_ref.py; the bound above divides a one-bin error by N)
    rng = np.random.default_rng(1000 + m)
    for n1, n2 in _xcorr_cases(m)[:2]:
        a1, a2 = white(n1, rng), white(n2, rng)
        got = native.xcorr(_dev(a1), _dev(a2)).cpu().numpy().astype(np.float64)
        units = spectral_error(got, a1, a2)
        print(f"xcorr 2^{m} ({n1}, {n2}): {units:.3f} units of eps32 log2 N per bin")
        assert units <= K, (m, n1, n2, units, K)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("m", [25, 26])
def test_xcorr_largest_sizes_by_direct_sums(native, m):
    N = 1 << m
    lag = 12345 if m == 25 else -54321
    n1 = (N // 2) - 1001
    n2 = N - n1 - 3 if m == 25 else N + 1 - n1               # 2^26: n1 + n2 - 1 == N exactly
    a1, a2 = _tracks(n1, n2, lag, m)
    got = native.xcorr(_dev(a1), _dev(a2))
    assert got.shape == (n1 + n2 - 1,)
    peak = int(torch.argmax(got.abs()).item()) - (n1 - 1)
    assert peak == lag
    rng = np.random.default_rng(m)
    lags = [lag, lag - 1, lag + 1, 0, -(n1 - 1), n2 - 1, -(n1 - 2), n2 - 2]
    lags += [int(x) for x in rng.integers(-(n1 - 1), n2, 64 - len(lags))]
    tol = 1e-5 * np.linalg.norm(a1.astype(np.float64)) * np.linalg.norm(a2.astype(np.float64))
    host = got.cpu().numpy()
    x1, x2 = a1.astype(np.float64), a2.astype(np.float64)
    vals = {}
    for L in lags:
        vals[L] = _direct(x1, x2, L)
        assert abs(float(host[L + n1 - 1]) - vals[L]) <= tol, (m, L)
    assert max(vals, key=lambda L: abs(vals[L])) == lag


def test_xcorr_refuses_oversize(native):
    with pytest.raises(native.NativeError, match="unsupported"):
        native.xcorr(torch.zeros(2, device="cuda"), torch.zeros(2 ** 26, device="cuda"))


# ---------------------------------------------------------------- v3d_align_audio

@pytest.mark.timeout(600)
@pytest.mark.parametrize("n1,n2,lag", [
    (50000, 50000, 0), (50000, 50000, 1234), (50000, 50000, -1234), (70001, 33333, 20000), (33333, 70001, -15000),
    (5000, 400000, 300000), (RATE * 20, RATE * 20 - 7, 2205 * 3)])
def test_align_audio_lags(native, n1, n2, lag):
    a1, a2 = _tracks(n1, n2, lag, n1 + n2 + abs(lag))
    got = native.align_audio(_dev(a1), _dev(a2)).cpu().numpy()
    L, c, strength, sd = _oracle_align(a1, a2)
    assert L == lag
    assert int(got[0]) == L and got[0] == int(got[0])
    assert abs(got[2] - strength) <= 1e-6, (got[2], strength)
    assert abs(got[1] - c) <= 1e-6 * np.sqrt(n1 * n2), (got[1], c)
    assert abs(got[3] - sd) <= 1e-9 * sd


@pytest.mark.timeout(900)
def test_align_audio_full_300s(native):
    n = 300 * RATE
    lag = -int(2.5 * RATE) + 11
    a1, a2 = _tracks(n, n, lag, 300)
    got = native.align_audio(_dev(a1), _dev(a2)).cpu().numpy()
    L, c, strength, _ = _oracle_align(a1, a2)
    assert L == lag and int(got[0]) == L
    assert abs(got[2] - strength) <= 1e-6


@pytest.mark.timeout(300)
def test_align_audio_near_tie_pure_tone(native):
    n1, n2 = 40000, 46000
    t = np.arange(max(n1, n2)) / RATE
    a1 = np.sin(2 * np.pi * 441.0 * t[:n1]).astype(np.float32)
    a2 = np.sin(2 * np.pi * 441.0 * t[:n2] + 0.3).astype(np.float32)
    got = native.align_audio(_dev(a1), _dev(a2)).cpu().numpy()
    x1, x2 = _norm64(a1), _norm64(a2)
    c = _ref_corr(x1, x2)
    L = int(got[0])
    cl = _direct(x1, x2, L)
    assert abs(cl) >= (1 - 1e-6) * np.abs(c).max()
    E = np.sqrt(np.sum(x1 * x1) * np.sum(x2 * x2))
    assert abs(got[2] - abs(cl) / E) <= 1e-6 and abs(got[2] - np.abs(c).max() / E) <= 1e-6


@pytest.mark.timeout(120)
def test_align_audio_is_deterministic(native):
    a1, a2 = _tracks(123457, 98765, 4321, 7)
    d1, d2 = _dev(a1), _dev(a2)
    first = native.align_audio(d1, d2).cpu().numpy()
    for _ in range(3):
        assert np.array_equal(native.align_audio(d1, d2).cpu().numpy(), first)


# ---------------------------------------------------------------- run_pipeline.py step 1, then --alignment-file

SW, SH = 384, 96
FPS = 24.0


@pytest.mark.timeout(900)
def test_run_pipeline_step1_and_alignment_file(native, tmp_path):
    from video_3d_pipeline import synthetic as syn
    from video_3d_pipeline.align import VideoAligner
    from video_3d_pipeline.pipeline import main as pipeline_main

    lag = 1838                                                  # 0.0834 s: the 4K clip runs 2 frames ahead
    a1, a2 = _tracks(RATE * 12, RATE * 12 + 500, lag, 42)
    st = np.stack([a1, a1 * 0.5 + 0.01], axis=1)               # stereo SBS track, int16
    sbs_audio = np.clip(np.rint(st * 20000), -32768, 32767).astype(np.int16)
    np.savez(tmp_path / "sbs.npz", frames=np.stack([syn.sbs_frame(SW, SH, i) for i in range(5)]), fps=FPS,
             audio=sbs_audio, audio_rate=RATE)
    g = np.stack([np.repeat(syn.guide_frame(SW, SH, i)[..., None], 3, axis=2) for i in range(9)])
    np.savez(tmp_path / "v4k.npz", frames=g, fps=FPS, audio=a2, audio_rate=RATE)
    sbs, v4k, work = str(tmp_path / "sbs.npz"), str(tmp_path / "v4k.npz"), str(tmp_path / "work")

    aligner = VideoAligner(sbs, v4k, work)                      # run_pipeline.py:41-43
    data = aligner.find_alignment(max_audio_length=300)
    quality = aligner.assess_alignment_quality(data)

    m1 = (sbs_audio.astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float32)
    L, _, strength, _ = _oracle_align(m1, a2)
    assert L == lag
    keys = ["video1_path", "video2_path", "time_offset_seconds", "offset_frames", "correlation_strength", "frame_duration",
            "video1_fps", "video2_fps", "sample_rate", "audio_length_analyzed"]
    saved = json.loads(open(os.path.join(work, "alignment_data.json")).read())
    assert list(data) == keys and saved == data
    assert data["video1_path"] == sbs and data["video2_path"] == v4k
    assert data["time_offset_seconds"] == lag / RATE and data["sample_rate"] == RATE
    assert data["frame_duration"] == 1 / FPS and data["offset_frames"] == (lag / RATE) / (1 / FPS)
    assert data["video1_fps"] == FPS and data["video2_fps"] == FPS and data["audio_length_analyzed"] == 300.0
    assert abs(data["correlation_strength"] - strength) <= 1e-6
    assert quality == ("GOOD" if strength > 0.8 else "MODERATE" if strength > 0.6 else "POOR")

    gsf = round(data["time_offset_seconds"] * FPS)
    assert gsf == 2
    outs = {}
    for tag, extra in (("file", ["--alignment-file", os.path.join(work, "alignment_data.json")]),
                       ("frame", ["--guide-start-frame", str(gsf)])):
        out = str(tmp_path / f"{tag}.json")
        assert pipeline_main([sbs, v4k, "--stereo-only", "--work-dir", str(tmp_path / f"w_{tag}"), "--output", out] + extra) == 0
        d = json.loads(open(out).read())["frames_dir"]
        outs[tag] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    assert len(outs["file"]) == 5 and outs["file"] == outs["frame"]
