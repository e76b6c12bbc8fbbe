"""The DIBR step end to end on the MI355X: the convert CLI's frames against the NumPy contract (tests/stereo_ref.py), and the
one-pass pipeline's --stereo-output against the convert CLI run on that pipeline's own depth output (real HIP backends)."""
import json
import os

import numpy as np
import pytest

import stereo_ref as R

pytestmark = pytest.mark.gpu

SW, SH = 192, 48                      # SBS frame; the "4K" frame is 2SW x 2SH


def _pngs(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("layout", ["full-sbs", "half-sbs"])
def test_convert_cli_equals_the_reference(native, tmp_path, layout):
    from video_3d_pipeline import convert
    from video_3d_pipeline.utils import iter_frames, write_png16
    rng = np.random.default_rng(3)
    W, H = 1000, 72                                                       # rows not a multiple of 16 bytes
    frames = rng.integers(0, 256, (7, H, W, 3), dtype=np.uint8)
    np.save(tmp_path / "v4k.npy", frames)
    ddir = tmp_path / "d_frames"
    ddir.mkdir()
    x = np.arange(W)[None, :]
    depths = []
    for i in range(6):
        d = np.clip(rng.integers(0, 65536) + x * int(rng.integers(-120, 120)) + rng.integers(-900, 900, (H, 1)), 0, 65535)
        d[:, 300:420] = rng.integers(0, 65536)
        if i == 5:
            d = rng.integers(0, 65536, (H, W))                              # noise: dense collisions and cracks
        depths.append(d.astype(np.uint16))
        write_png16(ddir / f"depth4k_{i:06d}.png", depths[-1])
    out = tmp_path / "o.json"
    rc = convert.main([str(tmp_path / "v4k.npy"), str(ddir), "--output", str(out), "--layout", layout, "--max-shift", "90",
                       "--convergence", "0.35", "--eye-split", "0.6", "--guide-start-frame", "1"])
    assert rc == 0
    man = json.loads(out.read_text())
    got = list(iter_frames(man["frames_dir"]))
    gains = R.stereo_gains(90, 0.35, 0.6)
    lay = R.FULL_SBS if layout == "full-sbs" else R.HALF_SBS
    assert len(got) == 6 and man["count"] == 6
    for i in range(6):
        assert np.array_equal(got[i], R.render(frames[1 + i], depths[i], *gains, lay)), i
    conv = convert.DepthTo3DConverter(max_shift=90, convergence=0.35, eye_split=0.6, layout=layout)
    assert np.array_equal(conv.render_frame(frames[1], depths[0]), got[0])


@pytest.mark.timeout(600)
def test_pipeline_stereo_output_equals_the_convert_cli(native, tmp_path):
    from video_3d_pipeline import convert, synthetic as syn
    from video_3d_pipeline.pipeline import SbsTo4kDepthPipeline
    sbs = np.stack([syn.sbs_frame(SW, SH, i) for i in range(5)])
    rng = np.random.default_rng(9)
    v4k = rng.integers(0, 256, (4, 2 * SH, 2 * SW, 3), dtype=np.uint8)     # one frame short: the last one has no stereo frame
    np.save(tmp_path / "sbs.npy", sbs)
    np.save(tmp_path / "v4k.npy", v4k)

    def run(tag, **kw):
        pipe = SbsTo4kDepthPipeline(work_dir=str(tmp_path / f"w_{tag}"), batch_size=4, stereo_only=True, guide_batch=3)
        return json.loads(open(pipe.run(str(tmp_path / "sbs.npy"), str(tmp_path / "v4k.npy"),
                                        output_path=str(tmp_path / f"depth_{tag}.json"), **kw)).read())

    plain = run("plain")
    opts = dict(max_shift=40.0, convergence=0.45, eye_split=0.3, layout="half-sbs")
    man = run("st", stereo_output=str(tmp_path / "st3d.json"), stereo_options=opts)
    assert _pngs(man["frames_dir"]) == _pngs(plain["frames_dir"])            # the depth files do not change
    rc = convert.main([str(tmp_path / "v4k.npy"), str(tmp_path / "depth_st.json"), "--output", str(tmp_path / "cli3d.json"),
                       "--layout", "half-sbs", "--max-shift", "40", "--convergence", "0.45", "--eye-split", "0.3"])
    assert rc == 0
    got, want = json.loads((tmp_path / "st3d.json").read_text()), json.loads((tmp_path / "cli3d.json").read_text())
    assert got["count"] == want["count"] == 4
    assert _pngs(got["frames_dir"]) == _pngs(want["frames_dir"])
