"""--png-encoder gpu through the real HIP backends on a small synthetic clip: the depth CLI, the one-pass pipeline (with
--keep-depth-maps and --stereo-output), the upscale CLI and the convert CLI write, in both modes, the same file names with
the same decoded pixels and equal manifests; the gpu mode's files are the wrapped streams of tests/png_ref.py."""
import io
import json
import os

import numpy as np
import pytest

import png_ref as P

pytestmark = pytest.mark.gpu

SW, SH, NF = 192, 64, 3


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    from video_3d_pipeline import synthetic as syn
    d = tmp_path_factory.mktemp("pclips")
    np.save(d / "sbs.npy", syn.temporal_sbs_clip(SW, SH, NF, speed=4))
    rng = np.random.default_rng(9)
    np.save(d / "v4k.npy", rng.integers(0, 256, (NF, 2 * SH, 2 * SW, 3), dtype=np.uint8))
    return str(d / "sbs.npy"), str(d / "v4k.npy")


def _decoded(d):
    from PIL import Image
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".png"):
            with Image.open(io.BytesIO(open(os.path.join(d, f), "rb").read())) as im:
                out[f] = np.asarray(im).copy()
    return out


def _same(a, b):
    assert list(a) == list(b) and len(a) > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _manifest(path):
    return {k: v for k, v in json.loads(open(path).read()).items() if k != "frames_dir"}


def _depth_dir(work):
    dirs = [d for d in sorted(os.listdir(work)) if d.startswith("depth_") and os.path.isdir(os.path.join(work, d))]
    assert len(dirs) == 1, dirs
    return os.path.join(work, dirs[0])


def test_depth_and_convert_clis_in_both_modes(native, tmp_path, clips):
    from video_3d_pipeline import convert, depth, upscale
    from video_3d_pipeline.utils import read_png16
    sbs, v4k = clips
    ddir, up, c3d = {}, {}, {}
    for mode in ("zlib", "gpu"):
        work = str(tmp_path / f"d_{mode}")
        assert depth.main([sbs, "--work-dir", work, "--stereo-only", "--png-encoder", mode]) == 0
        ddir[mode] = _depth_dir(work)
        up[mode] = str(tmp_path / f"up_{mode}.json")
        assert upscale.main([ddir[mode], v4k, "--output", up[mode], "--png-encoder", mode]) == 0
        c3d[mode] = str(tmp_path / f"c_{mode}.json")
        assert convert.main([v4k, up[mode], "--output", c3d[mode], "--png-encoder", mode]) == 0
    assert os.path.basename(ddir["zlib"]) == os.path.basename(ddir["gpu"]) and sorted(os.listdir(ddir["zlib"])) == sorted(os.listdir(ddir["gpu"]))
    _same(_decoded(ddir["zlib"]), _decoded(ddir["gpu"]))
    for m in (up, c3d):
        fz, fg = json.loads(open(m["zlib"]).read())["frames_dir"], json.loads(open(m["gpu"]).read())["frames_dir"]
        assert sorted(os.listdir(fz)) == sorted(os.listdir(fg))
        _same(_decoded(fz), _decoded(fg))
        assert _manifest(m["zlib"]) == _manifest(m["gpu"])
    # the gpu mode's file is the reference stream in its chunks
    f = os.path.join(ddir["gpu"], "depth_000000.png")
    img = read_png16(f)
    assert open(f, "rb").read() == P.png(P.stream(img, P.GRAY16), SW, SH, 16, 0)


def test_pipeline_in_both_modes(native, tmp_path, clips):
    from video_3d_pipeline import pipeline
    sbs, v4k = clips
    out = {}
    for mode in ("zlib", "gpu"):
        work, o, s = str(tmp_path / f"p_{mode}"), str(tmp_path / f"p_{mode}.json"), str(tmp_path / f"s_{mode}.json")
        assert pipeline.main([sbs, v4k, "--work-dir", work, "--output", o, "--stereo-only", "--keep-depth-maps", "--stereo-output", s,
                              "--png-encoder", mode]) == 0
        out[mode] = (_depth_dir(work), o, s)
    _same(_decoded(out["zlib"][0]), _decoded(out["gpu"][0]))
    for k in (1, 2):
        _same(_decoded(json.loads(open(out["zlib"][k]).read())["frames_dir"]), _decoded(json.loads(open(out["gpu"][k]).read())["frames_dir"]))
        assert _manifest(out["zlib"][k]) == _manifest(out["gpu"][k])
