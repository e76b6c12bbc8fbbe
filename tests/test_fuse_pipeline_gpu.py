"""--fuse-source through the real HIP backends, on the clips of tests/test_source_parallax_pipeline_gpu.py (480 x 270 eyes stored
side by side, a 960 x 540 "4K" release): the depth, upscale and convert CLIs with and without the flag.  The fused right eye is the
NumPy chain (tests/stereo_source_ref.py -> tests/verify_ref.py -> tests/fuse_ref.py) byte for byte, alone, after --verify-source,
after --match-colour clip and on the top-bottom layout; the manifest names it; --fidelity-report's `final` series measures the
fused eye; and without the flag the convert CLI writes the bytes it wrote before."""
import json
import os

import numpy as np
import pytest

import colour_ref as CR
import fidelity_ref as FR
import fuse_ref as F
import stereo_source_ref as X
import verify_ref as V
from test_source_parallax_pipeline_gpu import EH, EW, FLAGS, NF, _three_clis, clips  # noqa: F401

pytestmark = pytest.mark.gpu

Q = (32768, -16384, 32768, -16384)                             # a 480 x 270 eye under a 960 x 540 frame
W, H = 2 * EW, 2 * EH
RUNS = {"f": ("--fuse-source",), "vf": ("--verify-source", "--fuse-source"), "tb": ("--fuse-source", "--verify-source", "--layout", "full-tb"),
        "tb_plain": ("--layout", "full-tb"), "cm": ("--match-colour", "clip", "--match-probes", "2", "--fuse-source"),
        "vfr": ("--verify-source", "--fuse-source", "--fidelity-report"), "png": ("--fuse-source", "--png-encoder", "gpu")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory, clips):
    """one depth and upscale run, then the convert CLI on it: without the flag and with it in every combination above"""
    from video_3d_pipeline import convert
    from video_3d_pipeline.utils import iter_frames, read_png16
    tmp = tmp_path_factory.mktemp("fuse")
    sbs, v4k, truth = clips
    base = ("--parallax", "source", "--fill-from-source", sbs)
    _, up, plain = _three_clis(tmp, "plain", sbs, v4k, FLAGS, base)
    upj = str(tmp / "up_plain.json")
    mans = {"plain": plain}
    for tag, extra in RUNS.items():
        assert convert.main([v4k, upj, "--output", str(tmp / f"3d_{tag}.json"), *base, *extra]) == 0
        mans[tag] = json.loads(open(tmp / f"3d_{tag}.json").read())
    depth = [read_png16(os.path.join(up["frames_dir"], f"depth4k_{i:06d}.png")) for i in range(NF)]
    return mans, {k: list(iter_frames(m["frames_dir"])) for k, m in mans.items()}, list(iter_frames(sbs)), list(iter_frames(v4k)), depth, truth


def test_the_fused_eye_is_the_numpy_chain(native, runs):
    mans, frames, sbs, v4k, depth, _ = runs
    man = mans["plain"]
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    for tag, plain, tau, eye in (("f", "plain", None, lambda f: f[:, W:]), ("vf", "plain", 48, lambda f: f[:, W:]),
                                 ("tb", "tb_plain", 48, lambda f: f[H:])):
        for i in range(NF):
            E = np.ascontiguousarray(eye(frames[plain][i]))
            if tau is not None:
                E = V.verify(E, sbs[i], 1, *Q, tau)[0]
            want = frames[plain][i].copy()
            eye(want)[...] = F.fuse(E, sbs[i], 1, *Q)
            assert (eye(want) != E).any()
            assert np.array_equal(frames[tag][i], want), (tag, i)          # the fused right eye, and the left eye as it was
        assert mans[tag]["fuse_source"] == {"samples_per_pixel": [0.5, 0.5]}
        assert ("verify_source" in mans[tag]) == (tau is not None) and "fuse_source" not in mans[plain]
    assert sorted(mans["f"]) == sorted(list(man) + ["fuse_source"])
    # --match-colour clip: the render and the fusion read the stored right eye through the clip's table
    lut = np.array(json.loads(open(mans["cm"]["colour_lut"]).read())["lut"], np.uint8)
    graded = CR.apply(np.stack(sbs), lut, (EW, 0, 2 * EW, EH))
    for i in range(NF):
        want = X.render(v4k[i], depth[i], *gains, 0, False, graded[i], 2, *Q)
        want[:, W:] = F.fuse(np.ascontiguousarray(want[:, W:]), graded[i], 1, *Q)
        assert np.array_equal(frames["cm"][i], want), i
    # the device PNG encoder takes the fused frames
    assert all(np.array_equal(a, b) for a, b in zip(frames["png"], frames["f"])) and mans["png"]["fuse_source"] == mans["f"]["fuse_source"]


def test_without_the_flag_the_bytes_are_the_contracts(native, runs):
    """the runs without it: the source render of the 4K frame and the 4K depth, byte for byte (the parent's path)"""
    mans, frames, sbs, v4k, depth, _ = runs
    man = mans["plain"]
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    for i in range(NF):
        assert np.array_equal(frames["plain"][i], X.render(v4k[i], depth[i], *gains, 0, False, sbs[i], 2, *Q)), i
        assert np.array_equal(frames["tb_plain"][i], X.render(v4k[i], depth[i], *gains, 2, False, sbs[i], 2, *Q)), i
    assert "fuse_source" not in man and "fuse_source" not in mans["tb_plain"]


def test_the_final_series_measures_the_fused_eye(native, runs):
    from video_3d_pipeline.fidelity import FIELDS
    mans, frames, sbs, _, _, _ = runs
    assert all(np.array_equal(a, b) for a, b in zip(frames["vfr"], frames["vf"]))            # the report changes no byte
    report = json.loads(open(mans["vfr"]["fidelity_report"]["path"]).read())
    for i in range(NF):
        want = FR.fidelity(np.ascontiguousarray(frames["vfr"][i][:, W:]), sbs[i], 1, *Q, 48).tolist()
        assert [report["frames"][i]["final"][k] for k in FIELDS] == want, i
    assert list(mans["vfr"])[-3:] == ["verify_source", "fuse_source", "fidelity_report"]

