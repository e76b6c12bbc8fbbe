"""--verify-source through the real HIP backends, on the clips of tests/test_source_parallax_pipeline_gpu.py (480 x 270 eyes stored
side by side, a 960 x 540 "4K" release): the depth, upscale and convert CLIs with and without the flag.  The verified right eye is
tests/verify_ref.py applied to the unverified run's output, its error against the clip's true right eye falls, and without the
flag the convert CLI writes the bytes it wrote before."""
import json

import numpy as np
import pytest

import stereo_source_ref as X
import verify_ref as V
from test_source_parallax_pipeline_gpu import EH, EW, FLAGS, NF, _pngs, _right_eye_error, _three_clis, clips  # noqa: F401

pytestmark = pytest.mark.gpu

Q = (32768, -16384, 32768, -16384)                             # a 480 x 270 eye under a 960 x 540 frame: cells of 2 x 2


@pytest.fixture(scope="module")
def runs(tmp_path_factory, clips):
    """one depth and upscale run, then the convert CLI on it: without the flag, with it, with it on the top-bottom layout"""
    from video_3d_pipeline import convert
    from video_3d_pipeline.utils import iter_frames
    tmp = tmp_path_factory.mktemp("verify")
    sbs, v4k, truth = clips
    base = ("--parallax", "source", "--fill-from-source", sbs)
    _, up, plain = _three_clis(tmp, "plain", sbs, v4k, FLAGS, base)
    upj = str(tmp / "up_plain.json")
    mans = {"plain": plain}
    for tag, extra in (("v", ("--verify-source",)), ("tb", ("--verify-source", "--layout", "full-tb")), ("tb_plain", ("--layout", "full-tb")),
                       ("v_gpu_png", ("--verify-source", "--png-encoder", "gpu"))):
        assert convert.main([v4k, upj, "--output", str(tmp / f"3d_{tag}.json"), *base, *extra]) == 0
        mans[tag] = json.loads(open(tmp / f"3d_{tag}.json").read())
    return mans, {k: list(iter_frames(m["frames_dir"])) for k, m in mans.items()}, list(iter_frames(sbs)), truth, up


def test_the_verified_eye_is_the_reference_applied_to_the_unverified_output(native, runs):
    mans, frames, sbs, _, _ = runs
    W, H = 2 * EW, 2 * EH
    assert V.cell(Q[0], Q[2]) == (2, 2)
    cells = (W // 2) * (H // 2)
    for plain, ver, eye in (("plain", "v", lambda f: f[:, W:]), ("tb_plain", "tb", lambda f: f[H:])):
        shares = []
        for i in range(NF):
            want, n = V.verify(np.ascontiguousarray(eye(frames[plain][i])), sbs[i], 1, *Q, 48)
            shares.append(n / cells)
            assert np.array_equal(eye(frames[ver][i]), want), (ver, i)
            expect = frames[plain][i].copy()
            eye(expect)[...] = want
            assert np.array_equal(frames[ver][i], expect), "the left eye changed"
        rec = mans[ver]["verify_source"]
        assert rec == {"tau": 48, "cell": [2, 2], "replaced_share": float(np.mean(shares)), "replaced_share_max": max(shares)}
        assert 0 < rec["replaced_share"] < 0.25 and "verify_source" not in mans[plain]
    # the device PNG encoder takes the verified frames: the counters are read after its own copy back
    assert all(np.array_equal(a, b) for a, b in zip(frames["v_gpu_png"], frames["v"]))
    assert mans["v_gpu_png"]["verify_source"] == mans["v"]["verify_source"]


def test_verification_lowers_the_right_eyes_error(native, runs):
    """the right eye against the clip's true right eye (enlarged 2x), mean absolute BGR error over the clip, driven by the matcher's
    own disparity through the guided upscale.  The references alone, with the depth repeated 2x, give a ratio of 0.52 (tests/
    test_verify_host.py); the bound leaves room for the guided-upscaled depth.  Measured on one MI355X: source fill alone 5.30,
    verified at tau 48 1.97 (ratio 0.372), 10.53 % of the 2 x 2 cells replaced."""
    mans, _, _, truth, _ = runs
    e_plain, e_ver = _right_eye_error(mans["plain"], truth), _right_eye_error(mans["v"], truth)
    print(f"right eye vs truth: source fill alone {e_plain:.2f}, verified at tau 48 {e_ver:.2f} (ratio {e_ver / e_plain:.3f}), "
          f"{mans['v']['verify_source']['replaced_share']:.2%} of the cells replaced")
    assert e_ver <= 0.8 * e_plain


def test_without_the_flag_the_bytes_are_the_contracts(native, runs):
    """the unverified runs: the source render of the 4K frame and the 4K depth, byte for byte (the parent's path)"""
    from video_3d_pipeline.utils import iter_frames, read_png16
    import os
    mans, frames, sbs, _, up = runs
    man = mans["plain"]
    gains = (man["gain_left"], man["gain_right"], man["conv"])
    v4k = list(iter_frames(clips_path(man)))
    for i in range(NF):
        d = read_png16(os.path.join(up["frames_dir"], f"depth4k_{i:06d}.png"))
        assert np.array_equal(frames["plain"][i], X.render(v4k[i], d, *gains, 0, False, sbs[i], 2, *Q)), i
        assert np.array_equal(frames["tb_plain"][i], X.render(v4k[i], d, *gains, 2, False, sbs[i], 2, *Q)), i
    assert sorted(mans["v"]) == sorted(list(man) + ["verify_source"])


def clips_path(man):
    """the 4K clip next to the SBS clip a manifest names"""
    import os
    return os.path.join(os.path.dirname(man["fill_from_source"]), "v4k.npy")
