"""bench.py itself under test on the one-GPU box: the multi-rank launch line the driver uses (torch.distributed.run, one
process per rank) with two ranks sharing GPU 0 and gloo as the transport, every guide-exchange mode; the lock-step recovery
path driven over several steps; and, when the box has two GPUs, the same over RCCL."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(cmd, timeout=420):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, f"rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}\n{r.stdout[-2000:]}"
    return json.loads(lines[0])


def _torchrun(n, port, extra):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), "bench.py", "--gpus", str(n)] + extra


COMMON = ["--batch", "4", "--steps", "2", "--warmup", "1", "--workload", "full", "--no-cpu-baseline", "--no-e2e"]


@pytest.fixture(scope="module")
def single_rank_frame0(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bench1") / "f0.npz")
    res = _run([sys.executable, "bench.py", "--gpus", "1", "--dump-frame0", out] + COMMON)
    assert res["n_gpus"] == 1 and res["lockstep_timeouts"] == 0
    return np.load(out)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("exchange", ["broadcast", "scatter", "auto"])
def test_bench_two_ranks_share_gpu0_over_gloo(tmp_path, single_rank_frame0, exchange):
    """exactly the driver's multi-GPU command (minus the backend): one JSON line from rank 0, n_gpus = 2, no lock-step
    time-outs, the one-round exchange probe present, and rank 0's frame 0 bit-identical to the single-rank run"""
    out = str(tmp_path / "f0.npz")
    port = 29700 + (os.getpid() % 200) + {"broadcast": 0, "scatter": 1, "auto": 2}[exchange]
    res = _run(_torchrun(2, port, ["--dist-backend", "gloo", "--guide-exchange", exchange, "--dump-frame0", out] + COMMON))
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["scaling"] == "weak"
    assert res["lockstep_timeouts"] == 0 and res["lockstep_recomputed"] is False
    assert res["value"] > 0 and res["config"]["frames_per_step_per_gpu"] == 4
    assert res["config"]["guide_exchange"] in (("broadcast", "scatter") if exchange == "auto" else (exchange,))
    probe = res["config"]["guide_exchange_probe"]
    assert probe["broadcast_one_round_ms"] > 0 and probe["scatter_one_round_ms"] > 0
    got = np.load(out)
    assert np.array_equal(got["disp"], single_rank_frame0["disp"])
    assert np.array_equal(got["q"], single_rank_frame0["q"])


@pytest.mark.timeout(600)
def test_bench_recovers_from_lockstep_timeouts_over_several_steps(tmp_path, single_rank_frame0):
    """every lock-step workgroup of the first timed region reports a time-out (vdd_spin_limit = -1): the first step poisons
    its output and raises the host flag, the following steps are refused (V3D_ERR_LOCKSTEP) -- bench.py must neither
    traceback nor report that region: it switches the handle to per-direction launches, times again, says so, and the
    recomputed output has the bits of the healthy run"""
    out = str(tmp_path / "f0.npz")
    res = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--test-inject-lockstep-timeout", "--dump-frame0", out]
               + [a for a in COMMON if a not in ("--steps", "2")] + ["--no-cli"])
    assert res["lockstep_timeouts"] > 0 and res["lockstep_recomputed"] is True
    assert res["lockstep_timeouts_after_switch"] == 0 and res["value"] > 0
    got = np.load(out)
    assert np.array_equal(got["disp"], single_rank_frame0["disp"]) and np.array_equal(got["q"], single_rank_frame0["q"])


@pytest.mark.timeout(600)
def test_bench_dump_outputs_are_the_timed_output_and_repeat(tmp_path, single_rank_frame0):
    """--dump-outputs: float32 / float64 files, under 64 MB in all; frame 0 of the 4K depth has the bits --dump-frame0 saw,
    the sampled rows of frame 0 are its rows, and a second run with the same arguments writes the same arrays"""
    dirs = [tmp_path / "o0", tmp_path / "o1"]
    for d in dirs:
        res = _run([sys.executable, "bench.py", "--gpus", "1", "--dump-outputs", str(d)] + COMMON)
        assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["lockstep_timeouts"] == 0
    names = sorted(os.listdir(dirs[0]))
    assert names == ["depth4k_frame0.npy", "depth4k_rows.npy", "depth4k_rows_index.npy"]
    assert sum((dirs[0] / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        a = np.load(dirs[0] / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, np.load(dirs[1] / n)), n
    f0 = np.load(dirs[0] / "depth4k_frame0.npy")
    assert np.array_equal(f0, single_rank_frame0["q"])
    rows, idx = np.load(dirs[0] / "depth4k_rows.npy"), np.load(dirs[0] / "depth4k_rows_index.npy").astype(np.int64)
    own = idx[:, 0] == 0
    assert own.any() and np.array_equal(rows[own], f0[idx[own, 1]])


@pytest.mark.timeout(900)
def test_bench_two_ranks_over_rccl(tmp_path, single_rank_frame0):
    """the driver's command as it is (backend nccl = RCCL, one GPU per rank); skips on a one-GPU box"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    out = str(tmp_path / "f0.npz")
    res = _run(_torchrun(2, 29950 + (os.getpid() % 40), ["--dump-frame0", out] + COMMON))
    assert res["n_gpus"] == 2 and res["lockstep_timeouts"] == 0
    assert res["config"]["guide_exchange"] == "scatter"
    got = np.load(out)
    assert np.array_equal(got["disp"], single_rank_frame0["disp"]) and np.array_equal(got["q"], single_rank_frame0["q"])


@pytest.mark.timeout(900)
def test_bench_default_batch_dump_meets_the_oracle_on_every_frame(tmp_path, oracle):
    """bench.py at its DEFAULT batch (one full lock-step launch, B frames; its own parity_check looks at frame 0 only): frame 0
    of the 4K depth and every row of the dumped sample -- which reaches every frame index 0 .. B-1 -- within 1e-3 of the float64
    oracle of the base frame that position carries (frame f holds synthetic frame f % N_DISTINCT, as bench builds it)"""
    from concurrent.futures import ThreadPoolExecutor
    import bench
    from test_guided_gpu import RTOL, _rel_err
    from video_3d_pipeline import _native as N, synthetic as syn
    probe = N.StereoSGBM(bench.W, bench.H, 1)
    B = probe.get_option("vdd_frames_per_launch_dpl8")
    probe.close()
    assert B >= 2, f"bench batch B = {B}"
    d = tmp_path / "out"
    res = _run([sys.executable, "bench.py", "--gpus", "1", "--workload", "full", "--steps", "1", "--warmup", "1",
                "--no-cpu-baseline", "--no-e2e", "--dump-outputs", str(d)], timeout=600)
    assert res["config"]["frames_per_step_per_gpu"] == B and res["lockstep_timeouts"] == 0, (B, res["config"])
    nd = min(B, bench.N_DISTINCT)

    def want(i):
        sbs, guide = syn.sbs_frame(bench.W, bench.H, i), syn.guide_frame(bench.W, bench.H, i, bench.SCALE)
        disp = oracle.sgbm_compute(*oracle.sbs_to_gray(sbs, True))
        return oracle.guided_upscale(oracle.disp_to_depth(disp), guide, bench.GF_R, bench.GF_EPS)
    with ThreadPoolExecutor(max(1, min(nd, 16, len(os.sched_getaffinity(0))))) as ex:
        q = list(ex.map(want, range(nd)))
    f0 = np.load(d / "depth4k_frame0.npy").astype(np.float64)
    err = _rel_err(f0, q[0])
    assert err.max() <= RTOL, f"B = {B}, frame 0: max rel err {err.max():.3e}"
    rows, idx = np.load(d / "depth4k_rows.npy"), np.load(d / "depth4k_rows_index.npy").astype(np.int64)
    assert rows.shape == (len(idx), bench.W * bench.SCALE)
    assert set(idx[:, 0].tolist()) == set(range(B)), f"B = {B}: the sample misses frames {sorted(set(range(B)) - set(idx[:, 0].tolist()))}"
    floor = [1e-6 * max(float(np.abs(w).max()), 1e-30) for w in q]        # _rel_err's floor, of the whole frame
    for (f, y), row in zip(idx, rows):
        w = q[f % nd][y]
        err = np.abs(row.astype(np.float64) - w) / np.maximum(np.abs(w), floor[f % nd])
        assert err.max() <= RTOL, f"B = {B}, frame {f} (base {f % nd}) row {y}: max rel err {err.max():.3e}"
