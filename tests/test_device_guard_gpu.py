"""Every wrapper launches on the device of its tensors (_native._call), not on whatever device is current: inputs on cuda:1 with
device 0 current give what the same call gives with device 1 current, and the result lives on cuda:1.  These five are wrappers
that carried no device guard of their own and sit on the hot path of the depth CLI, the pipeline and bench.py.  Needs two GPUs;
skips on a one-GPU box like the other two-GPU tests."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_wrappers_launch_on_their_tensors_device(native):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    N = native
    rng = np.random.default_rng(11)
    d1 = torch.device("cuda", 1)
    bgr = N.to_device(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), d1)
    disp = N.to_device(rng.integers(-16, 1024, 64).astype(np.int16), d1)
    img = N.to_device(rng.integers(-16, 1024, (8, 16)).astype(np.int16), d1)
    depth = N.to_device((rng.random((2, 4, 8)) * 64).astype(np.float32), d1)
    lo = N.to_device((rng.random((1, 8, 8)) * 64).astype(np.float32), d1)
    guide = N.to_device(rng.integers(0, 256, (1, 16, 16), dtype=np.uint8), d1)
    calls = {"bgr_to_gray": lambda: N.bgr_to_gray(bgr), "disp_to_depth": lambda: N.disp_to_depth(disp),
             "median3x3": lambda: N.median3x3(img), "depth_to_u16_batch": lambda: N.depth_to_u16_batch(depth),
             "guided_upscale_batch": lambda: N.guided_upscale_batch(lo, guide, 2, 1e-3)}
    cur = torch.cuda.current_device()
    try:
        torch.cuda.set_device(1)
        want = {k: f() for k, f in calls.items()}
        torch.cuda.synchronize(1)
        torch.cuda.set_device(0)
        got = {k: f() for k, f in calls.items()}
        torch.cuda.synchronize(1)
    finally:
        torch.cuda.set_device(cur)
    for k in calls:
        assert got[k].device == d1 and want[k].device == d1, k
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=got[k].is_floating_point()), k
