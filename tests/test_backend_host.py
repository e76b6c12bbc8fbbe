"""backend.HipBackend on CPU: what the device backends share, through test_fill_host's stand-in (CPU torch, a logging fake
`native`, no pinned memory).  The three SBS surfaces of HipStereoBackend go through one front end -- one gather, one upload, one
gray split into the staging buffers the later stages read -- and the fetch helpers hand back what was on the "device"."""
import numpy as np
import pytest
import torch

from test_fill_host import _FakeNative, _hip_backend


class _Native(_FakeNative):
    def frame_signature_batch(self, gray):
        self.log.append("signatures")
        return gray

    def plane_profiles_batch(self, gray):
        self.log.append("profiles")
        return gray, gray


class _Event:
    """stands for torch.cuda.Event: fires when told to, and counts who waited for it"""

    def __init__(self, fired):
        self.fired, self.waits = fired, 0

    def query(self):
        return self.fired

    def synchronize(self):
        self.waits += 1
        self.fired = True


def _backend(native=None, fired=True):
    be = _hip_backend(native or _Native())
    be.events, be.syncs = [], 0

    def event():
        be.events.append(_Event(fired))
        return be.events[-1]

    def synchronize():
        be.syncs += 1

    be._pinned = lambda shape, dtype: torch.empty(shape, dtype=dtype)          # no pinned memory on a CPU-only box
    be._event, be._synchronize = event, synchronize
    return be


@pytest.mark.parametrize("surface, then", [("sbs_to_disparity", ["compute", "depth"]), ("sbs_left_signatures", ["signatures"]),
                                           ("sbs_left_profiles", ["profiles"])])
@pytest.mark.parametrize("unsqueeze", [True, False])
def test_sbs_surfaces_share_one_front_end(surface, then, unsqueeze):
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (4, 16, 3), dtype=np.uint8) for _ in range(2)]
    nat = _Native()
    be = _backend(nat)
    getattr(be, surface)(frames, unsqueeze)
    assert nat.log == ["gray"] + then                                          # exactly one gray split, and first
    ow = 16 if unsqueeze else 8
    assert tuple(be._bufs["lg"].shape) == tuple(be._bufs["rg"].shape) == (2, 4, ow)
    assert be.left_gray(2).data_ptr() == be._bufs["lg"].data_ptr() and be.right_gray(2).data_ptr() == be._bufs["rg"].data_ptr()
    assert np.array_equal(be._bufs["sbs_dev"].numpy(), np.stack(frames))      # the gathered frames are what was uploaded
    before = dict(be._bufs)
    getattr(be, surface)(frames, unsqueeze)
    assert nat.log == (["gray"] + then) * 2
    assert be._bufs.keys() == before.keys() and all(be._bufs[k] is before[k] for k in before), "a second pass allocated"


def test_upload_keeps_capacity_and_skips_missing_frames():
    be = _backend()
    a, b = np.full((2, 3), 7, np.uint8), np.full((2, 3), 9, np.uint8)
    dev = be._upload("x", [a, b], (2, 3), torch.uint8, capacity=4)
    assert tuple(dev.shape) == (2, 2, 3) and tuple(be._bufs["x_dev"].shape) == tuple(be._bufs["x_host"].shape) == (4, 2, 3)
    assert np.array_equal(dev.numpy(), np.stack([a, b]))
    again = be._upload("x", [None, a], (2, 3), torch.uint8, capacity=4)      # None: the slot keeps what it held
    assert again.data_ptr() == dev.data_ptr() and np.array_equal(again.numpy(), np.stack([a, a]))


def test_blocking_fetch_returns_a_block_of_its_own():
    be = _backend()
    t = be._staging("src", (3, 5), torch.int16, False)
    t.copy_(torch.arange(15, dtype=torch.int16).reshape(3, 5))
    got = be._fetch(t)
    assert got.dtype == np.int16 and np.array_equal(got, t.numpy()) and be.syncs == 1
    assert not any(np.shares_memory(got, b.numpy()) for b in be._bufs.values())
    assert not np.shares_memory(got, be._fetch(t))                             # nor the block of the next fetch
    u16 = be.to_host_u16(t)
    assert u16.dtype == np.uint16 and np.array_equal(u16, t.numpy().view(np.uint16))
    assert np.array_equal(be.depth_to_host(t.to(torch.float32)), t.numpy().astype(np.float32))


def test_non_blocking_fetch_and_its_reader():
    rec = torch.arange(8, dtype=torch.int64).reshape(2, 4)
    trio = (rec, rec[0] * 3, rec[:, 0] + 5)
    # the event has fired: nobody waits, with or without the flag
    be = _backend(fired=True)
    handle = be.quality_fetch(rec)
    assert np.array_equal(be.read_quality(handle, wait=False), rec.numpy()) and np.array_equal(be.read_quality(handle), rec.numpy())
    assert be.events[0].waits == 0
    # not yet: wait=False returns None and does not block; wait=True blocks once and returns the records
    be = _backend(fired=False)
    handle = be.quality_fetch(rec)
    assert be.read_quality(handle, wait=False) is None and be.events[0].waits == 0
    got = be.read_quality(handle)
    assert isinstance(got, np.ndarray) and np.array_equal(got, rec.numpy()) and be.events[0].waits == 1
    assert np.array_equal(be.read_quality(handle, wait=False), rec.numpy())
    # the scores: a tuple of three arrays, copies of the host blocks
    be.native.signature_scores = lambda a, b: trio
    handle = be.signature_scores(None, None)
    got = be.read_scores(handle)
    assert isinstance(got, tuple) and len(got) == 3 and be.events[1].waits == 1
    for g, want, block in zip(got, trio, handle[0]):
        assert g.dtype == np.int64 and np.array_equal(g, want.numpy()) and not np.shares_memory(g, block.numpy())
    assert be.syncs == 0                                                       # neither path synchronises the stream
