"""What every device backend of the CLIs shares: the constructor, reusable staging buffers, the gather-and-upload of host
frames, the two ways a result comes back to the host, and the device PNG encoder.  HipStereoBackend (depth.py, and through
it HipPipelineBackend), HipUpscaleBackend (upscale.py) and HipRenderBackend (convert.py) derive from HipBackend and add
their own device steps."""
import numpy as np


def require_hip_device(device):
    """what a driver checks before it builds its own backend (a given stand-in is never asked): there is no CPU path"""
    if not str(device).startswith("cuda"):
        raise RuntimeError(f"device {device!r} requested, but this build only has the MI355X (HIP) path")


class HipBackend:
    """PyTorch-ROCm buffers on one device + libv3d_hip.so.  Every method also works on a subclass whose __init__ set only
    torch / native / device (the host tests' stand-ins): nothing else is assumed to exist."""

    def __init__(self, device: str = "cuda"):
        import torch
        from . import _native
        if not torch.cuda.is_available():
            raise RuntimeError("CUDA not available but requested")
        self.torch = torch
        self.native = _native
        _native.lib()                                  # fail now, loudly, if the HIP library is missing
        # resolved ONCE: a bare "cuda" is the current device (what torch.cuda.set_device / LOCAL_RANK selected), and
        # tensors, the matcher's workspace and its kernels all live on that same index
        self.device = _native.resolve_device(device)
        self._bufs = {}

    # ---- the three places that touch pinned memory, a stream or an event (a CPU stand-in overrides these) ----
    def _pinned(self, shape, dtype):
        """a pinned host block from torch's caching host allocator, which takes it back when the last reference goes"""
        return self.torch.empty(shape, dtype=dtype, pin_memory=True)

    def _synchronize(self):
        """wait for the current stream of THIS backend's device, whatever device is current"""
        self.torch.cuda.current_stream(self.device).synchronize()

    def _event(self):
        """an event recorded on the current stream of this backend's device"""
        ev = self.torch.cuda.Event()
        ev.record(self.torch.cuda.current_stream(self.device))
        return ev

    # ---- buffers ----
    def _staging(self, key, shape, dtype, pinned):
        """reusable buffers: pinned host staging + device tensors (no allocation on the steady-state path)"""
        bufs = self.__dict__.setdefault("_bufs", {})
        t = bufs.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._pinned(shape, dtype) if pinned else self.torch.empty(shape, dtype=dtype, device=self.device)
            bufs[key] = t
        return t

    def _upload(self, name, frames, shape, dtype, capacity=None):
        """host frames of `shape` (None = leave the slot as it is) -> the device view [n, *shape]: gathered in the pinned
        staging `<name>_host` of `capacity` frames (default n), ONE asynchronous copy into `<name>_dev`.  Both are reused by
        the next call, so the caller synchronises before it comes back here."""
        n = len(frames)
        full = (max(n, capacity or n),) + tuple(shape)
        host = self._staging(name + "_host", full, dtype, True)
        dev = self._staging(name + "_dev", full, dtype, False)
        view = host.numpy()
        for i, f in enumerate(frames):
            if f is not None:
                view[i] = f
        dev[:n].copy_(host[:n], non_blocking=True)
        return dev[:n]

    # ---- results back to the host ----
    def _fetch(self, t) -> np.ndarray:
        """device tensor -> NumPy through pinned memory, blocking.  The pinned block is a fresh one from torch's caching host
        allocator and goes back to it once the caller (a writer thread, say) drops the array: no allocation in the steady
        state, and no buffer is overwritten while somebody still reads it."""
        host = self._pinned(tuple(t.shape), t.dtype)
        host.copy_(t, non_blocking=True)
        self._synchronize()
        return host.numpy()

    def _fetch_async(self, tensors):
        """small device tensors -> a handle for _read: each goes to pinned memory without blocking, an event marks the end of
        the copies"""
        host = []
        for t in tensors:
            h = self._pinned(tuple(t.shape), t.dtype)
            h.copy_(t, non_blocking=True)
            host.append(h)
        return host, self._event()

    @staticmethod
    def _read(handle, wait: bool = True):
        """-> the NumPy copies of a _fetch_async handle, or None when the copies have not finished and wait is False.  After
        the stream's next synchronise the event has fired and nothing waits here"""
        host, ev = handle
        if not ev.query():
            if not wait:
                return None
            ev.synchronize()
        return [h.numpy().copy() for h in host]

    # ---- --png-encoder gpu ----
    def _png_encoder(self):
        if getattr(self, "_png", None) is None:
            from .png_gpu import DevicePngEncoder
            self._png = DevicePngEncoder(self.torch, self.native, self.device)
        return self._png
