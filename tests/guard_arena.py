"""Guarded buffers for calling the C ABI (include/v3d_hip.h) with every argument under the test's control.

An Arena carves named buffers out of ONE allocation (a uint8 torch tensor on any device, so the checker itself runs on the
CPU).  Every buffer sits between two red zones of at least 4096 bytes and at least one row of that buffer; its payload
starts at 256 * k + skew bytes; rows may be `pitch` elements apart and frames `frame_stride` elements apart, the padding
belonging to the buffer's extent but not to its payload.

    a = Arena("cuda", 0xA5)
    src = a.buf("src", "in", np.uint8, (n, H, W), pitch=W + 3, frame_stride=H * (W + 3) + 7).set(images)
    dst = a.buf("dst", "out", np.int16, (n, H, W), skew=2)
    a.fill(); a.snapshot()
    rc = entry(src.ptr, ..., src.pitch_bytes, src.frame_stride_bytes, dst.ptr, stream)
    synchronise
    a.check()            # GuardError names the buffer, before / inside / after, the first offset and the byte count
    got = dst.get()

fill() writes the poison byte over the whole allocation and then the data of the `in` and `inout` payloads: red zones,
padding, `out` and `ws` payloads hold poison.  check() compares every byte that is not the payload of an `out`, `ws` or
`inout` buffer with the snapshot: red zones, padding (of every role) and `in` payloads.

Blind spot: a stray store of the poison byte itself changes nothing.  Running a case over two poison bytes closes it unless the
stored value follows the poison (a copy kernel that reads its extra element from a red zone and writes it to one).
"""
import numpy as np
import torch

ROLES = ("in", "out", "ws", "inout")
RED_ZONE = 4096
SLOT = 256


class GuardError(AssertionError):
    """damage outside the bytes an entry may write: .name (buffer), .where ('before' / 'inside' / 'after' its extent),
    .offset (first differing byte, relative to the payload's first byte: negative before it), .count (bytes that differ
    in that region)"""

    def __init__(self, name, where, offset, count, detail=""):
        self.name, self.where, self.offset, self.count = name, where, int(offset), int(count)
        super().__init__(f"buffer {name!r}: {count} byte(s) changed {where} the payload, first at offset {int(offset)}{detail}")


class Buf:
    """one buffer of an Arena: logical shape (cols,), (rows, cols) or (frames, rows, cols) of `dtype` elements"""

    def __init__(self, arena, name, role, dtype, shape, align, skew, pitch, frame_stride):
        self.arena, self.name, self.role, self.dtype = arena, name, role, np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        if not 1 <= len(shape) <= 3 or min(shape) < 1:
            raise ValueError(f"{name}: shape {shape} (flatten trailing dimensions into the row)")
        self.shape = shape
        self.frames, self.rows, self.cols = ((1, 1) + shape)[-3:]
        self.pitch = self.cols if pitch is None else int(pitch)                    # elements between rows
        self.frame_stride = self.rows * self.pitch if frame_stride is None else int(frame_stride)   # elements between frames
        if self.pitch < self.cols or (self.frames > 1 and self.frame_stride < (self.rows - 1) * self.pitch + self.cols):
            raise ValueError(f"{name}: pitch {self.pitch} / frame stride {self.frame_stride} overlap the payload")
        self.itemsize = self.dtype.itemsize
        self.align = self.itemsize if align is None else int(align)
        self.skew = int(skew)
        if self.skew % self.align or not 0 <= self.skew < SLOT or SLOT % self.align:
            raise ValueError(f"{name}: skew {skew} does not keep the granted alignment {self.align}")
        # extent in elements: first payload element to the last one
        self.extent = ((self.frames - 1) * self.frame_stride + (self.rows - 1) * self.pitch + self.cols) * self.itemsize
        self.zone = max(RED_ZONE, self.pitch * self.itemsize)
        self.data = None
        self.start = None                                                          # byte offset inside the arena

    # ---- geometry the entry is told ----
    @property
    def ptr(self):
        return self.arena.base_ptr + self.start

    @property
    def pitch_bytes(self):
        return self.pitch * self.itemsize

    @property
    def frame_stride_bytes(self):
        return self.frame_stride * self.itemsize

    @property
    def nbytes(self):
        """payload bytes (without padding)"""
        return self.frames * self.rows * self.cols * self.itemsize

    def set(self, data):
        """host data of an `in` / `inout` payload (any shape with the payload's element count)"""
        if self.role not in ("in", "inout"):
            raise ValueError(f"{self.name}: only in / inout buffers take data")
        a = np.ascontiguousarray(data)
        if a.dtype.itemsize != self.itemsize or a.size != self.frames * self.rows * self.cols:
            raise ValueError(f"{self.name}: data {a.dtype} {a.shape} does not fill {self.dtype} {self.shape}")
        self.data = a.view(self.dtype).reshape(self.frames, self.rows, self.cols)
        return self

    def _index(self):
        """arena byte offsets of the payload, shape (frames, rows, cols * itemsize)"""
        f = np.arange(self.frames, dtype=np.int64)[:, None, None] * self.frame_stride_bytes
        r = np.arange(self.rows, dtype=np.int64)[None, :, None] * self.pitch_bytes
        c = np.arange(self.cols * self.itemsize, dtype=np.int64)[None, None, :]
        return self.start + f + r + c

    def view(self, image):
        """the payload inside a host image of the arena, as an array of the logical shape (a copy)"""
        return image[self._index().reshape(-1)].view(self.dtype).reshape(self.shape)

    def get(self):
        """the payload as the device holds it now (logical shape, padding dropped)"""
        return self.view(self.arena.download())


class Arena:
    def __init__(self, device="cpu", poison=0xA5):
        self.device, self.poison = torch.device(device), int(poison) & 0xFF
        self.bufs, self._cursor = [], 0
        self.mem = self.base_ptr = self._snap = self._mask = None

    def buf(self, name, role, dtype, shape, align=None, skew=0, pitch=None, frame_stride=None):
        if role not in ROLES:
            raise ValueError(f"role {role!r} not in {ROLES}")
        if self.mem is not None:
            raise RuntimeError("the arena is laid out: add buffers before the first fill()")
        if any(b.name == name for b in self.bufs):
            raise ValueError(f"duplicate buffer {name!r}")
        b = Buf(self, name, role, dtype, shape, align, skew, pitch, frame_stride)
        slot = -(-(self._cursor + b.zone) // SLOT) * SLOT
        b.start = slot + b.skew
        b.lo = self._cursor                                # [lo, start): red zone before; [start + extent, hi): after
        b.hi = self._cursor = b.start + b.extent + b.zone
        self.bufs.append(b)
        return b

    def _layout(self):
        total = self._cursor                               # ends with the last buffer's red zone
        self.mem = torch.empty(total + SLOT, dtype=torch.uint8, device=self.device)
        off = (-self.mem.data_ptr()) % SLOT                # slot 0 on a 256-byte boundary whatever the allocator returned
        self.mem = self.mem[off:off + total]
        self.base_ptr = self.mem.data_ptr()
        assert self.base_ptr % SLOT == 0
        self._total = total
        mask = np.ones(total, bool)                        # True = must not change
        for b in self.bufs:
            if b.role != "in":
                mask[b._index().reshape(-1)] = False
        self._mask = mask

    def fill(self, poison=None):
        """poison everything, then write the inputs' data; (re)usable with another poison byte"""
        if poison is not None:
            self.poison = int(poison) & 0xFF
        if self.mem is None:
            self._layout()
        image = np.full(self._total, self.poison, np.uint8)
        for b in self.bufs:
            if b.role in ("in", "inout"):
                if b.data is None:
                    raise RuntimeError(f"{b.name}: no data set")
                image[b._index().reshape(-1)] = b.data.reshape(-1).view(np.uint8)
        self.mem.copy_(torch.from_numpy(image))
        self._snap = None
        return self

    def download(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        return self.mem.cpu().numpy().copy()

    def host(self):
        """the arena's bytes as a writable NumPy array (CPU arenas only: what a stand-in for an entry writes into)"""
        if self.device.type != "cpu":
            raise RuntimeError("host() needs a CPU arena")
        return self.mem.numpy()

    def snapshot(self):
        self._snap = self.download()
        return self

    def check(self):
        """raise GuardError for the first damaged buffer (all of them are named in the message)"""
        if self._snap is None:
            raise RuntimeError("check() before snapshot()")
        now = self.download()
        bad = (now != self._snap) & self._mask
        if not bad.any():
            return
        found = []
        for b in self.bufs:
            for where, lo, hi in (("before", b.lo, b.start), ("inside", b.start, b.start + b.extent), ("after", b.start + b.extent, b.hi)):
                idx = np.flatnonzero(bad[lo:hi])
                if idx.size:
                    found.append((b.name, where, lo + int(idx[0]) - b.start, idx.size))
        name, where, off, cnt = found[0]
        at = self.bufs[[b.name for b in self.bufs].index(name)].start + off
        detail = f" (0x{self._snap[at]:02x} -> 0x{now[at]:02x}; all damage: {found})"
        raise GuardError(name, where, off, cnt, detail)
