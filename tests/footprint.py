"""The write footprint of a call, observed from outside, byte for byte
(tests/test_gpu_footprint.py; the check itself is tested on the host in
tests/test_footprint_harness.py).  Not a test module.

An Arena puts every buffer of a call -- sources, parity, outputs, erasure
lists, workspace, status -- into ONE allocation, a device tensor or a pinned
host tensor, with a guard band of at least GUARD bytes before the first
buffer, between any two and after the last, so that an overrun from any
buffer lands in a guard or in a neighbour and never in allocator slack.  A
buffer starts at a multiple of ALIGN bytes plus an optional byte offset (the
misaligned cases).  The whole arena is filled with seeded noise, not with a
constant: a kernel that happens to write the fill byte must not pass.

A row buffer holds (rows - 1) * pitch + len bytes, what the library's row
calls ask for: the padding of the last row is already guard.  A flat buffer
(workspace, status, lists) holds exactly its declared size.

check(before, after, allowed) compares two host copies of the arena: every
byte outside the allowed ranges must be unchanged, and a failure names the
region of the first offending byte:
    guard before src            the band in front of the first buffer
    guard after out             the band behind a row buffer
    out row (b=1, i=3) padding  [len, pitch) of a row
    out row (b=1, i=3)          [0, len) of a row that the call may not write
    workspace + 17 past its size   the 17th byte behind a flat buffer
    err + 5                     byte 5 of a flat buffer
"""
import bisect

import numpy as np

GUARD = 4096
ALIGN = 256


def align_up(x, a):
    return (x + a - 1) // a * a


class Region:
    """One buffer of the arena: [start, start + size).  A row buffer has
    blocks x per rows of `length` bytes at `pitch`."""

    def __init__(self, name, start, size, blocks=0, per=0, pitch=0, length=0):
        self.name, self.start, self.size = name, start, size
        self.blocks, self.per, self.pitch, self.length = blocks, per, pitch, length

    @property
    def end(self):
        return self.start + self.size

    @property
    def is_rows(self):
        return self.per > 0

    def row_start(self, b, i):
        return self.start + (b * self.per + i) * self.pitch

    def row_ranges(self, blocks=None):
        """[0, len) of every row of the first `blocks` blocks."""
        nb = self.blocks if blocks is None else blocks
        if not self.length:
            return []
        return [(self.row_start(b, i), self.row_start(b, i) + self.length)
                for b in range(nb) for i in range(self.per)]

    def head(self, nbytes):
        """The first nbytes of a flat buffer."""
        assert 0 <= nbytes <= self.size
        return [(self.start, self.start + nbytes)] if nbytes else []

    def describe(self, off):
        """The name of arena byte `off`, inside this buffer."""
        rel = off - self.start
        if not self.is_rows:
            return f"{self.name} + {rel}"
        r, col = divmod(rel, self.pitch) if self.pitch else (0, rel)
        b, i = divmod(r, self.per)
        where = f"{self.name} row (b={b}, i={i})"
        return where + " padding" if col >= self.length else where


class Layout:
    """Where the buffers of an arena lie; host arithmetic only."""

    def __init__(self):
        self.regions = []
        self.by_name = {}

    def _place(self, offset):
        assert 0 <= offset < ALIGN
        prev_end = self.regions[-1].end if self.regions else 0
        return align_up(prev_end + GUARD, ALIGN) + offset

    def _add(self, r):
        assert r.name not in self.by_name
        self.regions.append(r)
        self.by_name[r.name] = r
        return r

    def rows(self, name, blocks, per, pitch, length, offset=0):
        """blocks x per rows of `length` bytes at `pitch`, `offset` bytes past
        the alignment."""
        assert length <= pitch or blocks * per <= 1
        n = blocks * per
        size = (n - 1) * pitch + length if n else 0
        return self._add(Region(name, self._place(offset), size, blocks, per, pitch, length))

    def flat(self, name, size, offset=0):
        return self._add(Region(name, self._place(offset), size))

    def __getitem__(self, name):
        return self.by_name[name]

    @property
    def size(self):
        return (self.regions[-1].end if self.regions else 0) + GUARD

    def describe(self, off):
        """The name of arena byte `off`."""
        assert 0 <= off < self.size
        idx = bisect.bisect_right([r.start for r in self.regions], off) - 1
        if idx < 0:
            return f"guard before {self.regions[0].name}"
        r = self.regions[idx]
        if off < r.end:
            return r.describe(off)
        if r.is_rows:
            return f"guard after {r.name}"
        return f"{r.name} + {off - r.end + 1} past its size"

    def check(self, before, after, allowed):
        """before, after: numpy uint8 copies of the arena; allowed: [(start,
        end)] byte ranges the call may write.  Everything else must be equal;
        raises AssertionError naming the region of the first other byte."""
        assert before.dtype == np.uint8 and after.dtype == np.uint8
        assert before.shape == after.shape == (self.size,)
        diff = before != after
        for s, e in allowed:
            assert 0 <= s <= e <= self.size
            diff[s:e] = False
        if diff.any():
            off = int(np.argmax(diff))
            raise AssertionError(f"{self.describe(off)}: arena byte {off} written "
                                 f"(0x{int(before[off]):02x} -> 0x{int(after[off]):02x}), "
                                 f"{int(diff.sum())} bytes outside the footprint in all")

    def noise(self, seed):
        return np.random.default_rng(seed).integers(0, 256, self.size, dtype=np.uint8)


def decode_allowed(lay, workspace_bytes, blocks=None, out=True, prepare=True):
    """What a decode of the first `blocks` blocks may write: [0, len) of each
    output row (out), the first workspace_bytes bytes of the workspace and the
    first `blocks` ints of the status (prepare).  Never src, par or err."""
    nb = lay["out"].blocks if blocks is None else blocks
    allowed = lay["out"].row_ranges(nb) if out else []
    if prepare:
        if "workspace" in lay.by_name:
            allowed += lay["workspace"].head(workspace_bytes)
        allowed += lay["status"].head(4 * nb)
    return allowed


def encode_allowed(lay, blocks=None):
    """What an encode may write: [0, len) of each parity row."""
    return lay["par"].row_ranges(blocks)


class Arena(Layout):
    """A Layout with its allocation: `device` a torch device, or None for a
    pinned host tensor.  allocate() after the buffers are laid out."""

    def allocate(self, device=None, seed=1):
        import torch
        fill = torch.from_numpy(self.noise(seed))
        if device is None:
            self.t = torch.empty(self.size, dtype=torch.uint8).pin_memory()
            self.t.copy_(fill)
        else:
            self.t = fill.to(device)
        assert self.t.data_ptr() % ALIGN == 0
        return self

    def buf(self, name):
        """The bytes of a buffer, a view."""
        r = self[name]
        return self.t[r.start: r.end]

    def ptr(self, name):
        return self.t.data_ptr() + self[name].start

    def view(self, name):
        """[blocks, per, len] view of a row buffer."""
        r = self[name]
        return self.t.as_strided((r.blocks, r.per, r.length), (r.per * r.pitch, r.pitch, 1), r.start)

    def ints(self, name):
        """A flat buffer as int32."""
        import torch
        return self.buf(name).view(torch.int32)

    def snapshot(self):
        """A host copy of the whole arena (numpy), for check()."""
        return self.t.cpu().numpy().copy()
