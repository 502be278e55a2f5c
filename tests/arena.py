"""A guarded device arena for the -m gpu bounds tests (tests/test_gpu_bounds.py).

Every device argument of one library call lives in ONE allocation, each region between two guard bands of at least GUARD
bytes.  Guards, and every payload byte that was not uploaded, hold the byte 0xA5, so the word 0xA5A5A5A5: it is above P, so a
kernel that reads it as a field element produces a wrong word, and no canonical output equals it.  After the call the whole
arena is downloaded once and check() asserts that every guard byte and every `in` region is what was uploaded; the `out` /
`inout` payloads come back for the comparison with the oracle.

Two halves: the layout and the image check are pure numpy (tests/test_cpu_arena.py runs them without a GPU); the device half
(one tstwo_malloc, one upload, one download) needs the library and imports it lazily.
"""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5A5A5A5
SENTINEL_BYTE = 0xA5
GUARD = 16384                 # bytes before and after every region
ALIGN = 16
ROLES = ("in", "out", "inout")
OFFSETS = (0, 4, 8, 12)       # byte offset from a 16-byte boundary (0 = aligned; the others force the scalar dispatches)


class Region:
    """name, role, placement and either the payload to upload (`data`: any numpy array, taken as bytes) or, for an output
    that starts as sentinel, its size in bytes (`nbytes`)."""

    def __init__(self, name, role, data=None, nbytes=None, offset=0):
        assert role in ROLES, role
        assert offset in OFFSETS, offset
        if data is not None:
            data = np.ascontiguousarray(data)
            data = data.reshape(-1).view(np.uint8) if data.size else np.zeros(0, dtype=np.uint8)
            assert nbytes is None or nbytes == data.size
            nbytes = data.size
        assert nbytes is not None and nbytes >= 0
        assert role != "in" or data is not None, f"input region {name} has nothing to upload"
        self.name, self.role, self.data, self.nbytes, self.offset = name, role, data, int(nbytes), offset


def rin(name, data, offset=0):
    return Region(name, "in", data=data, offset=offset)


def rout(name, n_words, offset=0):
    return Region(name, "out", nbytes=4 * int(n_words), offset=offset)


def rinout(name, data, offset=0):
    return Region(name, "inout", data=data, offset=offset)


class Layout:
    """Byte offsets of the regions inside one arena: start[name], and `total` bytes in all."""

    def __init__(self, regions):
        self.regions = list(regions)
        names = [r.name for r in self.regions]
        assert len(set(names)) == len(names), "region names must be unique"
        self.start = {}
        cur = 0
        for r in self.regions:
            cur += GUARD
            cur = (cur + ALIGN - 1) // ALIGN * ALIGN + r.offset
            self.start[r.name] = cur
            cur += r.nbytes
        self.total = (cur + GUARD + ALIGN - 1) // ALIGN * ALIGN

    def end(self, name):
        return self.start[name] + self.by_name(name).nbytes

    def by_name(self, name):
        for r in self.regions:
            if r.name == name:
                return r
        raise KeyError(name)

    def guards(self):
        """[(lo, hi, region, side)]: every guard byte range with the region it is reported against.  The gap between two
        regions is split in the middle: the first half is `after` the earlier region, the second `before` the later one."""
        out = []
        prev_end, prev = 0, None
        for r in self.regions:
            lo, hi = prev_end, self.start[r.name]
            mid = lo if prev is None else (lo + hi) // 2
            if prev is not None:
                out.append((lo, mid, prev, "after"))
            out.append((mid, hi, r, "before"))
            prev_end, prev = hi + r.nbytes, r
        if prev is not None:
            out.append((prev_end, self.total, prev, "after"))
        return out

    def image(self):
        """The arena as uploaded: sentinel everywhere, the regions' data in place."""
        img = np.full(self.total, SENTINEL_BYTE, dtype=np.uint8)
        for r in self.regions:
            if r.data is not None:
                img[self.start[r.name]:self.start[r.name] + r.nbytes] = r.data
        return img


def _span(changed):
    idx = np.flatnonzero(changed)
    return int(idx[0]), int(idx[-1])


def find_violations(layout, before, after):
    """Every guard range and every `in` region of `after` that differs from `before`, as text: the region, the side (before /
    after / input) and the first and last changed byte offsets relative to the region's first byte."""
    assert before.dtype == np.uint8 and after.dtype == np.uint8 and before.size == after.size == layout.total
    msgs = []
    for lo, hi, r, side in layout.guards():
        seg = after[lo:hi]
        if (seg != SENTINEL_BYTE).any():
            a, b = _span(seg != SENTINEL_BYTE)
            s = layout.start[r.name]
            msgs.append(f"guard {side} region '{r.name}' ({r.role}, {r.nbytes} bytes) was written: first changed byte at "
                        f"{lo + a - s:+d}, last at {lo + b - s:+d} relative to the region's start")
    for r in layout.regions:
        if r.role == "in":
            s = layout.start[r.name]
            diff = after[s:s + r.nbytes] != before[s:s + r.nbytes]
            if diff.any():
                a, b = _span(diff)
                msgs.append(f"input region '{r.name}' ({r.nbytes} bytes) was modified: first changed byte at {a:+d}, last at "
                            f"{b:+d} relative to the region's start")
    return msgs


def check_image(layout, before, after, dtype=np.uint32):
    """Assert the guards and inputs of `after` are those of `before`; return {name: payload} of the out / inout regions."""
    msgs = find_violations(layout, before, after)
    assert not msgs, "; ".join(msgs)
    res = {}
    for r in layout.regions:
        if r.role != "in":
            s = layout.start[r.name]
            raw = after[s:s + r.nbytes].tobytes()
            res[r.name] = np.frombuffer(raw, dtype=dtype if r.nbytes % np.dtype(dtype).itemsize == 0 else np.uint8).copy()
    return res


class Arena:
    """The device half: one tstwo_malloc, one upload of the whole image, pointers into it, one download, check(), free().
    Use as a context manager so the block is freed at the end of the test."""

    def __init__(self, regions):
        from tstwo_amd import _lib as L
        self._L = L
        self.layout = Layout(regions)
        self.before = self.layout.image()
        self.buf = L.DeviceBuffer(self.layout.total)
        assert self.buf.ptr % ALIGN == 0
        self.buf.upload(self.before)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False

    def addr(self, name, byte_offset=0):
        return self.buf.ptr + self.layout.start[name] + byte_offset

    def ptr(self, name, byte_offset=0):
        import ctypes
        return ctypes.c_void_p(self.addr(name, byte_offset))

    def p4(self, names):
        return self._L.p4([self.addr(n) for n in names])

    def ptrs(self, names):
        return self._L.ptr_array([self.addr(n) for n in names])

    def check(self, dtype=np.uint32):
        """Download the arena (synchronises), assert guards and inputs, return the out / inout payloads."""
        after = self.buf.download(np.uint8)
        return check_image(self.layout, self.before, after, dtype)

    def free(self):
        if self.buf is not None:
            self.buf.free()
            self.buf = None
