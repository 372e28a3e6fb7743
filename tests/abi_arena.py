"""One big byte buffer cut into the arrays of a `_dev` call, the way a caller that owns a single device allocation binds the
library: every array sits between guard bands of a known byte pattern, at an address of the caller's choosing,
and check() tells which call wrote where it had no business.  Works on CPU tensors too (tests/test_abi_arena.py proves with
planted faults that it sees them).  Test helper.

Placement of an array: `aligned=True` puts it on a multiple of 256; `aligned=False` at the natural alignment of its element type
and no better -- address = itemsize (mod 16) for 2-, 4- and 8-byte types, an odd address for bytes; `address_mod=(m, r)` asks
for address = r (mod m) outright (a workspace at exactly the alignment a header states: (2 N, N); one byte off: (256, 1))."""
import collections

import numpy as np
import torch

PATTERN = 0xA5
GUARD = 4096
ROLES = ("in", "out", "ws")

_Entry = collections.namedtuple("_Entry", "name role offset nbytes stated dtype shape")


def itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def natural_residue(dtype):
    """(m, r) of the natural-alignment placement of `dtype`."""
    s = itemsize(dtype)
    if s not in (1, 2, 4, 8):
        raise ValueError("no natural placement for an element of %d bytes" % s)
    return (16, s) if s > 1 else (2, 1)


def _numel(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def room(specs):
    """Bytes that surely hold the arrays `specs` = [(dtype, shape) or nbytes, ...] whatever their placement."""
    total = GUARD + 512
    for s in specs:
        nbytes = int(s) if isinstance(s, (int, np.integer)) else itemsize(s[0]) * _numel(s[1])
        total += nbytes + GUARD + 512
    return total


class Arena:
    def __init__(self, nbytes, device="cpu"):
        self.buf = torch.full((int(nbytes),), PATTERN, dtype=torch.uint8, device=device)
        self.guard = torch.zeros((int(nbytes),), dtype=torch.bool, device=device)   # the bytes check() looks at
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.entries = collections.OrderedDict()
        self.views = {}

    def _place(self, nbytes, mod):
        m, r = mod
        start = self.cursor + GUARD
        start += (r - (self.base + start)) % m
        end = start + nbytes + GUARD
        if end > self.buf.numel():
            raise ValueError("arena of %d bytes is full" % self.buf.numel())
        self.cursor = start + nbytes   # the next array's front band begins where this one's back band does: they may share it
        return start

    def carve(self, name, dtype, shape, role, aligned=True, address_mod=None, stated_bytes=None):
        """The array `name` as a contiguous tensor view.  role "ws" with stated_bytes < its size: the bytes from stated_bytes
        on are watched like a guard band (a call told that size must leave them alone)."""
        if role not in ROLES:
            raise ValueError("role must be one of %s" % (ROLES,))
        if name in self.entries:
            raise ValueError("array %r carved twice" % name)
        shape = tuple(int(d) for d in shape)
        nbytes = itemsize(dtype) * _numel(shape)
        mod = address_mod if address_mod is not None else ((256, 0) if aligned else natural_residue(dtype))
        off = self._place(nbytes, mod)
        stated = nbytes if stated_bytes is None else int(stated_bytes)
        if not 0 <= stated <= nbytes or (stated != nbytes and role != "ws"):
            raise ValueError("stated_bytes is for a workspace, within its size")
        self.guard[off - GUARD:off] = True
        self.guard[off + stated:off + nbytes + GUARD] = True
        self.guard[off:off + stated] = False   # (a front band shared with the previous array's back band stays watched)
        self.entries[name] = _Entry(name, role, off, nbytes, stated, dtype, shape)
        view = self.buf[off:off + nbytes].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() == self.base + off
        self.views[name] = view
        return view

    def address(self, name):
        return self.base + self.entries[name].offset

    def bytes_of(self, name):
        e = self.entries[name]
        return self.buf[e.offset:e.offset + e.nbytes]

    def fill(self, name, byte):
        self.bytes_of(name).fill_(int(byte))

    def holds_pattern(self, name):
        return bool((self.bytes_of(name) == PATTERN).all().item())

    @property
    def guard_bytes(self):
        return int(self.guard.sum().item())

    def check(self):
        """[(array, byte offset relative to the array's first byte)] of every array with a byte of its guard bands, or past its
        stated size, off the pattern: the first such byte of each, negative in the band before it.  Empty = clean."""
        bad = torch.nonzero(self.guard & (self.buf != PATTERN)).reshape(-1).cpu().numpy()
        found = []
        if bad.size == 0:
            return found
        for e in self.entries.values():
            lo, hi = e.offset - GUARD, e.offset + e.nbytes + GUARD
            mine = bad[(bad >= lo) & (bad < hi)]
            mine = mine[(mine < e.offset) | (mine >= e.offset + e.stated)]
            if mine.size:
                found.append((e.name, int(mine[0]) - e.offset))
        return found


def same_bits(a, b):
    """Bit-for-bit equality of two tensors or arrays (NaN payloads and signed zeros included)."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
