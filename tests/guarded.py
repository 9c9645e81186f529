"""Guarded buffers: an output buffer between two guard zones that the test owns, so that a store before or behind the
payload changes a byte the test can see, and is reported as an offset, where a buffer of exactly the size asked for lets it
land in a neighbour's memory unseen.

Sizing.  A guard has to hold the furthest stray store the entries could make by one mistake in an index or a bound: one
whole block of 256 threads each storing the widest element (tjamd_union_tract_summary, 64 bytes: 16 KiB), one row of
counts too many (4096 samples of 4 bytes: 16 KiB), or one list entry too many of per-sample values (5 statistics of 4096
doubles: 160 KiB).  GUARD_BYTES is 256 KiB, above all three and above the 64 KiB floor, so such a store stays inside the
one allocation and cannot fault the device: the failing test names the offset instead.

The guards carry a byte pattern that depends on the position, (i * 131 + 17) & 0xFF, so that a stray store of any constant,
0 and -1 included, and of any run of one value, changes at least one byte; the payload starts with another pattern,
(i * 29 + 101) & 0xFF, so that a test can tell the elements a call wrote from those it left alone.
"""
import contextlib
import ctypes as C

import numpy as np

GUARD_BYTES = 256 << 10
ALIGN = 512                              # what a fresh torch allocation gives a tensor: kernels take their usual (vector) paths
assert GUARD_BYTES >= 64 << 10 and GUARD_BYTES % ALIGN == 0


def guard_pattern(n):
    return ((np.arange(n, dtype=np.int64) * 131 + 17) & 0xFF).astype(np.uint8)


def payload_pattern(n):
    return ((np.arange(n, dtype=np.int64) * 29 + 101) & 0xFF).astype(np.uint8)


def _first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return int(bad[0]) if len(bad) else None


class GuardedHost:
    """nbytes of host memory between two guards, in one numpy allocation; .ptr is the payload's address"""

    def __init__(self, nbytes, guard=GUARD_BYTES):
        self.nbytes, self.guard = int(nbytes), int(guard)
        self._raw = np.empty(2 * self.guard + self.nbytes + ALIGN, dtype=np.uint8)
        self._off = self.guard + (-(self._raw.ctypes.data + self.guard)) % ALIGN      # the front guard: [_off - guard, _off)
        self._raw[:] = 0xC3
        self._front()[:] = guard_pattern(self.guard)
        self._back()[:] = guard_pattern(self.guard)
        self.payload[:] = payload_pattern(self.nbytes)

    def _front(self):
        return self._raw[self._off - self.guard: self._off]

    def _back(self):
        return self._raw[self._off + self.nbytes: self._off + self.nbytes + self.guard]

    @property
    def payload(self):
        return self._raw[self._off: self._off + self.nbytes]

    @property
    def ptr(self):
        return self._raw.ctypes.data + self._off

    @property
    def c(self):
        return C.c_void_p(self.ptr)

    def view(self, dtype, n=None):
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if n is None else int(n)
        assert n * dt.itemsize <= self.nbytes
        return self.payload[: n * dt.itemsize].copy().view(dt)

    def untouched(self):
        """the payload still holds its first pattern: nothing was written to it"""
        return bool((self.payload == payload_pattern(self.nbytes)).all())

    def damage(self):
        """None, or the offset of the first changed guard byte relative to the payload (negative: in front of it)"""
        want = guard_pattern(self.guard)
        at = _first_difference(self._front(), want)
        if at is not None:
            return at - self.guard
        at = _first_difference(self._back(), want)
        return None if at is None else self.nbytes + at

    def check(self, what="buffer"):
        at = self.damage()
        assert at is None, f"{what}: a byte outside the payload of {self.nbytes} bytes was changed, the first at offset {at} from its start"


class GuardedDevice:
    """nbytes of device memory between two guards, in one torch uint8 allocation; .ptr is the payload's address, a
    multiple of 512 as that of a tensor of its own would be"""

    _patterns = {}

    def __init__(self, nbytes, guard=GUARD_BYTES, device="cuda"):
        import torch
        self.nbytes, self.guard = int(nbytes), int(guard)
        self._raw = torch.empty(2 * self.guard + self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        self._off = self.guard + (-(self._raw.data_ptr() + self.guard)) % ALIGN
        self._raw.fill_(0xC3)
        self._front().copy_(self._pattern(self.guard))
        self._back().copy_(self._pattern(self.guard))
        if self.nbytes:
            self.payload.copy_(torch.from_numpy(payload_pattern(self.nbytes)).to(self._raw.device))
        torch.cuda.synchronize()
        assert self.ptr % ALIGN == 0

    def _pattern(self, n):
        import torch
        key = (str(self._raw.device), n)
        if key not in GuardedDevice._patterns:
            GuardedDevice._patterns[key] = torch.from_numpy(guard_pattern(n)).to(self._raw.device)
        return GuardedDevice._patterns[key]

    def _front(self):
        return self._raw[self._off - self.guard: self._off]

    def _back(self):
        return self._raw[self._off + self.nbytes: self._off + self.nbytes + self.guard]

    @property
    def payload(self):
        """the payload as a uint8 tensor (a view: what a later call reads as its input)"""
        return self._raw[self._off: self._off + self.nbytes]

    @property
    def ptr(self):
        return self._raw.data_ptr() + self._off

    @property
    def c(self):
        return C.c_void_p(self.ptr)

    def view(self, dtype, n=None):
        """n elements of the payload, downloaded"""
        dt = np.dtype(dtype)
        n = self.nbytes // dt.itemsize if n is None else int(n)
        assert n * dt.itemsize <= self.nbytes
        return np.frombuffer(self.payload[: n * dt.itemsize].cpu().numpy().tobytes(), dtype=dt)

    def untouched(self):
        return bool((self.payload.cpu().numpy() == payload_pattern(self.nbytes)).all())

    def damage(self):
        import torch
        want = self._pattern(self.guard)
        if torch.equal(self._front(), want) and torch.equal(self._back(), want):
            return None
        at = _first_difference(self._front().cpu().numpy(), want.cpu().numpy())
        if at is not None:
            return at - self.guard
        return self.nbytes + _first_difference(self._back().cpu().numpy(), want.cpu().numpy())

    def check(self, what="buffer"):
        at = self.damage()
        assert at is None, f"{what}: a byte outside the payload of {self.nbytes} bytes was changed, the first at offset {at} from its start"


def _snapshot(x):
    if isinstance(x, np.ndarray):
        return x.copy()
    return x.detach().clone()                            # a torch tensor, on whatever device


def _same_bits(x, snap):
    if isinstance(x, np.ndarray):
        return x.shape == snap.shape and x.tobytes() == snap.tobytes()
    import torch
    return x.shape == snap.shape and torch.equal(x.contiguous().view(torch.uint8), snap.contiguous().view(torch.uint8))


@contextlib.contextmanager
def frozen(*tensors_or_arrays):
    """the const inputs of a call (numpy arrays, torch tensors; None is skipped): on leaving the block they must be bit for
    bit what they were on entering it"""
    held = [(i, x, _snapshot(x)) for i, x in enumerate(tensors_or_arrays) if x is not None]
    yield
    for i, x, snap in held:
        assert _same_bits(x, snap), f"input {i} of the call was changed by it"
