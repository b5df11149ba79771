"""Shared pieces of tests/test_gpu_abi_strides.py and tests/test_gpu_abi_workspace.py: device arrays laid out as windows
of wider, poisoned allocations, and a workspace server that hands out exactly the asked bytes between guard bands.

A ``Win`` is one argument of a C ABI call.  Its allocation is larger than the array: ``lead`` elements in front, the pitch
gaps of its strides, ``tail`` elements behind.  Everything outside the array holds ``fill`` (NaN for an input, the
sentinel for an output), so a read of a gap poisons the result and a write to one is seen afterwards.
"""
import ctypes

import numpy as np
import torch

from bayesianoptimizer_amd import _capi

DEV = torch.device("cuda", 0)
SENT = -12345.5                 # a finite odd value no result takes (tests/test_gpu_svgp_zgrad.py)
ISENT = 0x5A5A5A5A              # the same for int32 / int64 outputs
NAN = float("nan")
_BITS = {torch.float64: torch.int64, torch.int64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8}


def t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), device=DEV)


def ptr(a):
    if a is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p((a.view if isinstance(a, Win) else a).data_ptr())


def bits(a):
    """The array's bit patterns (NaN payloads and signed zeros count)."""
    return a.view(_BITS[a.dtype])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


class Win:
    """An array of ``shape`` and element ``strides`` inside a 1-D allocation filled with ``fill``; ``data`` (any tensor
    that broadcasts to the shape) is copied in."""

    def __init__(self, shape, strides=None, fill=SENT, data=None, lead=2, tail=6, dtype=torch.float64):
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= s
        strides = tuple(int(s) for s in strides)
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
        self.fill, self.lead = fill, lead
        self.buf = torch.full((lead + span + tail,), fill, dtype=dtype, device=DEV)
        self.view = self.buf.as_strided(shape, strides, lead)
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        self.mask.as_strided(shape, strides, lead).fill_(True)
        if data is not None:
            self.view.copy_(data)
        self.snap = None

    def freeze(self):
        """Remember the whole allocation (a const input): ``unchanged`` compares against it."""
        self.snap = self.buf.clone()
        return self

    def unchanged(self):
        return same_bits(self.buf, self.snap)

    def outside_intact(self, defined=None):
        """Every element outside the array (or outside ``defined``, a bool tensor of the array's shape) still holds the
        fill pattern."""
        mask = self.mask
        if defined is not None:
            mask = torch.zeros_like(self.mask)
            mask.as_strided(self.view.shape, self.view.stride(), self.lead).copy_(defined)
        ref = torch.full((1,), self.fill, dtype=self.buf.dtype, device=DEV)
        return bool((bits(self.buf)[~mask] == bits(ref)).all())

    def sentinels(self, region=None):
        """How many elements of the array (or of ``region``, a view of it) still hold the sentinel."""
        a = self.view if region is None else region
        hit = torch.isnan(a) if self.fill != self.fill else a == self.fill
        return int(hit.sum().item())


def rows(data, ld, fill=NAN, col0=0, lead=1, **kw):
    """A 2-D input whose rows lie ``ld`` apart, starting ``col0`` columns into a wider matrix."""
    r, c = data.shape
    assert ld >= c + col0
    return Win((r, c), (ld, 1), fill, data, lead=lead + col0, tail=ld, **kw).freeze()


def matrix(npad, ld, fill=SENT, data=None, extra_rows=2):
    """An npad x npad matrix of even pitch ``ld`` at a 16-byte aligned address, ``extra_rows`` rows of fill behind it."""
    assert ld % 2 == 0
    return Win((npad, npad), (ld, 1), fill, data, lead=2, tail=extra_rows * ld)


def stack(B, shape, strides, gap, fill=SENT, data=None, lead=2, **kw):
    """B arrays of ``shape`` / ``strides``, ``gap`` elements further apart than one array needs.  Returns (Win, stride)."""
    one = 1 + sum((s - 1) * st for s, st in zip(shape, strides))
    stride = one + gap
    return Win((B,) + tuple(shape), (stride,) + tuple(strides), fill, data, lead=lead, tail=gap + 4, **kw), stride


def out_i32(nvals=1):
    return Win((nvals,), None, ISENT, dtype=torch.int32, lead=1, tail=3)


def out_i64(nvals=1):
    return Win((nvals,), None, ISENT, dtype=torch.int64, lead=1, tail=3)


def out_f64(*shape):
    return Win(shape, None, SENT, lead=1, tail=5)


def plain_ws(nbytes):
    """A workspace of exactly the reported bytes (test_gpu_abi_strides.py: its subject is the other arguments)."""
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


def ws_size(fn, *args):
    nbytes = ctypes.c_size_t()
    assert fn(*args, ctypes.byref(nbytes)) == _capi.GPX_OK
    return nbytes.value


def ok(engine, status):
    _capi.check(status, engine.handle)


def lower_zero(W):
    return not bool(torch.tril(W, -1).any())


GUARD = 4096


class GuardedWorkspace:
    """Replaces ``engine.workspace``: every request is served from a fresh allocation of offset + asked + 4096 bytes of
    0xFF, the workspace starting ``offset`` bytes in; request number ``short_at`` (if any) gets one byte less than it asked
    for (the rejection test).  The requests and their allocations are kept, so the caller compares the sizes with the size
    query and checks the bytes in front of and behind every workspace after a synchronisation."""

    def __init__(self, offset, short_at=None):
        self.offset, self.short_at = offset, short_at
        self.asked, self.bufs = [], []

    def __call__(self, key, nbytes):
        nbytes = int(nbytes)
        big = torch.full((self.offset + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        assert big.data_ptr() % 256 == 0
        short = 1 if len(self.asked) == self.short_at else 0
        self.asked.append(nbytes)
        self.bufs.append((big, nbytes))
        return big[self.offset:self.offset + nbytes - short]

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(bool((big[:self.offset] == 0xFF).all()) and bool((big[self.offset + nb:] == 0xFF).all())
                   for big, nb in self.bufs)
