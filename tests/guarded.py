"""Buffers between guard bands, for tests that call the C entry points directly (a helper module, not a conftest): the only guard
implementation for the image and region-graph pipeline.  tests/raw_calls.py runs every raw call on it, tests/rg_train_calls.py the training call; tests/test_guarded.py holds it,
on CPU tensors, to seeing a byte written on either side of a piece.

A kernel that writes a few elements past an extent lands in whatever the allocator put next, unseen.  Here every buffer is a piece
of exactly the stated size, ``skew`` bytes past a 256-byte boundary, in the middle of a tensor of its own that is filled with one byte
value and has at least GUARD bytes on either side of the piece: a write before or past the piece changes a byte this module owns and checks.

Fill values: 0x00, 0xFF, 0xA5 and 0x7F.  0xFF reads as -1 in every integer type and as a NaN in fp32 and fp64, so a missed
initialisation shows as a wrong result, and a wrongly read index is -1 and stays inside the front guard; a pattern that reads as a
large positive integer would turn the same mistake into an out-of-bounds access.  0xA5 and 0x7F are such patterns: they are for
arrays the library only writes (where a reference holds -1 entries, 0xFF would let a missed store pass)."""
import numpy as np
import torch

GUARD = 4096
FILLS = (0x00, 0xFF, 0xA5, 0x7F)


def guarded(nbytes, fill, skew=0, device="cuda"):
    """(whole, piece): `piece` is `nbytes` bytes, `skew` bytes past a 256-byte boundary, in the middle of the uint8 tensor `whole`,
    which is filled with `fill` and has at least GUARD bytes on either side of the piece."""
    whole = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device=device)
    at = GUARD + (skew - (whole.data_ptr() + GUARD)) % 256
    piece = whole[at:at + nbytes]
    assert 0 <= skew < 256 and (whole.data_ptr() + at) % 256 == skew and at >= GUARD and whole.numel() - at - nbytes >= GUARD
    return whole, piece


def guards_intact(whole, piece, fill):
    at = piece.storage_offset()
    return bool((whole[:at] == fill).all()) and bool((whole[at + piece.numel():] == fill).all())


def _of(value, name):
    return value.get(name, value[None]) if isinstance(value, dict) else value


class Arrays:
    """Named arrays, each in a guarded tensor of its own: ``spec`` is name -> (shape, numpy dtype), or name -> a number of bytes
    (a workspace).  ``fill`` and ``skew`` are one value for all, or a dict name -> value whose key None is the default.
    ``ptr(name)`` is the address to hand to the library; ``collect()`` checks every guard and returns the arrays as numpy
    (a workspace as uint8)."""

    def __init__(self, spec, fill, skew=0, device="cuda"):
        self.fill, self.device, self.spec, self.whole, self.piece = {}, device, {}, {}, {}
        for name, what in spec.items():
            shape, dtype = ((int(what),), np.uint8) if np.isscalar(what) else (tuple(int(v) for v in what[0]), np.dtype(what[1]))
            self.spec[name], self.fill[name] = (shape, np.dtype(dtype)), _of(fill, name)
            assert self.fill[name] in FILLS
            self.whole[name], self.piece[name] = guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, self.fill[name], _of(skew, name), device)

    def ptr(self, name):
        return self.whole[name].data_ptr() + self.piece[name].storage_offset()      # (an empty piece has no data_ptr of its own)

    def nbytes(self, name):
        return self.piece[name].numel()

    def refill(self, name, start=0):
        """Bytes ``start`` .. of the piece back to the fill value (the part of a workspace a call is not given)."""
        self.piece[name][start:] = self.fill[name]

    def tail_intact(self, name, start):
        return bool((self.piece[name][start:] == self.fill[name]).all())

    def check_guards(self):
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        for name in self.spec:
            assert guards_intact(self.whole[name], self.piece[name], self.fill[name]), f"a byte outside {name} was written"

    def collect(self):
        self.check_guards()
        return {name: self.piece[name].cpu().numpy().view(dtype).reshape(shape).copy() for name, (shape, dtype) in self.spec.items()}
