"""Device buffers between guard bands, for tests that call the C entry points directly (a helper module, not a conftest).

A kernel that writes a few elements past an extent lands in whatever the allocator put next, unseen.  Here every buffer is a piece
of exactly the stated size, on a 256-byte boundary, in the middle of a tensor of its own that is filled with one byte value and has
at least GUARD bytes on either side of the piece: a write before or past the piece changes a byte this module owns and checks.

Fill values: 0x00 and 0xFF only.  0xFF reads as -1 in every integer type and as a NaN in fp32 and fp64, so a missed initialisation
shows as a wrong result, and a wrongly read index is -1 and stays inside the front guard; a pattern that reads as a large positive
integer would turn the same mistake into an out-of-bounds access."""
import numpy as np
import torch

GUARD = 4096


def guarded(nbytes, fill):
    """(whole, piece): `piece` is `nbytes` bytes on a 256-byte boundary in the middle of the uint8 device tensor `whole`, which is
    filled with `fill` and has at least GUARD bytes on either side of the piece."""
    whole = torch.full((nbytes + 2 * GUARD + 256,), fill, dtype=torch.uint8, device="cuda")
    at = GUARD + (-(whole.data_ptr() + GUARD)) % 256
    piece = whole[at:at + nbytes]
    assert piece.data_ptr() % 256 == 0 and at >= GUARD and whole.numel() - at - nbytes >= GUARD
    return whole, piece


def guards_intact(whole, piece, fill):
    at = piece.data_ptr() - whole.data_ptr()
    return bool((whole[:at] == fill).all()) and bool((whole[at + piece.numel():] == fill).all())


class Arrays:
    """Named arrays, each in a guarded tensor of its own: ``spec`` is name -> (shape, numpy dtype), or name -> a number of bytes
    (a workspace).  ``ptr(name)`` is the device address to hand to the library; ``collect()`` checks every guard and returns the
    arrays as numpy (a workspace as uint8)."""

    def __init__(self, spec, fill):
        assert fill in (0x00, 0xFF)
        self.fill, self.spec, self.whole, self.piece = fill, {}, {}, {}
        for name, what in spec.items():
            shape, dtype = ((int(what),), np.uint8) if np.isscalar(what) else (tuple(int(v) for v in what[0]), np.dtype(what[1]))
            self.spec[name] = (shape, np.dtype(dtype))
            self.whole[name], self.piece[name] = guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill)

    def ptr(self, name):
        return self.piece[name].data_ptr()

    def nbytes(self, name):
        return self.piece[name].numel()

    def refill(self, name, start=0):
        """Bytes ``start`` .. of the piece back to the fill value (the part of a workspace a call is not given)."""
        self.piece[name][start:] = self.fill

    def tail_intact(self, name, start):
        return bool((self.piece[name][start:] == self.fill).all())

    def check_guards(self):
        torch.cuda.synchronize()
        for name in self.spec:
            assert guards_intact(self.whole[name], self.piece[name], self.fill), f"a byte outside {name} was written"

    def collect(self):
        self.check_guards()
        return {name: self.piece[name].cpu().numpy().view(dtype).reshape(shape).copy() for name, (shape, dtype) in self.spec.items()}
