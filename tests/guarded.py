"""A caller's float buffer as include/ugsm.h allows it (test infrastructure): at any 4-byte base, between two guard bands.

    guarded(ctx, nfloats, shift, init=None, const=False) -> (payload pointer, check)

allocates GUARD + shift + nfloats + GUARD floats, fills every byte with POISON (a byte pattern, not NaN: results hold NaNs of their own), copies
`init` to the payload and returns the payload's address, base + 4 * (GUARD + shift): shift 0 is a 16-byte base, 1 and 3 are 4-byte bases, 2 an
8-byte base.  check(what) reads the whole allocation back, asserts that every byte in front of the payload (the shift floats included) and behind
it is still POISON, for a `const` buffer also that the payload is byte for byte what was uploaded, and returns the payload as float32.
GUARD is wider than any tile row plus a quad, so a store a few floats or a row off still lands inside the allocation.

Guards collects the buffers of one test: buf() as guarded(), check() by pointer, done() checks every buffer that was not checked yet (the
inputs) and frees them all.  done() is meant for a `finally`: where an assertion of the test is already on its way out, that first failure
stays the one reported and what done() finds is printed and attached to it as a note, not raised in its place.
"""
import sys

import numpy as np

GUARD = 4096        # floats on either side
POISON = 0xA5       # the clouds' poison byte (tests/test_gpu_cloud.py)
SHIFTS = (0, 1, 2, 3)


def _touched(band, what, where, origin):
    bad = np.flatnonzero(band != POISON)
    if bad.size:
        raise AssertionError(f"{what}: guard: {bad.size} bytes {where} the buffer were written, from byte {int(bad[0]) - origin} to byte "
                             f"{int(bad[-1]) - origin} relative to the payload's {'start' if origin else 'end'}")


def guarded(ctx, nfloats, shift, init=None, const=False):
    assert shift in SHIFTS and nfloats > 0
    total = 4 * (2 * GUARD + shift + nfloats)
    lo, hi = 4 * (GUARD + shift), 4 * (GUARD + shift + nfloats)
    raw = np.full(total, POISON, np.uint8)
    if init is not None:
        src = np.ascontiguousarray(init, np.float32).reshape(-1)
        assert src.size == nfloats, (src.size, nfloats)
        raw[lo:hi] = src.view(np.uint8)
    else:
        assert not const, "a const buffer has contents"
    base = ctx.to_device(raw)
    assert base % 16 == 0, f"the allocator's base {base:#x} is not 16-byte aligned: shift {shift} would not be the residue it stands for"
    sent = raw[lo:hi].copy() if const else None

    def check(what=""):
        back = ctx.to_host(base, (total,), np.uint8)
        _touched(back[:lo], what, "in front of", lo)
        _touched(back[hi:], what, "behind", 0)
        if const:
            assert np.array_equal(back[lo:hi], sent), f"{what}: an input buffer was written"
        return back[lo:hi].view(np.float32).copy()

    check.base = base
    return base + lo, check


class Guards:
    def __init__(self, ctx):
        self.ctx, self.checks, self.pending, self.plain = ctx, {}, set(), []

    def buf(self, nfloats, shift, init=None, const=False):
        p, check = guarded(self.ctx, nfloats, shift, init, const)
        self.checks[p] = check
        self.pending.add(p)
        return p

    def inp(self, arr, shift):
        """A const input: its contents must survive the call."""
        arr = np.ascontiguousarray(arr, np.float32)
        return self.buf(arr.size, shift, arr, const=True)

    def image(self, arr):
        """Not a float buffer (images need no alignment and are covered elsewhere): a plain upload, freed with the rest."""
        p = self.ctx.to_device(np.ascontiguousarray(arr))
        self.plain.append(p)
        return p

    def check(self, p, shape, what=""):
        self.pending.discard(p)
        return self.checks[p](what).reshape(shape)

    def done(self, what=""):
        first = sys.exc_info()[1]                      # the test's own failure, if done() runs in its `finally`
        try:
            for p in sorted(self.pending):
                self.checks[p](f"{what}: a buffer the test did not read back")
        except AssertionError as e:
            if first is None:
                raise
            print(f"(also, while the failure above was on its way out) {e}")
            if hasattr(first, "add_note"):
                first.add_note(f"also: {e}")
        finally:
            self.free()

    def free(self):
        for check in self.checks.values():
            self.ctx.free(check.base)
        for p in self.plain:
            self.ctx.free(p)
        self.checks, self.pending, self.plain = {}, set(), []
