"""tests/guarded.py on a stand-in for the device (no GPU): the guard must notice one byte written in front of a buffer, one behind it and one
inside a const input, and must leave a call that stays inside its floats alone."""
import numpy as np
import pytest

from guarded import GUARD, POISON, SHIFTS, Guards, guarded


class HostCtx:
    """to_device / to_host / free of _lib.Context over host memory; a "device pointer" is the address of a numpy buffer kept alive here."""

    def __init__(self, misalign=0):
        self.mem, self.misalign = {}, misalign

    def to_device(self, arr):
        src = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        room = np.empty(src.size + 32, np.uint8)       # a 16-byte aligned base (or `misalign` bytes past one), as a device allocator gives
        at = (-room.ctypes.data) % 16 + self.misalign
        buf = room[at:at + src.size]
        buf[:] = src
        self.mem[buf.ctypes.data] = buf
        return buf.ctypes.data

    def to_host(self, ptr, shape, dtype=np.float32):
        return self.mem[ptr][:int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy()

    def free(self, ptr):
        del self.mem[ptr]

    def poke(self, addr, value=0):
        """One byte at an absolute address inside any live allocation."""
        for base, buf in self.mem.items():
            if base <= addr < base + buf.size:
                buf[addr - base] = value
                return
        raise AssertionError("outside every allocation")


@pytest.mark.parametrize("shift", SHIFTS)
def test_payload_address_and_round_trip(shift):
    ctx = HostCtx()
    init = np.arange(10, dtype=np.float32)
    p, check = guarded(ctx, 10, shift, init)
    assert p == check.base + 4 * (GUARD + shift) and (p - check.base) % 16 == 4 * shift
    assert (ctx.mem[check.base][:4 * (GUARD + shift)] == POISON).all() and ctx.mem[check.base].size == 4 * (2 * GUARD + shift + 10)
    assert np.array_equal(check("untouched"), init)
    ctx.poke(p + 4, 0x7F)                            # inside the payload of an output: allowed
    assert check("written inside")[1] != init[1]


@pytest.mark.parametrize("where,offset", [("in front of", -1), ("in front of", -4 * (GUARD + 1)), ("behind", 40), ("behind", 40 + 4 * GUARD - 1)])
def test_a_byte_outside_the_payload_is_noticed(where, offset):
    ctx = HostCtx()
    p, check = guarded(ctx, 10, 1)
    ctx.poke(p + offset)
    with pytest.raises(AssertionError, match=f"guard: 1 bytes {where} the buffer"):
        check("case")


def test_a_written_input_is_noticed_and_done_checks_what_was_not_read_back():
    ctx = HostCtx()
    g = Guards(ctx)
    a, b = g.inp(np.ones(8, np.float32), 2), g.buf(8, 3)
    assert np.array_equal(g.check(b, (8,)).view(np.uint8), np.full(32, POISON, np.uint8))
    ctx.poke(a + 5, 0x7F)
    with pytest.raises(AssertionError, match="an input buffer was written"):
        g.done("call")
    assert not ctx.mem, "done() frees every buffer, also when a check fails"


def test_a_base_that_is_not_16_byte_aligned_is_refused():
    with pytest.raises(AssertionError, match="not 16-byte aligned"):
        guarded(HostCtx(misalign=4), 10, 0)


def test_done_in_a_finally_keeps_the_first_failure(capsys):
    ctx = HostCtx()
    g = Guards(ctx)
    a = g.inp(np.ones(8, np.float32), 1)
    ctx.poke(a - 1)
    with pytest.raises(AssertionError, match="the value assertion of the test"):
        try:
            raise AssertionError("the value assertion of the test")
        finally:
            g.done("call")
    assert "guard: 1 bytes in front of the buffer" in capsys.readouterr().out and not ctx.mem
