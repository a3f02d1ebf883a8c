"""The input format in the queue (csrc/ugsm_queue.cpp) on a machine without a GPU: the real queue source compiled against the recording
stand-in runtime (tests/fake_runtime.cpp) plus a setter for the context's format (tests/fake_input_format.cpp), driven through the C-ABI.

include/ugsm.h: the format is captured by ugsm_enqueue_* for the pair it enqueues, and pairs of different formats never share a call.  Here
every pair has the same mode, memory kind, size and stride, so the format is the only thing that can keep two pairs apart; the stride check
of ugsm_enqueue_* uses the format's bytes per pixel; and the host's setting is what it was once the queue has sent its calls."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, SIZE_MISMATCH, EMPTY = 0, 2, 9
RGB8, BGR8, RGBA8, BGRA8, MONO8 = 0, 1, 2, 3, 4
W, H = 64, 32
BASE = 0x7F0000000000  # made-up "device" addresses: the queue hands them on and never looks behind them


class Completion(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("status", C.c_int), ("slot", C.c_int), ("call_pairs", C.c_int), ("reserved", C.c_int),
                ("call_index", C.c_longlong), ("done_ns", C.c_longlong), ("result", C.POINTER(C.c_float) * 5)]


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakeqf") / "libugsm_queue_fake_fmt.so")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden",
           os.path.join(ROOT, "tests", "fake_runtime.cpp"), os.path.join(ROOT, "tests", "fake_input_format.cpp"),
           os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm_queue.cpp"),
           "-Wl,--version-script=" + os.path.join(ROOT, "ug_stereomatcher_amd", "csrc", "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = C.CDLL(out)
    vp, i, u64, ll = C.c_void_p, C.c_int, C.c_uint64, C.c_longlong
    lib.ugsm_fake_create.restype = vp
    lib.ugsm_fake_create.argtypes = [i, i, i, i]
    lib.ugsm_fake_destroy.argtypes = [vp]
    lib.ugsm_fake_destroy.restype = None
    lib.ugsm_fake_calls.argtypes = [vp]
    lib.ugsm_fake_calls.restype = ll
    lib.ugsm_fake_call.argtypes = [vp, ll, C.POINTER(i * 7), C.POINTER(vp * 16)]
    lib.ugsm_fake_violations.argtypes = [vp]
    lib.ugsm_fake_set_input_format.argtypes = [vp, i]
    lib.ugsm_fake_get_input_format.argtypes = [vp]
    lib.ugsm_enqueue_full.argtypes = [vp, vp, vp, i, i, i, vp, u64]
    lib.ugsm_enqueue_full_managed.argtypes = [vp, vp, vp, i, i, i, u64]
    lib.ugsm_next_done.argtypes = [vp, C.POINTER(Completion), i]
    return lib


def _calls(fq, ctx):
    """The pairs (tags) of every call the queue made, in order."""
    out = []
    for k in range(fq.ugsm_fake_calls(ctx)):
        v, L = (C.c_int * 7)(), (C.c_void_p * 16)()
        assert fq.ugsm_fake_call(ctx, k, C.byref(v), C.byref(L)) == 0
        out.append([(L[b] - BASE) // 4096 for b in range(v[1])])
    return out


def _fetch(fq, ctx, block, tags):
    """Completions into `tags`: every outstanding one (block) or those already finished (at most (slots + 1) x batch may be outstanding)."""
    while True:
        c = Completion()
        st = fq.ugsm_next_done(ctx, C.byref(c), 1 if block else 0)
        if st == EMPTY or (not block and st == 8):  # (UGSM_PENDING)
            return tags
        assert st == OK and c.status == OK, (st, c.status)
        tags.append(int(c.tag))


def _drain(fq, ctx, tags=None):
    return _fetch(fq, ctx, True, [] if tags is None else tags)


@pytest.mark.parametrize("slots,batch", [(2, 4), (1, 8), (4, 3)])
def test_pairs_that_differ_only_in_format_never_share_a_call(fq, slots, batch):
    order = [RGB8, RGB8, BGR8, BGR8, RGB8, MONO8, MONO8, MONO8, RGBA8, BGRA8, BGRA8, RGB8, BGR8, RGB8, RGB8, RGB8]
    ctx = fq.ugsm_fake_create(slots, batch, 8, 4)
    try:
        done = []
        for tag, fmt in enumerate(order):
            assert fq.ugsm_fake_set_input_format(ctx, fmt) == OK
            p = BASE + 4096 * tag
            assert fq.ugsm_enqueue_full(ctx, p, p + 1, W, H, 4 * W, p + 2, tag) == OK
            _fetch(fq, ctx, False, done)
        assert fq.ugsm_fake_set_input_format(ctx, MONO8) == OK
        assert _drain(fq, ctx, done) == list(range(len(order)))
        calls = _calls(fq, ctx)
        assert sorted(t for c in calls for t in c) == list(range(len(order)))
        for c in calls:
            assert len({order[t] for t in c}) == 1, (calls, [[order[t] for t in c] for c in calls])
        assert max(len(c) for c in calls) > 1  # (pairs of one format do share calls)
        # the host's own setting is left as it set it, whatever the queue's calls were sent with
        assert fq.ugsm_fake_get_input_format(ctx) == MONO8
        assert fq.ugsm_fake_violations(ctx) == 0
    finally:
        fq.ugsm_fake_destroy(ctx)


def test_enqueue_checks_the_stride_against_the_format(fq):
    ctx = fq.ugsm_fake_create(2, 4, 8, 4)
    try:
        p = BASE
        for fmt, bpp in ((RGB8, 3), (BGR8, 3), (RGBA8, 4), (BGRA8, 4), (MONO8, 1)):
            assert fq.ugsm_fake_set_input_format(ctx, fmt) == OK
            assert fq.ugsm_enqueue_full(ctx, p, p + 1, W, H, bpp * W - 1, p + 2, 0) == SIZE_MISMATCH, fmt
        assert fq.ugsm_fake_set_input_format(ctx, MONO8) == OK
        assert fq.ugsm_enqueue_full(ctx, p, p + 1, W, H, W, p + 2, 7) == OK  # (a stride of W bytes is enough for mono8 ...)
        assert _drain(fq, ctx) == [7]
        assert fq.ugsm_fake_set_input_format(ctx, RGB8) == OK
        assert fq.ugsm_enqueue_full(ctx, p, p + 1, W, H, W, p + 2, 8) == SIZE_MISMATCH  # (... and not for rgb8)
    finally:
        fq.ugsm_fake_destroy(ctx)
