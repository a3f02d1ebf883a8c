"""The queue of include/ugsm.h (csrc/ugsm_queue.cpp) on a machine without a GPU: the real queue source compiled against a recording
stand-in for the runtime (tests/fake_runtime.cpp -- test infrastructure) and driven through the C-ABI with ctypes.

The queue is host logic written against the public slot-level entry points; what it promises is stated in the header:
  * UGSM_OK from ugsm_enqueue_* = the pair is accepted and is reported by ugsm_next_done EXACTLY ONCE, in enqueue order, with the status
    of the library call it went out in; anything else = rejected, never reported;
  * a failed call's pairs are reported only after the slot has drained;
  * calls hold pairs of one kind, at most `batch` of them, the first `slots` calls of a burst staggered (ugsm_queue_plan);
  * no slot is given a second call before its first has been seen finished;
  * the `more` hint (CtxHooks::queue_more) that makes the runtime take a call to share the chip: set when pairs wait behind the call or
    the call filled up by itself, clear for a flushed call with nothing behind it;
  * nothing is thrown across the C-ABI: with the Nth host allocation failing, entry points answer UGSM_ERR_NOMEM and the first rule
    still holds;
  * a call carries exactly the arguments its pairs were enqueued with, at the right slot-level entry point (test_marshalling: the fake
    records everything a ugsm_submit_* stand-in is handed; the cloud kinds and every refusal of the ten entry points: test_queue_cloud_host.py).
The reference has no counterpart (one blocking match() per callback, UG_GPU_matcher.cpp:126-185, 749-752)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, NOMEM, STATE, PENDING, EMPTY = 0, 1, 6, 7, 8, 9


class Completion(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("status", C.c_int), ("slot", C.c_int), ("call_pairs", C.c_int), ("reserved", C.c_int),
                ("call_index", C.c_longlong), ("done_ns", C.c_longlong), ("result", C.POINTER(C.c_float) * 5)]


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fakeq") / "libugsm_queue_fake.so")
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
    lib.ugsm_fake_poll_delay.argtypes = [vp, i]
    lib.ugsm_fake_poll_delay.restype = None
    lib.ugsm_fake_fail_call.argtypes = [vp, ll, i]
    lib.ugsm_fake_calls.argtypes = [vp]
    lib.ugsm_fake_calls.restype = ll
    lib.ugsm_fake_call.argtypes = [vp, ll, C.POINTER(i * 7), C.POINTER(vp * 16)]
    lib.ugsm_fake_call_args.argtypes = [vp, ll, C.POINTER(ll * 7), C.POINTER(ll * (9 * 16))]
    lib.ugsm_fake_set_input_format.argtypes = [vp, i]
    lib.ugsm_fake_get_input_format.argtypes = [vp]
    lib.ugsm_fake_violations.argtypes = [vp]
    lib.ugsm_fake_fail_alloc_after.argtypes = [ll]
    lib.ugsm_fake_fail_alloc_after.restype = None
    lib.ugsm_fake_allocs.restype = ll
    lib.ugsm_enqueue_full.argtypes = [vp, vp, vp, i, i, i, vp, u64]
    lib.ugsm_enqueue_foveated.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, u64]
    lib.ugsm_enqueue_full_host.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, u64]
    lib.ugsm_enqueue_foveated_host.argtypes = [vp, vp, vp, i, i, i, i, i, vp, vp, vp, vp, vp, u64]
    lib.ugsm_enqueue_full_managed.argtypes = [vp, vp, vp, i, i, i, u64]
    lib.ugsm_enqueue_foveated_managed.argtypes = [vp, vp, vp, i, i, i, i, i, i, u64]
    lib.ugsm_flush.argtypes = [vp]
    lib.ugsm_next_done.argtypes = [vp, C.POINTER(Completion), i]
    lib.ugsm_queue_depth.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ugsm_queue_plan.argtypes = [vp, i, C.POINTER(i), i]
    lib.ugsm_last_error.argtypes = [vp]
    lib.ugsm_last_error.restype = C.c_char_p
    return lib


BASE = 0x7F0000000000   # made-up "device" addresses: the queue hands them on and never looks behind them


def ptr_of(tag):
    return BASE + 4096 * tag


class Host:
    """A host program on the queue; keeps the books the assertions need."""

    def __init__(self, lib, slots, batch, poll_delay=0):
        self.lib, self.slots, self.batch = lib, slots, max(1, batch)
        self.ctx = lib.ugsm_fake_create(slots, batch, 8, 4)
        assert self.ctx
        lib.ugsm_fake_poll_delay(self.ctx, poll_delay)
        self.accepted, self.kind_of, self.reported, self.rejected = [], {}, [], []
        self.next_tag = 0
        self.img = np.zeros((2, 16, 3 * 32), np.uint8)   # a 32 x 16 rgb8 pair for the managed entry point (it copies the images)

    def close(self):
        self.lib.ugsm_fake_destroy(self.ctx)
        self.ctx = None

    def outstanding(self):
        return len(self.accepted) - len(self.reported)

    def enqueue(self, kind, size=(64, 32)):
        tag = self.next_tag
        self.next_tag += 1
        W, H = size
        p = ptr_of(tag)
        if kind == "full":
            st = self.lib.ugsm_enqueue_full(self.ctx, p, p + 1, W, H, 3 * W, p + 2, tag)
        elif kind == "fovea":
            st = self.lib.ugsm_enqueue_foveated(self.ctx, p, p + 1, W, H, 3 * W, 0, 0, p + 2, None, None, tag)
        elif kind == "host":
            st = self.lib.ugsm_enqueue_full_host(self.ctx, p, p + 1, W, H, 3 * W, p + 2, p + 3, p + 4, tag)
        else:
            st = self.lib.ugsm_enqueue_full_managed(self.ctx, self.img[0].ctypes.data, self.img[1].ctypes.data, 32, 16, 96, tag)
        if st == OK:
            self.accepted.append(tag)
            self.kind_of[tag] = (kind, size if kind != "managed" else (32, 16))
        else:
            self.rejected.append((tag, st))
        return st

    def call(self, k):
        v, L = (C.c_int * 7)(), (C.c_void_p * 16)()
        assert self.lib.ugsm_fake_call(self.ctx, k, C.byref(v), C.byref(L)) == 0, k
        return dict(slot=v[0], n=v[1], mode=v[2], mem=v[3], status=v[4], more=v[5], drained=v[6], L=[L[b] for b in range(v[1])])

    def calls(self):
        return [self.call(k) for k in range(self.lib.ugsm_fake_calls(self.ctx))]

    def next_done(self, block):
        c = Completion()
        st = self.lib.ugsm_next_done(self.ctx, C.byref(c), block)
        if st == OK:
            rec = self.call(c.call_index)
            # reported only once its slot has been seen finished -- a failed call too ("a completion always means the buffers are free")
            assert rec["drained"] == 1, (c.tag, rec)
            assert c.status == rec["status"] and c.call_pairs == rec["n"] and c.slot == rec["slot"], (c.tag, c.status, rec)
            self.reported.append(c.tag)
            if self.kind_of[c.tag][0] == "managed":
                assert c.result[0] and c.result[1] and c.result[2]          # the planes the library lends
            else:
                assert not c.result[0]
        return st

    def drain(self, tolerate=False):
        spins = 0
        while True:
            st = self.next_done(1)
            if st == EMPTY:
                return
            if st != OK:
                assert tolerate and st == NOMEM, (st, self.lib.ugsm_last_error(self.ctx))
                spins += 1
                assert spins < 50, "ugsm_next_done keeps failing"

    def check(self, faults=False):
        """The invariants, after a drain."""
        assert self.reported == self.accepted, (self.reported, self.accepted)            # exactly once, in enqueue order
        assert self.lib.ugsm_fake_violations(self.ctx) == 0                               # no slot reused before it was seen finished
        sent = []
        for rec in self.calls():
            assert 1 <= rec["n"] <= self.batch, rec
            tags = [(p - BASE) // 4096 if p and p >= BASE else None for p in rec["L"]]
            kinds = set()
            for t, p in zip(tags, rec["L"]):
                if t is None or t not in self.kind_of or self.kind_of[t][0] == "managed":
                    kinds.add("managed")            # (staged by the library: not the host's pointer)
                else:
                    kinds.add(self.kind_of[t])
                    sent.append(t)
            assert len(kinds) == 1, (rec, kinds)                                          # one kind per call
            assert rec["mode"] == (1 if next(iter(kinds))[0] == "fovea" else 0) if "managed" not in kinds else True
        plain = [t for t in self.accepted if self.kind_of[t][0] != "managed"]
        if not faults:
            assert sent == plain, (sent, plain)                                           # every pair went out once, in order
        else:
            assert sorted(set(sent)) == sorted(sent) and set(plain) <= set(sent)
        w, f, u = C.c_int(), C.c_int(), C.c_int()
        assert self.lib.ugsm_queue_depth(self.ctx, C.byref(w), C.byref(f), C.byref(u)) == OK and (w.value, f.value, u.value) == (0, 0, 0)


def plan(lib, slots, batch, n):
    """ugsm_queue_plan: what the header says a burst of n pairs becomes."""
    class Config(C.Structure):   # ugsm_config (include/ugsm.h; the layout is pinned against the header by tests/test_abi_host.py through _lib.Config)
        _fields_ = [(n, C.c_float if n in ("early_exit_threshold", "lr_check_threshold") else C.c_int) for n in (
            "device", "levels", "fovea_levels", "slots", "kernel_path", "profile_events", "march_min_pixels", "march_np", "march_rows", "march_smooth",
            "early_exit_threshold", "small_max_pixels", "lr_check_threshold", "streams", "batch", "stream_priority")]
    cfg = Config()
    cfg.slots, cfg.batch, cfg.levels, cfg.fovea_levels = slots, batch, 8, 4
    sizes = (C.c_int * 64)()
    k = lib.ugsm_queue_plan(C.byref(cfg), n, sizes, 64)
    return [sizes[i] for i in range(k)]


def test_a_burst_is_staggered_and_hinted(fq):
    """Four slots, calls of up to eight, 32 pairs enqueued back to back from idle while nothing finishes: calls of 4, 5, 7, 8, then the
    enqueue that fills the fifth call waits for the oldest call's slot (back-pressure) and sends 8.  Every call of the burst carries the
    `more` hint (it filled up by itself: a host that submits faster than the chip matches)."""
    h = Host(fq, 4, 8, poll_delay=10 ** 6)
    try:
        for _ in range(32):
            assert h.enqueue("full") == OK
        calls = h.calls()
        assert [c["n"] for c in calls] == [4, 5, 7, 8, 8] == plan(fq, 4, 8, 32), calls
        assert [c["slot"] for c in calls] == [0, 1, 2, 3, 0]
        assert all(c["more"] == 1 for c in calls)
        assert h.next_done(0) == OK and h.reported == [0]          # (the back-pressure wait retired call 0: its pairs are ready)
        assert fq.ugsm_flush(h.ctx) == OK
        h.drain()
        h.check()
    finally:
        h.close()


def test_a_flushed_call_with_nothing_behind_it_is_taken_to_be_alone(fq):
    """The hint the kernel policy reads (call_alone, csrc/ugsm_policy.cpp): clear for one pair enqueued and flushed (the node's topic path when
    frames arrive slower than they are matched), for a partial call sent by a blocking ugsm_next_done, and for the LAST call of a burst;
    set for a call that leaves pairs waiting (here: a pair of another size behind it)."""
    h = Host(fq, 4, 8)
    try:
        assert h.enqueue("full") == OK and fq.ugsm_flush(h.ctx) == OK
        assert [(c["n"], c["more"]) for c in h.calls()] == [(1, 0)]
        h.drain()
        assert h.enqueue("full") == OK and h.enqueue("full") == OK
        assert fq.ugsm_fake_calls(h.ctx) == 1                      # two pairs of a call of four (the stagger restarts after a flush): they wait
        assert h.next_done(1) == OK                                 # ... until a blocking fetch sends them
        assert [(c["n"], c["more"]) for c in h.calls()][1:] == [(2, 0)]
        h.drain()
        assert h.enqueue("full") == OK and h.enqueue("full") == OK and h.enqueue("full", (128, 64)) == OK
        got = [(c["n"], c["more"]) for c in h.calls()][2:]
        assert got == [(2, 1)], got                                 # the pair of another size closes the group: it goes out, hinted
        assert fq.ugsm_flush(h.ctx) == OK
        assert [(c["n"], c["more"]) for c in h.calls()][3:] == [(1, 0)]
        h.drain()
        h.check()
    finally:
        h.close()


def test_the_queue_refuses_instead_of_recycling_unfetched_results(fq):
    """(slots + 1) x batch pairs outstanding with completions unfetched: UGSM_ERR_STATE, nothing enqueued, and room again after a fetch."""
    h = Host(fq, 2, 2)
    try:
        sts = [h.enqueue("full") for _ in range(8)]
        assert sts[:6] == [OK] * 6 and set(sts[6:]) == {STATE}, sts
        assert h.next_done(1) == OK
        assert h.enqueue("full") == OK
        h.drain()
        h.check()
        assert [t for t, _ in h.rejected] == [6, 7]
    finally:
        h.close()


@pytest.mark.parametrize("seed", range(24))
def test_every_accepted_pair_is_reported_exactly_once_in_order(fq, seed):
    """Random host programs (four kinds of pairs, two sizes, flushes, blocking and non-blocking fetches) on random contexts, with slots
    that take a random number of queries to finish and a random tenth of the library calls failing: the books balance."""
    rnd = random.Random(1000 + seed)
    slots, batch = rnd.choice([1, 2, 4]), rnd.choice([1, 2, 3, 8])
    h = Host(fq, slots, batch, poll_delay=rnd.choice([0, 1, 3, 7]))
    try:
        for k in range(400):
            if rnd.random() < 0.1:
                fq.ugsm_fake_fail_call(h.ctx, k, rnd.choice([5, 6]))
        for _ in range(rnd.randrange(50, 300)):
            r = rnd.random()
            if r < 0.6:
                st = h.enqueue(rnd.choice(["full", "full", "fovea", "host", "managed"]), rnd.choice([(64, 32), (64, 32), (128, 64)]))
                assert st == OK or (st == STATE and h.outstanding() >= (slots + 1) * h.batch), (st, h.outstanding())
            elif r < 0.7:
                assert fq.ugsm_flush(h.ctx) == OK
            elif r < 0.95:
                assert h.next_done(0) in (OK, PENDING, EMPTY)
            else:
                assert h.next_done(1) in (OK, EMPTY)
        h.drain()
        h.check()
    finally:
        h.close()


def scenario(h):
    """40 pairs of four kinds and two sizes, fetched as they finish (the books never fill up: no UGSM_ERR_STATE), then a flush."""
    kinds = [("full", (64, 32))] * 7 + [("managed", None)] * 5 + [("fovea", (64, 32))] * 6 + [("host", (128, 64))] * 3 + [("full", (128, 64))] * 4
    for kind, size in kinds + kinds[:15]:
        h.enqueue(kind, size or (32, 16))
        for _ in range(2):
            if h.next_done(0) not in (OK,):
                break
    h.lib.ugsm_flush(h.ctx)


def test_host_allocation_failures_lose_no_pair(fq):
    """Nothing is thrown across the C-ABI and nothing is lost: the same host program with the 1st, 2nd, 3rd ... host allocation inside the
    library failing.  An entry point may then answer UGSM_ERR_NOMEM (an enqueue: the pair is rejected; a fetch: ask again); every pair whose
    enqueue answered UGSM_OK is still reported exactly once, in order, and no slot is reused early."""
    h = Host(fq, 2, 3, poll_delay=1)
    a0 = fq.ugsm_fake_allocs()
    scenario(h)
    h.drain()
    h.check()
    n_allocs = fq.ugsm_fake_allocs() - a0
    h.close()
    assert n_allocs > 10, n_allocs
    refused = fetch_failed = 0
    for k in range(n_allocs + 2):
        h = Host(fq, 2, 3, poll_delay=1)
        try:
            fq.ugsm_fake_fail_alloc_after(k)
            scenario(h)
            before = len(h.reported)
            h.drain(tolerate=True)
            fq.ugsm_fake_fail_alloc_after(-1)
            h.check(faults=True)
            assert all(st in (NOMEM, STATE) for _, st in h.rejected), h.rejected
            refused += any(st == NOMEM for _, st in h.rejected)
            fetch_failed += len(h.accepted) == 40 and not h.rejected and before < 40
        finally:
            h.close()
    assert refused > 3, (refused, fetch_failed)     # (the faults do land: some in an enqueue, which then refuses its pair)


# ---- what a call carries: every argument of every pair ---------------------------------------------------------------------------------
E_BATCH, E_FOVEA, E_HOST = 1, 2, 4          # which ugsm_submit_* stand-in a call went to (tests/fake_runtime.cpp)
RGB8, RGBA8, MONO8 = 0, 2, 4
BPP = {RGB8: 3, RGBA8: 4, MONO8: 1}
FOVEA_LEVELS = 4


class Marshal:
    """A host whose every pointer argument and offset is distinct per pair; keeps what each pair was enqueued with and, for the managed
    kinds, what its staging held when the pair was reported."""

    def __init__(self, lib):
        self.lib = lib
        self.ctx = lib.ugsm_fake_create(2, 3, 8, FOVEA_LEVELS)
        assert self.ctx
        self.fmt = RGB8
        self.want, self.images, self.done, self.staged = {}, {}, [], {}

    def close(self):
        self.lib.ugsm_fake_destroy(self.ctx)

    def set_format(self, fmt):
        assert self.lib.ugsm_fake_set_input_format(self.ctx, fmt) == OK
        self.fmt = fmt

    def enqueue(self, kind, pyr="", size=(64, 32), stride=None):
        """kind: full, fovea, full_host, fovea_host, full_managed, fovea_managed; pyr: which pyramid stacks the pair asks for ("", "L", "LR")."""
        lib, ctx, tag = self.lib, self.ctx, len(self.want)
        W, H = size
        row = BPP[self.fmt] * W
        stride = row + 8 if stride is None else stride
        p = BASE + 4096 * tag
        L, R, o0, o1, o2 = (p + 64 * k for k in range(5))
        pl, pr = (p + 320 if "L" in pyr else None), (p + 384 if "R" in pyr else None)
        ox, oy = 3 + tag, 1000 + tag
        w = dict(kind=kind, pyr=pyr, fovea=kind.startswith("fovea"), host=not kind in ("full", "fovea"), managed=kind.endswith("managed"),
                 W=W, H=H, stride=stride, fmt=self.fmt, L=L, R=R, ox=0, oy=0)
        if w["fovea"]:
            w["ox"], w["oy"] = ox, oy
        if kind == "full":
            st, w["out"] = lib.ugsm_enqueue_full(ctx, L, R, W, H, stride, o0, tag), [o0, 0, 0, 0, 0]
        elif kind == "fovea":
            st, w["out"] = lib.ugsm_enqueue_foveated(ctx, L, R, W, H, stride, ox, oy, o0, pl, pr, tag), [o0, 0, 0, pl or 0, pr or 0]
        elif kind == "full_host":
            st, w["out"] = lib.ugsm_enqueue_full_host(ctx, L, R, W, H, stride, o0, o1, o2, tag), [o0, o1, o2, 0, 0]
        elif kind == "fovea_host":
            st = lib.ugsm_enqueue_foveated_host(ctx, L, R, W, H, stride, ox, oy, o0, o1, o2, pl, pr, tag)
            w["out"] = [o0, o1, o2, pl or 0, pr or 0]
        else:
            img = np.random.RandomState(tag).randint(0, 256, (2, H, stride)).astype(np.uint8)   # any memory: the library copies the images
            self.images[tag] = [img[s][:, :row].tobytes() for s in range(2)]                    # ... compacted to rows of bytes per pixel x W
            w["stride"] = row
            if kind == "full_managed":
                assert pyr == ""
                st = lib.ugsm_enqueue_full_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, W, H, stride, tag)
            else:
                assert pyr in ("", "LR")
                st = lib.ugsm_enqueue_foveated_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, W, H, stride, ox, oy, 1 if pyr else 0, tag)
            img[:] = 0                                                                          # (the caller's memory is not read again)
        assert st == OK, (kind, st, lib.ugsm_last_error(ctx))
        self.want[tag] = w
        return tag

    def args(self, k):
        head, pairs = (C.c_longlong * 7)(), (C.c_longlong * (9 * 16))()
        assert self.lib.ugsm_fake_call_args(self.ctx, k, C.byref(head), C.byref(pairs)) == 0, k
        rec = dict(zip(("entry", "W", "H", "stride", "fmt", "pyr_arrays", "n"), head))
        rec["pairs"] = [dict(L=pairs[9 * b], R=pairs[9 * b + 1], ox=pairs[9 * b + 2], oy=pairs[9 * b + 3], out=list(pairs[9 * b + 4:9 * b + 9]))
                        for b in range(rec["n"])]
        return rec

    def drain(self):
        while True:
            c = Completion()
            st = self.lib.ugsm_next_done(self.ctx, C.byref(c), 1)
            if st == EMPTY:
                return
            assert st == OK and c.status == OK, (st, c.status)
            tag, k = int(c.tag), int(c.call_index)
            b = sum(1 for _, kk, _ in self.done if kk == k)          # the pair's place in its call: pairs are reported in enqueue order
            self.done.append((tag, k, [C.cast(c.result[j], C.c_void_p).value or 0 for j in range(5)]))
            w = self.want[tag]
            if w["managed"]:                                         # the staging is lent until the next ugsm_next_done: look now
                pr = self.args(k)["pairs"][b]
                nbytes = w["stride"] * w["H"]
                self.staged[tag] = [C.string_at(pr["L"], nbytes), C.string_at(pr["R"], nbytes)]


def test_marshalling(fq):
    """Every recorded call carries exactly the arguments its pairs were enqueued with, in enqueue order, at the right one of the eight
    ugsm_submit_* entry points: two slots, calls of up to three, every non-cloud kind in calls of one pair and of several, kind changes in
    the backlog, host pairs with pyramid stacks going out alone, strides larger than a row, a format change between two enqueues."""
    m = Marshal(fq)
    try:
        # (the first call after idle or a flush takes two pairs, the later ones three: ugsm_queue_plan)
        m.enqueue("full"), m.enqueue("full")                                        # a call of two
        m.enqueue("full"), m.enqueue("fovea")                                       # another kind behind it: the full pair goes out alone
        m.enqueue("fovea"), m.enqueue("fovea", "LR")                                # three foveated pairs, one with pyramids
        m.drain()
        m.enqueue("fovea", "L"), m.drain()                                          # one pair, its left pyramid only
        m.enqueue("fovea"), m.enqueue("fovea")                                      # two without: no pyramid arrays
        m.enqueue("fovea"), m.drain()
        m.enqueue("full_host"), m.enqueue("full_host")
        m.enqueue("full_host"), m.enqueue("fovea_host")
        m.enqueue("fovea_host"), m.enqueue("fovea_host", "L")                       # pyramid stacks: ends the group and goes out alone
        m.drain()
        m.enqueue("fovea_host", "LR"), m.enqueue("fovea_host"), m.drain()
        m.enqueue("full_managed"), m.enqueue("full_managed", stride=3 * 64)          # (one with rows that need no compaction)
        m.enqueue("full_managed"), m.drain()
        m.enqueue("fovea_managed"), m.enqueue("fovea_managed")
        m.enqueue("fovea_managed", "LR")
        m.enqueue("fovea_managed"), m.drain()
        m.enqueue("full", size=(64, 32), stride=4 * 64 + 8), m.enqueue("full", size=(128, 64)), m.drain()   # another size
        a = m.enqueue("full", stride=4 * 64 + 8)
        m.set_format(RGBA8)
        b = m.enqueue("full", stride=4 * 64 + 8)                                    # differs from `a` in nothing but the format
        c = m.enqueue("full_managed")
        m.set_format(MONO8)                                                         # what the host sets later does not reach pairs already enqueued
        m.drain()
        assert fq.ugsm_fake_get_input_format(m.ctx) == MONO8
        assert fq.ugsm_fake_violations(m.ctx) == 0

        want = m.want
        assert [t for t, _, _ in m.done] == list(range(len(want)))                  # exactly once, in enqueue order
        ncalls = fq.ugsm_fake_calls(m.ctx)
        assert sorted({k for _, k, _ in m.done}) == list(range(ncalls))
        seen = set()
        for k in range(ncalls):
            rec = m.args(k)
            tags = [t for t, kk, _ in m.done if kk == k]
            results = [r for _, kk, r in m.done if kk == k]
            n, w0 = rec["n"], want[tags[0]]
            assert n == len(tags) and tags == list(range(tags[0], tags[0] + n)), (k, rec, tags)
            assert rec["entry"] == (E_FOVEA if w0["fovea"] else 0) + (E_HOST if w0["host"] else 0) + (E_BATCH if n > 1 else 0), (k, rec, w0)
            assert rec["pyr_arrays"] == (1 if rec["entry"] == E_FOVEA + E_BATCH and any(want[t]["pyr"] for t in tags) else 0), (k, rec)
            for t, got, res in zip(tags, rec["pairs"], results):
                w = want[t]
                assert (rec["W"], rec["H"], rec["stride"], rec["fmt"]) == (w["W"], w["H"], w["stride"], w["fmt"]), (k, t, rec, w)
                assert (got["ox"], got["oy"]) == (w["ox"], w["oy"]), (k, t, got, w)
                if not w["managed"]:
                    assert (got["L"], got["R"], got["out"]) == (w["L"], w["R"], w["out"]), (k, t, got, w)
                    assert res == [0] * 5, (t, res)
                else:
                    # the staging buffer's carve-up: both images, 256-byte aligned; three planes, then the two pyramid stacks of three planes each
                    img = (w["stride"] * w["H"] + 255) & ~255
                    plane = (FOVEA_LEVELS * (w["W"] // 8) * (w["H"] // 8) if w["fovea"] else w["W"] * w["H"]) * 4
                    o0 = got["out"][0]
                    assert got["L"] and o0 and got["R"] == got["L"] + img, (k, t, got)
                    assert got["out"] == [o0, o0 + plane, o0 + 2 * plane, o0 + 3 * plane if w["pyr"] else 0, o0 + 6 * plane if w["pyr"] else 0], (k, t, got)
                    assert res == got["out"], (t, res, got)
                    assert m.staged[t] == m.images[t], (k, t)
                seen.add((w["kind"], w["pyr"], n > 1))
            if w0["managed"]:
                assert len({g["L"] for g in rec["pairs"]}) == n and len({g["out"][0] for g in rec["pairs"]}) == n      # a buffer per pair
        # the format each of the last three pairs was enqueued in, alone in its call
        assert [(want[t]["fmt"], sum(1 for _, kk, _ in m.done if kk == m.done[t][1])) for t in (a, b, c)] == [(RGB8, 1), (RGBA8, 1), (RGBA8, 1)]
        both = lambda kind, pyr="": {(kind, pyr, False), (kind, pyr, True)}
        need = (both("full") | both("fovea") | {("fovea", "LR", True), ("fovea", "L", False)} | both("full_host") | both("fovea_host")
                | {("fovea_host", "L", False), ("fovea_host", "LR", False)} | both("full_managed") | both("fovea_managed") | {("fovea_managed", "LR", False)})
        assert seen == need, (sorted(seen ^ need))
        assert {m.args(k)["entry"] for k in range(ncalls)} == set(range(8))         # all eight entry points
    finally:
        m.close()
