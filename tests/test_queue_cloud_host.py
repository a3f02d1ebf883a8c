"""The cloud forms of the queue (ugsm_enqueue_*_cloud*, ugsm_done_cloud; include/ugsm.h, "the cloud from the queue") on a machine without
a GPU: the real csrc/ugsm_queue.cpp compiled against tests/fake_runtime_cloud.cpp -- tests/fake_runtime.cpp plus the two hooks through which
the queue reaches the runtime's cloud work, recorded -- and driven through the C-ABI with ctypes.

What the header promises and this file checks:
  * pairs of one call share a byte-equal spec; a pair with another spec, or without a cloud, ends the group like a pair of another kind;
  * the stagger and ugsm_queue_plan's sizes are what they are for plain pairs;
  * a managed cloud call completes in two steps: the finish hook runs exactly once, after the slot was first seen idle; the pairs are
    reported after the second drain, in enqueue order -- also when a later call finishes first;
  * ugsm_done_cloud gives the cloud of the pair just reported and UGSM_ERR_STATE otherwise; the staging is not handed on before the next
    ugsm_next_done;
  * a failed submit or finish hook reports every pair of the call once with that status; host allocation failures lose no pair;
  * bad arguments are rejected and leave the queue as it was -- for all ten ugsm_enqueue_*, every refusal with its status, its exact
    message and its place in the order of the refusals;
  * the hook receives every CloudJob field of every pair as it was enqueued, and the spec with `reserved` cleared;
  * the queue has no link-time dependency on the cloud work: it still builds and loads (RTLD_NOW) against tests/fake_runtime.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, DEVICE, NOMEM, STATE, PENDING, EMPTY = 0, 1, 5, 6, 7, 8, 9
CSRC = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")


class Completion(C.Structure):
    _fields_ = [("tag", C.c_uint64), ("status", C.c_int), ("slot", C.c_int), ("call_pairs", C.c_int), ("reserved", C.c_int),
                ("call_index", C.c_longlong), ("done_ns", C.c_longlong), ("result", C.POINTER(C.c_float) * 5)]


class CloudParams(C.Structure):
    _fields_ = [("sampling", C.c_int), ("format", C.c_int), ("compact", C.c_int), ("min_conf", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float)]


class QueueCloud(C.Structure):
    _fields_ = [("P1", C.c_double * 12), ("P2", C.c_double * 12), ("params", CloudParams), ("max_points", C.c_longlong), ("want_planes", C.c_int),
                ("reserved", C.c_int)]


class CloudResult(C.Structure):
    _fields_ = [("points", C.c_void_p), ("count", C.c_longlong), ("stored", C.c_longlong), ("point_step", C.c_int), ("levels", C.c_int),
                ("level_counts", C.c_longlong * 32)]


def build(tmp, fake):
    out = str(tmp / ("lib_" + fake.replace(".cpp", "") + ".so"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden", os.path.join(ROOT, "tests", fake),
           os.path.join(CSRC, "ugsm_queue.cpp"), "-Wl,--version-script=" + os.path.join(CSRC, "ugsm.map"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    lib = C.CDLL(build(tmp_path_factory.mktemp("fakeqc"), "fake_runtime_cloud.cpp"))
    vp, i, u64, ll = C.c_void_p, C.c_int, C.c_uint64, C.c_longlong
    qc = C.POINTER(QueueCloud)
    lib.ugsm_fake_create_cloud.restype = vp
    lib.ugsm_fake_create_cloud.argtypes = [i, i, i, i, i]
    lib.ugsm_fake_destroy_cloud.argtypes = [vp]
    lib.ugsm_fake_destroy_cloud.restype = None
    lib.ugsm_fake_poll_delay.argtypes = [vp, i]
    lib.ugsm_fake_poll_delay.restype = None
    lib.ugsm_fake_fail_call.argtypes = [vp, ll, i]
    lib.ugsm_fake_fail_finish.argtypes = [vp, ll, i]
    lib.ugsm_fake_calls.argtypes = [vp]
    lib.ugsm_fake_calls.restype = ll
    lib.ugsm_fake_call.argtypes = [vp, ll, C.POINTER(i * 7), C.POINTER(vp * 16)]
    lib.ugsm_fake_cloud_call.argtypes = [vp, ll, C.POINTER(i * 8), C.POINTER(C.c_double)]
    lib.ugsm_fake_call_args.argtypes = [vp, ll, C.POINTER(ll * 7), C.POINTER(ll * (9 * 16))]
    lib.ugsm_fake_cloud_jobs.argtypes = [vp, ll, C.POINTER(ll * (12 * 16)), C.POINTER(i)]
    lib.ugsm_fake_unpinned.argtypes = [vp]
    lib.ugsm_fake_unpinned.restype = None
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
    lib.ugsm_enqueue_full_cloud.argtypes = [vp, vp, vp, i, i, i, vp, qc, vp, ll, vp, u64]
    lib.ugsm_enqueue_foveated_cloud.argtypes = [vp, vp, vp, i, i, i, i, i, vp, qc, vp, ll, vp, vp, u64]
    lib.ugsm_enqueue_full_cloud_managed.argtypes = [vp, vp, vp, i, i, i, qc, u64]
    lib.ugsm_enqueue_foveated_cloud_managed.argtypes = [vp, vp, vp, i, i, i, i, i, qc, u64]
    lib.ugsm_done_cloud.argtypes = [vp, C.POINTER(CloudResult)]
    lib.ugsm_flush.argtypes = [vp]
    lib.ugsm_next_done.argtypes = [vp, C.POINTER(Completion), i]
    lib.ugsm_queue_depth.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ugsm_queue_plan.argtypes = [vp, i, C.POINTER(i), i]
    lib.ugsm_last_error.argtypes = [vp]
    lib.ugsm_last_error.restype = C.c_char_p
    return lib


BASE = 0x7F0000000000   # made-up "device" addresses: the queue hands them on and never looks behind them


def spec(p1=1.0, sampling=1, fmt=0, compact=0, min_conf=-np.inf, z=(-np.inf, np.inf), max_points=0, want_planes=0):
    s = QueueCloud()
    s.P1[0], s.P2[0] = p1, 1.0
    s.params = CloudParams(sampling, fmt, compact, min_conf, z[0], z[1])
    s.max_points, s.want_planes = max_points, want_planes
    return s


class Host:
    """A host program on the queue with cloud pairs; keeps the books the assertions need."""

    def __init__(self, lib, slots, batch, poll_delay=0, hooks=1):
        self.lib, self.slots, self.batch = lib, slots, max(1, batch)
        self.ctx = lib.ugsm_fake_create_cloud(slots, batch, 8, 4, hooks)
        assert self.ctx
        lib.ugsm_fake_poll_delay(self.ctx, poll_delay)
        self.accepted, self.reported, self.status, self.kind = [], [], {}, {}
        self.next_tag = 0
        self.clouds = {}

    def close(self):
        self.lib.ugsm_fake_destroy_cloud(self.ctx)
        self.ctx = None

    def images(self, tag):
        img = np.zeros((2, 16, 3 * 32), np.uint8)       # a 32 x 16 rgb8 pair; the fake takes the cloud's count from the left image's first word
        img[0].reshape(-1)[:4].view(np.uint32)[0] = tag
        return img

    def enqueue(self, kind, sp=None, size=(64, 32)):
        tag = self.next_tag
        self.next_tag += 1
        W, H = size
        p = BASE + 4096 * tag
        lib, ctx = self.lib, self.ctx
        sp = C.byref(sp) if sp is not None else None
        if kind == "full":
            st = lib.ugsm_enqueue_full(ctx, p, p + 1, W, H, 3 * W, p + 2, tag)
        elif kind == "managed":
            img = self.images(tag)
            st = lib.ugsm_enqueue_full_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, 32, 16, 96, tag)
        elif kind == "cloud":
            st = lib.ugsm_enqueue_full_cloud(ctx, p, p + 1, W, H, 3 * W, p + 2, sp, p + 16, 1000, p + 32, tag)
        elif kind == "fcloud":
            st = lib.ugsm_enqueue_foveated_cloud(ctx, p, p + 1, W, H, 3 * W, 0, 0, p + 2, sp, p + 16, 1000, p + 32, p + 40, tag)
        elif kind == "mcloud":
            img = self.images(tag)
            st = lib.ugsm_enqueue_full_cloud_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, 32, 16, 96, sp, tag)
        else:
            img = self.images(tag)
            st = lib.ugsm_enqueue_foveated_cloud_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, 32, 16, 96, 3, 4, sp, tag)
        if st == OK:
            self.accepted.append(tag)
            self.kind[tag] = kind
        return st

    def call(self, k):
        v, L = (C.c_int * 7)(), (C.c_void_p * 16)()
        assert self.lib.ugsm_fake_call(self.ctx, k, C.byref(v), C.byref(L)) == 0, k
        rec = dict(slot=v[0], n=v[1], mode=v[2], mem=v[3], status=v[4], more=v[5], drained=v[6], cloud=None)
        c, p1 = (C.c_int * 8)(), C.c_double()
        if self.lib.ugsm_fake_cloud_call(self.ctx, k, C.byref(c), C.byref(p1)) == 0:
            rec["cloud"] = dict(fovea=c[0], managed=c[1], n=c[2], finishes=c[3], want_planes=c[4], sampling=c[5], format=c[6], compact=c[7], p1=p1.value)
        return rec

    def calls(self):
        return [self.call(k) for k in range(self.lib.ugsm_fake_calls(self.ctx))]

    def done_cloud(self):
        r = CloudResult()
        st = self.lib.ugsm_done_cloud(self.ctx, C.byref(r))
        return st, r

    def next_done(self, block):
        c = Completion()
        st = self.lib.ugsm_next_done(self.ctx, C.byref(c), block)
        if st == OK:
            rec = self.call(c.call_index)
            assert rec["drained"] == 1, (c.tag, rec)          # reported only once the slot has been seen finished -- the second time, for a managed cloud call
            assert c.call_pairs == rec["n"] and c.slot == rec["slot"], (c.tag, rec)
            tag = int(c.tag)
            self.reported.append(tag)
            self.status[tag] = c.status
            dst, r = self.done_cloud()
            if self.kind[tag] in ("mcloud", "mfcloud") and c.status == OK:
                assert rec["cloud"]["finishes"] == 1, rec      # the finish hook ran, once
                assert dst == OK and r.count == tag + 100, (tag, dst, r.count)
                if r.stored:
                    assert C.cast(r.points, C.POINTER(C.c_uint32))[0] == tag                   # this pair's staging
                assert r.levels == (4 if self.kind[tag] == "mfcloud" else 0)
                assert [r.level_counts[l] for l in range(r.levels)] == [tag + l for l in range(r.levels)]
                assert bool(c.result[0]) == bool(rec["cloud"]["want_planes"])
                self.clouds[tag] = (r.points, r.stored, r.point_step)
            else:
                assert dst == STATE, (tag, self.kind[tag], dst)
            if self.kind[tag] == "managed":
                assert c.result[0] and c.result[1] and c.result[2]
            elif self.kind[tag] in ("full", "cloud", "fcloud"):
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

    def depth(self):
        w, f, u = C.c_int(), C.c_int(), C.c_int()
        assert self.lib.ugsm_queue_depth(self.ctx, C.byref(w), C.byref(f), C.byref(u)) == OK
        return w.value, f.value, u.value

    def check(self):
        assert self.reported == self.accepted, (self.reported, self.accepted)            # exactly once, in enqueue order
        assert self.lib.ugsm_fake_violations(self.ctx) == 0                               # no slot reused early, no finish on a busy slot or twice
        for rec in self.calls():
            assert 1 <= rec["n"] <= self.batch, rec
            if rec["cloud"] and rec["cloud"]["managed"] and rec["status"] == OK:
                assert rec["cloud"]["finishes"] == 1, rec
            elif rec["cloud"]:
                assert rec["cloud"]["finishes"] == 0, rec
        assert self.depth() == (0, 0, 0)


def plan(lib, slots, batch, n):
    """ugsm_queue_plan: what the header says a burst of n pairs becomes."""
    class Config(C.Structure):   # ugsm_config (include/ugsm.h)
        _fields_ = [(f, C.c_float if f in ("early_exit_threshold", "lr_check_threshold") else C.c_int) for f in (
            "device", "levels", "fovea_levels", "slots", "kernel_path", "profile_events", "march_min_pixels", "march_np", "march_rows", "march_smooth",
            "early_exit_threshold", "small_max_pixels", "lr_check_threshold", "streams", "batch", "stream_priority")]
    cfg = Config()
    cfg.slots, cfg.batch, cfg.levels, cfg.fovea_levels = slots, batch, 8, 4
    sizes = (C.c_int * 64)()
    k = lib.ugsm_queue_plan(C.byref(cfg), n, sizes, 64)
    return [sizes[i] for i in range(k)]


def test_pairs_with_equal_specs_share_a_call_and_any_difference_ends_the_group(fq):
    h = Host(fq, 4, 8, poll_delay=10 ** 6)
    try:
        groups = [("cloud", spec()), ("cloud", spec()), ("cloud", spec()),                # three pairs, equal specs (separate objects: copied at enqueue)
                  ("cloud", spec(p1=2.0)),                                                # another P1
                  ("cloud", spec(p1=2.0, sampling=3)), ("cloud", spec(p1=2.0, sampling=3)),   # another params field
                  ("cloud", spec(p1=2.0, sampling=3, compact=1, min_conf=0.5)),
                  ("full", None), ("full", None),                                         # plain pairs never share a call with cloud pairs
                  ("cloud", spec(p1=2.0, sampling=3, compact=1, min_conf=0.5)),
                  ("fcloud", spec(p1=2.0, sampling=3, compact=1, min_conf=0.5)),          # another mode
                  ("mcloud", spec()), ("mcloud", spec()), ("mcloud", spec(want_planes=1)),   # want_planes ends the group
                  ("managed", None),
                  ("mcloud", spec(want_planes=1)), ("mcloud", spec(want_planes=1, max_points=7))]
        for kind, sp in groups:
            assert h.enqueue(kind, sp) == OK
            if len(h.accepted) % 5 == 0:
                assert h.next_done(0) in (OK, PENDING)
        assert fq.ugsm_flush(h.ctx) == OK
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        h.drain()
        h.check()
        calls = h.calls()
        assert [c["n"] for c in calls] == [3, 1, 2, 1, 2, 1, 1, 2, 1, 1, 1, 1], [c["n"] for c in calls]
        assert [c["cloud"] is not None for c in calls] == [True] * 4 + [False] + [True] * 4 + [False] + [True] * 2
        assert [c["cloud"]["p1"] for c in calls[:4]] == [1.0, 2.0, 2.0, 2.0]
        assert [c["cloud"]["sampling"] for c in calls[:4]] == [1, 1, 3, 3] and calls[3]["cloud"]["compact"] == 1
        assert calls[6]["cloud"]["fovea"] == 1 and calls[6]["mode"] == 1
        assert [c["cloud"]["want_planes"] for c in calls[7:9]] == [0, 1] and calls[7]["cloud"]["managed"] == 1
    finally:
        h.close()


def test_a_burst_of_cloud_pairs_is_staggered_like_any_other(fq):
    """Four slots, calls of up to eight, 32 cloud pairs enqueued back to back while nothing finishes: the sizes ugsm_queue_plan gives."""
    for kind in ("cloud", "mcloud"):
        h = Host(fq, 4, 8, poll_delay=10 ** 6)
        try:
            sp = spec(compact=1, min_conf=0.25)
            for _ in range(32):
                assert h.enqueue(kind, sp) == OK
            assert [c["n"] for c in h.calls()] == [4, 5, 7, 8, 8] == plan(fq, 4, 8, 32), h.calls()
            assert [c["slot"] for c in h.calls()] == [0, 1, 2, 3, 0] and all(c["more"] == 1 for c in h.calls())
            fq.ugsm_fake_poll_delay(h.ctx, 0)
            assert fq.ugsm_flush(h.ctx) == OK
            h.drain()
            h.check()
        finally:
            h.close()


def test_a_managed_cloud_call_completes_in_two_steps(fq):
    """One managed cloud call whose slot needs three polls per drain: nothing is reported, and the finish hook has not run, until the slot
    was seen idle; then the hook has run once and the pairs are still not reported until the slot has drained a second time."""
    h = Host(fq, 2, 2, poll_delay=3)
    try:
        for _ in range(2):
            assert h.enqueue("mcloud", spec(fmt=1)) == OK
        assert len(h.calls()) == 1
        seen = []
        for _ in range(12):
            st = h.next_done(0)
            rec = h.call(0)
            seen.append((st, rec["cloud"]["finishes"], rec["drained"]))
            if st == OK:
                break
        # three polls pending; the fourth finds the slot idle: the hook runs, the slot is busy again and is asked at once (the first of three
        # more polls that find it pending); then the report
        assert seen == [(PENDING, 0, 0)] * 3 + [(PENDING, 1, 0)] * 3 + [(OK, 1, 1)], seen
        assert h.reported == [0]
        h.drain()
        h.check()
        assert h.clouds[0][2] == 16 and h.clouds[0][1] == 100
    finally:
        h.close()


def test_pairs_are_reported_in_enqueue_order_when_a_later_call_finishes_first(fq):
    h = Host(fq, 2, 1, poll_delay=6)
    try:
        assert h.enqueue("mcloud", spec()) == OK                                         # call 0: six polls per drain
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        assert h.enqueue("mfcloud", spec()) == OK                                        # call 1: finishes at once
        assert [c["n"] for c in h.calls()] == [1, 1]
        assert h.next_done(0) == PENDING
        assert h.call(1)["cloud"]["finishes"] == 1 and h.call(0)["cloud"]["finishes"] == 0   # the later call's clouds are on their way ...
        assert h.next_done(0) == PENDING and h.reported == []                             # ... and wait for the call before it
        h.drain()
        h.check()
        assert h.reported == [0, 1]
    finally:
        h.close()


def test_done_cloud_follows_the_completion_and_the_staging_stays_lent(fq):
    h = Host(fq, 2, 2)
    try:
        st, _ = h.done_cloud()
        assert st == STATE                                                                # nothing reported yet
        assert h.enqueue("mcloud", spec(max_points=40)) == OK and h.enqueue("managed") == OK and h.enqueue("cloud", spec()) == OK
        assert h.next_done(1) == OK and h.reported == [0]
        p0, stored, step = h.clouds[0]
        assert stored == 40 and step == 32                                                # count 100, capped
        word = C.cast(p0, C.POINTER(C.c_uint32))
        # more managed cloud pairs go through both steps while pair 0's cloud is lent: its staging is not handed to any of them
        for _ in range(3):
            assert h.enqueue("mcloud", spec(max_points=40)) == OK
            assert fq.ugsm_flush(h.ctx) == OK
        assert sum(1 for c in h.calls() if c["cloud"] and c["cloud"]["finishes"]) >= 2
        assert word[0] == 0
        assert h.next_done(1) == OK and h.reported == [0, 1]                              # a plain managed pair: no cloud (checked in next_done)
        assert h.next_done(1) == OK and h.reported == [0, 1, 2]                           # a device cloud pair: none either
        h.drain()
        h.check()
        assert len({h.clouds[t][0] for t in (3, 4, 5)}) >= 2
    finally:
        h.close()


@pytest.mark.parametrize("which", ["submit", "finish"])
def test_a_failing_hook_reports_every_pair_of_the_call_once(fq, which):
    h = Host(fq, 2, 3, poll_delay=2)
    try:
        (fq.ugsm_fake_fail_call if which == "submit" else fq.ugsm_fake_fail_finish)(h.ctx, 1, DEVICE)
        for _ in range(8):
            assert h.enqueue("mcloud", spec()) == OK
        assert fq.ugsm_flush(h.ctx) == OK
        h.drain()
        assert h.reported == h.accepted and fq.ugsm_fake_violations(h.ctx) == 0
        calls = h.calls()
        failed = [t for t in h.accepted if h.status[t] != OK]
        assert len(failed) == calls[1]["n"] and all(h.status[t] == DEVICE for t in failed), (failed, calls)
        assert calls[1]["cloud"]["finishes"] == (0 if which == "submit" else 1)
        assert all(c["cloud"]["finishes"] == 1 for k, c in enumerate(calls) if k != 1)
        assert h.depth() == (0, 0, 0)
    finally:
        h.close()


def scenario(h):
    kinds = [("mcloud", spec())] * 5 + [("cloud", spec())] * 4 + [("managed", None)] * 3 + [("mfcloud", spec(want_planes=1))] * 4 + [("full", None)] * 2
    for kind, sp in kinds + kinds[:9]:
        h.enqueue(kind, sp)
        for _ in range(2):
            if h.next_done(0) != OK:
                break
    h.lib.ugsm_flush(h.ctx)


def test_host_allocation_failures_lose_no_cloud_pair(fq):
    """The same host program with the 1st, 2nd, 3rd ... host allocation inside the library failing -- the queue's bookkeeping, the per-call
    cloud records, the managed staging, the cloud staging the finish hook asks for: an entry point may answer UGSM_ERR_NOMEM, a call may be
    reported as failed; every pair whose enqueue answered UGSM_OK is reported exactly once, in order."""
    h = Host(fq, 2, 3, poll_delay=1)
    a0 = fq.ugsm_fake_allocs()
    scenario(h)
    h.drain()
    h.check()
    n_allocs = fq.ugsm_fake_allocs() - a0
    assert len(h.accepted) == 27
    h.close()
    assert n_allocs > 10, n_allocs
    refused = failed = 0
    for k in range(n_allocs + 2):
        h = Host(fq, 2, 3, poll_delay=1)
        try:
            fq.ugsm_fake_fail_alloc_after(k)
            scenario(h)
            h.drain(tolerate=True)
            fq.ugsm_fake_fail_alloc_after(-1)
            assert h.reported == h.accepted, (k, h.reported, h.accepted)
            assert fq.ugsm_fake_violations(h.ctx) == 0 and h.depth() == (0, 0, 0)
            refused += len(h.accepted) < 27
            failed += any(s != OK for s in h.status.values())
        finally:
            h.close()
    assert refused > 3 and failed > 0, (refused, failed)      # (the faults do land: in an enqueue, which refuses its pair, and in a finish step)


def test_bad_arguments_are_rejected_and_leave_the_queue_alone(fq):
    h = Host(fq, 2, 4, poll_delay=10 ** 6)
    try:
        assert h.enqueue("cloud", spec()) == OK
        before = h.depth()
        nan = float("nan")
        bad = [spec(sampling=0), spec(fmt=2), spec(min_conf=nan), spec(z=(nan, 1.0)), spec(z=(0.0, nan)), spec(z=(2.0, 1.0)), spec(max_points=-1)]
        for kind in ("cloud", "fcloud", "mcloud", "mfcloud"):
            for sp in bad:
                assert h.enqueue(kind, sp) == BAD_ARG, (kind, sp.params.sampling, sp.params.format)
            assert h.enqueue(kind, None) == BAD_ARG                                       # no spec
        lib, ctx, p, sp = fq, h.ctx, BASE, C.byref(spec())
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, p, sp, None, 10, p + 32, 1) == BAD_ARG      # null points
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, p, sp, p + 8, 10, p + 32, 1) == BAD_ARG     # misaligned points
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, p, sp, p + 16, -1, p + 32, 1) == BAD_ARG    # cap < 0
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, p, sp, p + 16, 10, None, 1) == BAD_ARG      # null count
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, p, sp, p + 16, 10, p + 4, 1) == BAD_ARG     # misaligned count
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 192, None, sp, p + 16, 10, p + 32, 1) == BAD_ARG  # null d_out
        assert lib.ugsm_enqueue_full_cloud(ctx, p, p, 64, 32, 100, p, sp, p + 16, 10, p + 32, 1) != OK         # stride < 3 W
        assert lib.ugsm_enqueue_foveated_cloud(ctx, p, p, 64, 32, 192, 0, 0, p, sp, p + 16, 10, p + 32, p + 4, 1) == BAD_ARG   # misaligned level counts
        assert lib.ugsm_enqueue_full_cloud_managed(ctx, None, p, 32, 16, 96, sp, 1) == BAD_ARG
        assert h.depth() == before
        assert lib.ugsm_done_cloud(ctx, None) == BAD_ARG
    finally:
        h.close()
    h = Host(fq, 2, 4)
    try:
        fq.ugsm_fake_destroy_cloud(h.ctx)
        h.ctx = fq.ugsm_fake_create_cloud(2, 4, 8, 1, 1)                                  # a context without fovea levels
        for kind in ("fcloud", "mfcloud"):
            assert h.enqueue(kind, spec()) == BAD_ARG
        assert h.enqueue("cloud", spec()) == OK
        h.drain()
    finally:
        h.close()
    h = Host(fq, 2, 4, hooks=0)                                                           # a runtime without the cloud hooks: refused, not crashed
    try:
        assert h.enqueue("cloud", spec()) == STATE and h.enqueue("mcloud", spec()) == STATE
        assert h.enqueue("full") == OK
        h.drain()
        assert h.depth() == (0, 0, 0)
    finally:
        h.close()


def test_the_queue_still_links_against_the_plain_fake(tmp_path):
    """tests/fake_runtime.cpp knows nothing of clouds; the queue reaches the cloud work through hooks only, so the shared object of
    tests/test_queue_host.py still builds and loads with every symbol resolved at once."""
    so = build(tmp_path, "fake_runtime.cpp")
    lib = C.CDLL(so, mode=os.RTLD_NOW)
    for name in ("ugsm_enqueue_full_cloud", "ugsm_enqueue_foveated_cloud", "ugsm_enqueue_full_cloud_managed", "ugsm_enqueue_foveated_cloud_managed", "ugsm_done_cloud"):
        assert hasattr(lib, name), name


# ---- what a cloud call carries: every CloudJob field of every pair ---------------------------------------------------------------------
def _cloud_jobs(fq, ctx, k):
    head, pairs, jobs, reserved = (C.c_longlong * 7)(), (C.c_longlong * (9 * 16))(), (C.c_longlong * (12 * 16))(), C.c_int(-1)
    assert fq.ugsm_fake_call_args(ctx, k, C.byref(head), C.byref(pairs)) == 0
    assert fq.ugsm_fake_cloud_jobs(ctx, k, C.byref(jobs), C.byref(reserved)) == 0
    rec = dict(zip(("entry", "W", "H", "stride", "fmt", "pyr_arrays", "n"), head))
    rec["reserved"] = reserved.value
    rec["jobs"] = [list(jobs[12 * b:12 * b + 12]) for b in range(rec["n"])]
    return rec


def test_cloud_marshalling(fq):
    """Every cloud call the hook receives carries exactly what its pairs were enqueued with -- every CloudJob field, in enqueue order, the
    call's size and stride, the spec with `reserved` cleared -- for the four cloud kinds in calls of one pair and of several; a managed
    pair's images, planes and completion are its staging buffer's carve-up."""
    ctx = fq.ugsm_fake_create_cloud(2, 3, 8, 4, 1)
    want, images, done, staged = {}, {}, [], {}
    W, H = 64, 32

    def enqueue(kind, want_planes=0):
        tag = len(want)
        sp = spec(want_planes=want_planes, max_points=50)
        sp.reserved = 7
        p = BASE + 4096 * tag
        L, R, out, points, count, lc = p, p + 64, p + 128, p + 256, p + 512, p + 768
        ox, oy, cap = 3 + tag, 1000 + tag, 5000 + tag
        fovea, managed = kind in ("fcloud", "mfcloud"), kind in ("mcloud", "mfcloud")
        w = dict(kind=kind, fovea=fovea, managed=managed, want_planes=want_planes, stride=3 * W + 8, ox=ox if fovea else 0, oy=oy if fovea else 0)
        if kind == "cloud":
            st = fq.ugsm_enqueue_full_cloud(ctx, L, R, W, H, 3 * W + 8, out, C.byref(sp), points, cap, count, tag)
            w["job"] = [L, R, 0, 0, out, 0, 0, 0, points, cap, count, 0]
        elif kind == "fcloud":
            st = fq.ugsm_enqueue_foveated_cloud(ctx, L, R, W, H, 3 * W + 8, ox, oy, out, C.byref(sp), points, cap, count, lc, tag)
            w["job"] = [L, R, ox, oy, out, 0, 0, 0, points, cap, count, lc]
        else:
            img = np.random.RandomState(tag).randint(0, 256, (2, H, 3 * W + 8)).astype(np.uint8)
            img[0].reshape(-1)[:4].view(np.uint32)[0] = tag                 # (the fake takes the cloud's count from the left image's first word)
            images[tag] = [img[s][:, :3 * W].tobytes() for s in range(2)]
            w["stride"] = 3 * W
            if kind == "mcloud":
                st = fq.ugsm_enqueue_full_cloud_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, W, H, 3 * W + 8, C.byref(sp), tag)
            else:
                st = fq.ugsm_enqueue_foveated_cloud_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, W, H, 3 * W + 8, ox, oy, C.byref(sp), tag)
            img[:] = 0
        sp.reserved, sp.want_planes = 9, 1 - want_planes                   # (the spec was copied at enqueue)
        assert st == OK, (kind, st, fq.ugsm_last_error(ctx))
        want[tag] = w

    def drain():
        while True:
            c = Completion()
            st = fq.ugsm_next_done(ctx, C.byref(c), 1)
            if st == EMPTY:
                return
            assert st == OK and c.status == OK, (st, c.status)
            tag, k = int(c.tag), int(c.call_index)
            b = sum(1 for _, kk, _ in done if kk == k)
            done.append((tag, k, [C.cast(c.result[j], C.c_void_p).value or 0 for j in range(5)]))
            if want[tag]["managed"]:                                       # the staging is lent until the next ugsm_next_done: look now
                job = _cloud_jobs(fq, ctx, k)["jobs"][b]
                staged[tag] = [C.string_at(job[0], 3 * W * H), C.string_at(job[1], 3 * W * H)]

    try:
        # (the first call after idle or a flush takes two pairs, the later ones three)
        enqueue("cloud"), enqueue("cloud"), enqueue("cloud"), enqueue("fcloud"), enqueue("fcloud"), enqueue("fcloud"), drain()
        enqueue("fcloud"), drain()
        enqueue("mcloud", 1), enqueue("mcloud", 1), enqueue("mcloud", 1), enqueue("mcloud", 0), enqueue("mcloud", 0)
        enqueue("mfcloud", 1), enqueue("mfcloud", 1), enqueue("mfcloud", 1), drain()
        enqueue("mfcloud", 0), drain()
        assert fq.ugsm_fake_violations(ctx) == 0
        assert [t for t, _, _ in done] == list(range(len(want)))
        ncalls = fq.ugsm_fake_calls(ctx)
        assert sorted({k for _, k, _ in done}) == list(range(ncalls))
        seen = set()
        for k in range(ncalls):
            rec = _cloud_jobs(fq, ctx, k)
            tags = [t for t, kk, _ in done if kk == k]
            results = [r for _, kk, r in done if kk == k]
            n, w0 = rec["n"], want[tags[0]]
            assert n == len(tags) and tags == list(range(tags[0], tags[0] + n)), (k, rec, tags)
            assert rec["entry"] == 8 + (2 if w0["fovea"] else 0) + (4 if w0["managed"] else 0), (k, rec)
            assert (rec["W"], rec["H"], rec["stride"], rec["fmt"], rec["reserved"]) == (W, H, w0["stride"], 0, 0), (k, rec)
            v, p1 = (C.c_int * 8)(), C.c_double()
            assert fq.ugsm_fake_cloud_call(ctx, k, C.byref(v), C.byref(p1)) == 0
            assert (v[0], v[1], v[2], v[4]) == (int(w0["fovea"]), int(w0["managed"]), n, w0["want_planes"]), (k, list(v))
            for t, job, res in zip(tags, rec["jobs"], results):
                w = want[t]
                assert (w["kind"], w["want_planes"]) == (w0["kind"], w0["want_planes"])
                if not w["managed"]:
                    assert job == w["job"], (k, t, job, w["job"])
                    assert res == [0] * 5
                else:
                    img = (3 * W * H + 255) & ~255
                    plane = (4 * (W // 8) * (H // 8) if w["fovea"] else W * H) * 4
                    L = job[0]
                    planes = [res[0], res[0] + plane, res[0] + 2 * plane] if w["want_planes"] else [0, 0, 0]
                    assert L and bool(res[0]) == bool(w["want_planes"])
                    assert job == [L, L + img, w["ox"], w["oy"], 0] + planes + [0, 0, 0, 0], (k, t, job)
                    assert res == planes + [0, 0], (t, res)
                    assert staged[t] == images[t], (k, t)
                seen.add((w["kind"], n > 1))
        assert seen == {(kind, many) for kind in ("cloud", "fcloud", "mcloud", "mfcloud") for many in (False, True)}, seen
    finally:
        fq.ugsm_fake_destroy_cloud(ctx)


# ---- the refusals of all ten entry points, in their order ---------------------------------------------------------------------------------
SIZE_MISMATCH = 2
M_NULL = "ugsm_enqueue_%s: null buffer"
M_NULL_MANAGED = "ugsm_enqueue_*_managed: null image"
M_SIZE = "ugsm_enqueue_*: bad image size for the context's pyramid"
M_STRIDE = "ugsm_enqueue_*: stride < bytes per pixel of the input format * W"
M_FOVEA = "ugsm_enqueue_foveated*: the context has no fovea levels"
M_PINNED = ("ugsm_enqueue_%s: every host buffer must be page-locked (ugsm_host_alloc, hipHostMalloc or hipHostRegister); "
            "ugsm_enqueue_%s_managed takes any memory")
M_SPEC = "ugsm_enqueue_*_cloud*: null spec"
M_SAMPLING = "ugsm_enqueue_*_cloud*: sampling < 1 or an unknown record format"
M_NAN = "ugsm_enqueue_*_cloud*: a NaN min_conf / z_min / z_max, or z_min > z_max"
M_MAX_POINTS = "ugsm_enqueue_*_cloud*: max_points < 0"
M_BUFFERS = "ugsm_enqueue_*_cloud: a null or misaligned cloud buffer, or cap_points < 0"
M_NO_CLOUDS = "ugsm_enqueue_*_cloud*: this runtime makes no clouds"
M_FULL = ("ugsm_enqueue_*: (slots + 1) x batch pairs are outstanding and completions wait to be fetched: "
          "call ugsm_next_done first")

# name -> (the call, the result pointers it requires)
ENTRY_POINTS = {
    "full": (lambda q, c, a: q.ugsm_enqueue_full(c, a.L, a.R, a.W, a.H, a.stride, a.o0, a.tag), ["o0"]),
    "foveated": (lambda q, c, a: q.ugsm_enqueue_foveated(c, a.L, a.R, a.W, a.H, a.stride, a.ox, a.oy, a.o0, a.pl, a.pr, a.tag), ["o0"]),
    "full_host": (lambda q, c, a: q.ugsm_enqueue_full_host(c, a.L, a.R, a.W, a.H, a.stride, a.o0, a.o1, a.o2, a.tag), ["o0", "o1", "o2"]),
    "foveated_host": (lambda q, c, a: q.ugsm_enqueue_foveated_host(c, a.L, a.R, a.W, a.H, a.stride, a.ox, a.oy, a.o0, a.o1, a.o2, a.pl, a.pr, a.tag),
                      ["o0", "o1", "o2"]),
    "full_managed": (lambda q, c, a: q.ugsm_enqueue_full_managed(c, a.L, a.R, a.W, a.H, a.stride, a.tag), []),
    "foveated_managed": (lambda q, c, a: q.ugsm_enqueue_foveated_managed(c, a.L, a.R, a.W, a.H, a.stride, a.ox, a.oy, 1, a.tag), []),
    "full_cloud": (lambda q, c, a: q.ugsm_enqueue_full_cloud(c, a.L, a.R, a.W, a.H, a.stride, a.o0, a.spec, a.points, a.cap, a.count, a.tag), ["o0"]),
    "foveated_cloud": (lambda q, c, a: q.ugsm_enqueue_foveated_cloud(c, a.L, a.R, a.W, a.H, a.stride, a.ox, a.oy, a.o0, a.spec, a.points, a.cap, a.count,
                                                                    a.lc, a.tag), ["o0"]),
    "full_cloud_managed": (lambda q, c, a: q.ugsm_enqueue_full_cloud_managed(c, a.L, a.R, a.W, a.H, a.stride, a.spec, a.tag), []),
    "foveated_cloud_managed": (lambda q, c, a: q.ugsm_enqueue_foveated_cloud_managed(c, a.L, a.R, a.W, a.H, a.stride, a.ox, a.oy, a.spec, a.tag), []),
}


def refusals(name):
    """(what, context, arguments that differ from a good call, status, message) for entry point `name`, several refusals at once where the
    order between them is to be pinned: the one named first in `what` wins."""
    fovea, managed, cloud = "foveated" in name, name.endswith("managed"), "cloud" in name
    host, device_cloud = name.endswith("host"), cloud and not managed
    null = M_NULL_MANAGED if managed else M_NULL % name
    small, tiny = dict(stride=3 * 64 - 1), dict(W=8)
    out = [("null left image", "good", dict(L=None), BAD_ARG, null), ("null right image", "good", dict(R=None), BAD_ARG, null),
           ("null image, then size", "good", dict(R=None, **tiny), BAD_ARG, null),
           ("size", "good", tiny, BAD_ARG, M_SIZE), ("size, then stride", "good", dict(W=8, stride=1), BAD_ARG, M_SIZE),
           ("stride", "good", small, SIZE_MISMATCH, M_STRIDE), ("stride, then full queue", "full", small, SIZE_MISMATCH, M_STRIDE),
           ("full queue", "full", {}, STATE, M_FULL)]
    for r in ENTRY_POINTS[name][1]:
        out += [("null result " + r, "good", {r: None}, BAD_ARG, null), ("null result %s, then size" % r, "good", dict(tiny, **{r: None}), BAD_ARG, null)]
    if fovea:
        out += [("stride, then no fovea levels", "no fovea", small, SIZE_MISMATCH, M_STRIDE), ("no fovea levels", "no fovea", {}, BAD_ARG, M_FOVEA)]
    if host:
        pinned = M_PINNED % (name, name[:-5])
        out += [("not page-locked: " + r, "good", dict(unpinned=r), BAD_ARG, pinned) for r in ["L", "R"] + ENTRY_POINTS[name][1]]
        out += [("stride, then not page-locked", "good", dict(small, unpinned="L"), SIZE_MISMATCH, M_STRIDE),
                ("not page-locked, then full queue", "full", dict(unpinned="o1"), BAD_ARG, pinned)]
        if fovea:
            out += [("not page-locked: " + r, "good", {r: BASE + 8192, "unpinned": r}, BAD_ARG, pinned) for r in ("pl", "pr")]
            out += [("no fovea levels, then not page-locked", "no fovea", dict(unpinned="L"), BAD_ARG, M_FOVEA)]
    if cloud:
        nan = float("nan")
        out += [("stride, then null spec", "good", dict(small, spec=None), SIZE_MISMATCH, M_STRIDE),
                ("null spec", "good", dict(spec=None), BAD_ARG, M_SPEC), ("null spec, then no cloud hooks", "no hooks", dict(spec=None), BAD_ARG, M_SPEC),
                ("sampling 0", "good", dict(spec=spec(sampling=0)), BAD_ARG, M_SAMPLING),
                ("sampling 0, then NaN", "good", dict(spec=spec(sampling=0, min_conf=nan)), BAD_ARG, M_SAMPLING),
                ("NaN, then max_points", "good", dict(spec=spec(z=(nan, 1.0), max_points=-1)), BAD_ARG, M_NAN),
                ("max_points, then no cloud hooks", "no hooks", dict(spec=spec(max_points=-1)), BAD_ARG, M_MAX_POINTS),
                ("no cloud hooks", "no hooks", {}, STATE, M_NO_CLOUDS), ("no cloud hooks, then full queue", "no hooks, full", {}, STATE, M_NO_CLOUDS),
                ("null spec, then full queue", "full", dict(spec=None), BAD_ARG, M_SPEC)]
        if fovea:
            out += [("no fovea levels, then null spec", "no fovea", dict(spec=None), BAD_ARG, M_FOVEA)]
    if device_cloud:
        out += [("misaligned d_points", "good", dict(points=BASE + 8), BAD_ARG, M_BUFFERS), ("null d_count", "good", dict(count=None), BAD_ARG, M_BUFFERS),
                ("sampling 0, then misaligned d_points", "good", dict(spec=spec(sampling=0), points=BASE + 8), BAD_ARG, M_SAMPLING),
                ("max_points, then misaligned d_points", "good", dict(spec=spec(max_points=-1), points=BASE + 8), BAD_ARG, M_MAX_POINTS),
                ("misaligned d_points, then no cloud hooks", "no hooks", dict(points=BASE + 8), BAD_ARG, M_BUFFERS),
                ("misaligned d_points, then full queue", "full", dict(points=BASE + 8), BAD_ARG, M_BUFFERS)]
    return out


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_entry_point_refuses_in_order_with_its_message(fq, name):
    """Each refusal of each ugsm_enqueue_*: its status, the exact text of ugsm_last_error, which of two refusals that apply at once wins,
    and that nothing was enqueued -- the queue is as deep as before, and what it reports in the end are the pairs that were accepted."""
    import types
    call = ENTRY_POINTS[name][0]
    images = np.zeros((2, 32, 3 * 64), np.uint8)      # (real memory: the managed kinds read their images once a pair is accepted)

    def arguments(**over):
        a = types.SimpleNamespace(L=images[0].ctypes.data, R=images[1].ctypes.data, W=64, H=32, stride=3 * 64, ox=1, oy=2, o0=BASE + 128, o1=BASE + 192,
                                  o2=BASE + 256, pl=None, pr=None, spec=spec(), points=BASE + 1024, cap=10, count=BASE + 2048, lc=BASE + 3072, tag=77)
        unpinned = over.pop("unpinned", None)
        vars(a).update(over)
        a.spec = C.byref(a.spec) if a.spec is not None else None
        return a, getattr(a, unpinned) if unpinned else None

    def depth(ctx):
        w, f, u = C.c_int(), C.c_int(), C.c_int()
        assert fq.ugsm_queue_depth(ctx, C.byref(w), C.byref(f), C.byref(u)) == OK
        return w.value, f.value, u.value

    def context(kind):
        full = kind.endswith("full")
        ctx = fq.ugsm_fake_create_cloud(1 if full else 2, 1 if full else 3, 8, 1 if kind == "no fovea" else 4, 0 if kind.startswith("no hooks") else 1)
        assert ctx
        for tag in range(2 if full else 0):           # (slots + 1) x batch = 2 pairs outstanding: one finished and not fetched, one in flight
            assert fq.ugsm_enqueue_full(ctx, BASE, BASE + 64, 64, 32, 3 * 64, BASE + 128, tag) == OK
        return ctx

    assert call(fq, None, arguments()[0]) == BAD_ARG                                     # no context: no message either
    ctxs = {}
    try:
        for what, kind, over, status, message in refusals(name):
            ctx = ctxs[kind] = ctxs.get(kind) or context(kind)
            a, unpinned = arguments(**over)
            before, allocs = depth(ctx), fq.ugsm_fake_allocs()
            fq.ugsm_fake_unpinned(unpinned)
            st = call(fq, ctx, a)
            fq.ugsm_fake_unpinned(None)
            assert (st, fq.ugsm_last_error(ctx).decode()) == (status, message), (name, what)
            assert depth(ctx) == before, (name, what)
            if kind.endswith("full"):
                assert fq.ugsm_fake_allocs() == allocs, (name, what)                      # refused before any staging was made or filled
        for kind, ctx in ctxs.items():                                                    # never reported: only the pairs that filled the queue are
            tags = []
            while True:
                c = Completion()
                st = fq.ugsm_next_done(ctx, C.byref(c), 1)
                if st == EMPTY:
                    break
                assert st == OK
                tags.append(int(c.tag))
            assert tags == ([0, 1] if kind.endswith("full") else []), (name, kind, tags)
        a, _ = arguments()
        assert call(fq, ctxs["good"], a) == OK, (name, fq.ugsm_last_error(ctxs["good"]))       # the good call of the table is one
        c = Completion()
        assert fq.ugsm_next_done(ctxs["good"], C.byref(c), 1) == OK and c.tag == 77 and c.status == OK
    finally:
        for ctx in ctxs.values():
            fq.ugsm_fake_destroy_cloud(ctx)
