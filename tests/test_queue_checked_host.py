"""Checked full-mode pairs through the queue (ugsm_enqueue_full_checked[_managed | _cloud | _cloud_managed], ugsm_done_checked; include/ugsm.h,
"checked pairs through the queue") on a machine without a GPU: the real csrc/ugsm_queue.cpp compiled against tests/fake_runtime_checked.cpp --
the recorder of tests/fake_runtime.cpp, the cloud hooks of tests/fake_runtime_cloud.cpp and stand-ins for the two hooks through which the queue
reaches the runtime's checked call -- and driven through the C-ABI with ctypes.

What the header promises and this file checks:
  * every refusal of the four new ugsm_enqueue_*: status, exact message, which of two refusals wins, nothing enqueued; a runtime without the
    hooks refuses, it does not crash;
  * the hook receives L, R, out, back (NULL entries included), the planes and back planes of managed pairs, tau, the spec and the cloud
    buffers of every pair as it was enqueued;
  * pairs of one call are all checked with one bit-equal tau, or all plain; a cloud ends the group too; whether a pair takes its back field
    does not; call sizes are ugsm_queue_plan's otherwise;
  * completions in enqueue order; ugsm_done_checked answers for the pair just reported and UGSM_ERR_STATE otherwise;
  * a failed call is reported per pair after the drain; the outstanding limit; host allocation failures lose no pair and leave the queue
    usable."""
import ctypes as C
import os
import struct
import subprocess
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, SIZE_MISMATCH, DEVICE, NOMEM, STATE, PENDING, EMPTY = 0, 1, 2, 5, 6, 7, 8, 9
CSRC = os.path.join(ROOT, "ug_stereomatcher_amd", "csrc")
BASE = 0x7F0000000000   # made-up "device" addresses: the queue hands them on and never looks behind them
E_HOST, E_CLOUD, E_CHECKED = 4, 8, 16


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


class CheckedResult(C.Structure):
    _fields_ = [("back", C.POINTER(C.c_float) * 3), ("marked_fwd", C.c_longlong), ("marked_back", C.c_longlong)]


def build(tmp, fakes=("fake_runtime_checked.cpp",), extra=()):
    out = str(tmp / ("lib_" + fakes[0].replace(".cpp", "") + ".so"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-fvisibility=hidden", *[os.path.join(ROOT, "tests", f) for f in fakes],
           os.path.join(CSRC, "ugsm_queue.cpp"), "-Wl,--version-script=" + os.path.join(CSRC, "ugsm.map"), "-o", out, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def fq(tmp_path_factory):
    lib = C.CDLL(build(tmp_path_factory.mktemp("fakeqk")))
    vp, i, u64, ll, f = C.c_void_p, C.c_int, C.c_uint64, C.c_longlong, C.c_float
    qc = C.POINTER(QueueCloud)
    lib.ugsm_fake_create_checked.restype = vp
    lib.ugsm_fake_create_checked.argtypes = [i, i, i, i, i]
    lib.ugsm_fake_destroy_checked.argtypes = [vp]
    lib.ugsm_fake_destroy_checked.restype = None
    lib.ugsm_fake_set_config.argtypes = [vp, f, i]
    lib.ugsm_fake_set_config.restype = None
    lib.ugsm_fake_poll_delay.argtypes = [vp, i]
    lib.ugsm_fake_poll_delay.restype = None
    lib.ugsm_fake_fail_call.argtypes = [vp, ll, i]
    lib.ugsm_fake_calls.argtypes = [vp]
    lib.ugsm_fake_calls.restype = ll
    lib.ugsm_fake_call.argtypes = [vp, ll, C.POINTER(i * 7), C.POINTER(vp * 16)]
    lib.ugsm_fake_call_args.argtypes = [vp, ll, C.POINTER(ll * 7), C.POINTER(ll * (9 * 16))]
    lib.ugsm_fake_checked_call.argtypes = [vp, ll, C.POINTER(i * 6), C.POINTER(f)]
    lib.ugsm_fake_checked_jobs.argtypes = [vp, ll, C.POINTER(ll * (13 * 16)), C.POINTER(C.c_double), C.POINTER(i)]
    lib.ugsm_fake_cloud_call.argtypes = [vp, ll, C.POINTER(i * 8), C.POINTER(C.c_double)]
    lib.ugsm_fake_violations.argtypes = [vp]
    lib.ugsm_fake_fail_alloc_after.argtypes = [ll]
    lib.ugsm_fake_fail_alloc_after.restype = None
    lib.ugsm_fake_allocs.restype = ll
    lib.ugsm_enqueue_full.argtypes = [vp, vp, vp, i, i, i, vp, u64]
    lib.ugsm_enqueue_full_managed.argtypes = [vp, vp, vp, i, i, i, u64]
    lib.ugsm_enqueue_full_cloud.argtypes = [vp, vp, vp, i, i, i, vp, qc, vp, ll, vp, u64]
    lib.ugsm_enqueue_full_checked.argtypes = [vp, vp, vp, i, i, i, vp, vp, f, u64]
    lib.ugsm_enqueue_full_checked_managed.argtypes = [vp, vp, vp, i, i, i, f, i, u64]
    lib.ugsm_enqueue_full_checked_cloud.argtypes = [vp, vp, vp, i, i, i, vp, vp, f, qc, vp, ll, vp, u64]
    lib.ugsm_enqueue_full_checked_cloud_managed.argtypes = [vp, vp, vp, i, i, i, f, i, qc, u64]
    lib.ugsm_done_checked.argtypes = [vp, C.POINTER(CheckedResult)]
    lib.ugsm_done_cloud.argtypes = [vp, C.POINTER(CloudResult)]
    lib.ugsm_flush.argtypes = [vp]
    lib.ugsm_next_done.argtypes = [vp, C.POINTER(Completion), i]
    lib.ugsm_queue_depth.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    lib.ugsm_queue_plan.argtypes = [vp, i, C.POINTER(i), i]
    lib.ugsm_last_error.argtypes = [vp]
    lib.ugsm_last_error.restype = C.c_char_p
    return lib


def spec(p1=1.0, sampling=1, fmt=0, compact=0, min_conf=-np.inf, z=(-np.inf, np.inf), max_points=0, want_planes=0):
    s = QueueCloud()
    s.P1[0], s.P2[0] = p1, 1.0
    s.params = CloudParams(sampling, fmt, compact, min_conf, z[0], z[1])
    s.max_points, s.want_planes = max_points, want_planes
    return s


def plan(lib, slots, batch, n):
    class Config(C.Structure):   # ugsm_config (include/ugsm.h)
        _fields_ = [(f, C.c_float if f in ("early_exit_threshold", "lr_check_threshold") else C.c_int) for f in (
            "device", "levels", "fovea_levels", "slots", "kernel_path", "profile_events", "march_min_pixels", "march_np", "march_rows", "march_smooth",
            "early_exit_threshold", "small_max_pixels", "lr_check_threshold", "streams", "batch", "stream_priority")]
    cfg = Config()
    cfg.slots, cfg.batch, cfg.levels, cfg.fovea_levels = slots, batch, 8, 4
    sizes = (C.c_int * 64)()
    k = lib.ugsm_queue_plan(C.byref(cfg), n, sizes, 64)
    return [sizes[i] for i in range(k)]


W, H = 32, 16   # the managed pairs' images (real memory: they are copied at enqueue)


class Host:
    """A host program on the queue with checked pairs; keeps the books the assertions need.  Kinds: chk (device; back: d_back given),
    mchk (managed; back: want_back), cchk / mcchk (the same with a cloud), full / managed / cloud (plain pairs)."""

    def __init__(self, lib, slots, batch, poll_delay=0, hooks=3):
        self.lib, self.slots, self.batch = lib, slots, max(1, batch)
        self.ctx = lib.ugsm_fake_create_checked(slots, batch, 8, 4, hooks)
        assert self.ctx
        lib.ugsm_fake_poll_delay(self.ctx, poll_delay)
        self.accepted, self.reported, self.status, self.kind, self.back, self.marks = [], [], {}, {}, {}, {}
        self.next_tag = 0

    def close(self):
        self.lib.ugsm_fake_destroy_checked(self.ctx)
        self.ctx = None

    def images(self, tag):
        img = np.zeros((2, H, 3 * W), np.uint8)   # the fake makes a managed pair's counts from the left image's first word
        img[0].reshape(-1)[:4].view(np.uint32)[0] = tag
        return img

    def enqueue(self, kind, tau=1.0, back=True, sp=None):
        tag = self.next_tag
        self.next_tag += 1
        p = BASE + 4096 * tag
        lib, ctx = self.lib, self.ctx
        sp = C.byref(sp) if sp is not None else None
        img = self.images(tag)
        L, R = img[0].ctypes.data, img[1].ctypes.data
        if kind == "full":
            st = lib.ugsm_enqueue_full(ctx, p, p + 1, 64, 32, 192, p + 2, tag)
        elif kind == "managed":
            st = lib.ugsm_enqueue_full_managed(ctx, L, R, W, H, 3 * W, tag)
        elif kind == "cloud":
            st = lib.ugsm_enqueue_full_cloud(ctx, p, p + 1, 64, 32, 192, p + 2, sp, p + 16, 1000, p + 32, tag)
        elif kind == "chk":
            st = lib.ugsm_enqueue_full_checked(ctx, p, p + 1, 64, 32, 192, p + 2, p + 3 if back else None, tau, tag)
        elif kind == "mchk":
            st = lib.ugsm_enqueue_full_checked_managed(ctx, L, R, W, H, 3 * W, tau, int(back), tag)
        elif kind == "cchk":
            st = lib.ugsm_enqueue_full_checked_cloud(ctx, p, p + 1, 64, 32, 192, p + 2, p + 3 if back else None, tau, sp, p + 16, 1000, p + 32, tag)
        else:
            st = lib.ugsm_enqueue_full_checked_cloud_managed(ctx, L, R, W, H, 3 * W, tau, int(back), sp, tag)
        if st == OK:
            self.accepted.append(tag)
            self.kind[tag] = kind
            self.back[tag] = back
        return st

    def call(self, k):
        v, L = (C.c_int * 7)(), (C.c_void_p * 16)()
        assert self.lib.ugsm_fake_call(self.ctx, k, C.byref(v), C.byref(L)) == 0, k
        rec = dict(slot=v[0], n=v[1], mode=v[2], mem=v[3], status=v[4], more=v[5], drained=v[6], checked=None)
        c, tau = (C.c_int * 6)(), C.c_float()
        if self.lib.ugsm_fake_checked_call(self.ctx, k, C.byref(c), C.byref(tau)) == 0:
            rec["checked"] = dict(managed=c[0], n=c[1], has_spec=c[2], marks=c[3], want_planes=c[4], compact=c[5], tau=tau.value)
        return rec

    def calls(self):
        return [self.call(k) for k in range(self.lib.ugsm_fake_calls(self.ctx))]

    def done_checked(self):
        r = CheckedResult()
        return self.lib.ugsm_done_checked(self.ctx, C.byref(r)), r

    def next_done(self, block):
        c = Completion()
        st = self.lib.ugsm_next_done(self.ctx, C.byref(c), block)
        if st == OK:
            rec = self.call(c.call_index)
            assert rec["drained"] == 1, (c.tag, rec)
            assert c.call_pairs == rec["n"] and c.slot == rec["slot"], (c.tag, rec)
            tag = int(c.tag)
            kind = self.kind[tag]
            self.reported.append(tag)
            self.status[tag] = c.status
            dst, r = self.done_checked()
            if kind in ("chk", "mchk", "cchk", "mcchk") and c.status == OK:
                assert dst == OK and rec["checked"]["marks"] == 1, (tag, dst, rec)
                word = tag if kind.startswith("m") else ((BASE + 4096 * tag) >> 12) & 0xFFFFFFFF
                assert (r.marked_fwd, r.marked_back) == (word + 1000, word + 2000), (tag, r.marked_fwd, r.marked_back)
                self.marks[tag] = (r.marked_fwd, r.marked_back)
                lent = kind.startswith("m") and self.back[tag]
                assert [bool(r.back[k]) for k in range(3)] == [lent] * 3, (tag, kind)
                assert not c.result[3] and not c.result[4]
                if kind == "mchk":
                    assert c.result[0] and c.result[1] and c.result[2]
                    if lent:                                      # the back planes lie behind the forward ones in the pair's staging
                        plane = W * H * 4
                        base = C.cast(c.result[0], C.c_void_p).value
                        assert [C.cast(r.back[k], C.c_void_p).value for k in range(3)] == [base + (3 + k) * plane for k in range(3)]
                if kind in ("chk", "cchk"):
                    assert not c.result[0]
                cr = CloudResult()
                assert self.lib.ugsm_done_cloud(self.ctx, C.byref(cr)) == (OK if kind == "mcchk" else STATE)
                if kind == "mcchk":
                    assert cr.count == tag + 100
            else:
                assert dst == STATE, (tag, kind, dst)
                assert self.lib.ugsm_last_error(self.ctx).decode() == "ugsm_done_checked: the last pair ugsm_next_done reported was no checked pair of a call that succeeded"
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
        assert self.reported == self.accepted, (self.reported, self.accepted)   # exactly once, in enqueue order
        assert self.lib.ugsm_fake_violations(self.ctx) == 0                      # no slot reused early, no counts read from a busy slot or twice
        for rec in self.calls():
            assert 1 <= rec["n"] <= self.batch, rec
            if rec["checked"]:
                assert rec["checked"]["marks"] == (1 if rec["status"] == OK else 0), rec
        assert self.depth() == (0, 0, 0)


# ---- grouping -----------------------------------------------------------------------------------------------------------------------------
def test_a_burst_of_mixed_kinds_ends_its_calls_where_the_kinds_change(fq):
    """tau 1.0, 1.0, 0.5, a plain pair, a checked cloud pair, from idle on four slots with calls of up to eight: the first call's target is four
    (ugsm_queue_plan), and every change of kind ends a call before it."""
    h = Host(fq, 4, 8, poll_delay=10 ** 6)
    try:
        assert plan(fq, 4, 8, 5)[0] == 4
        for kind, tau, sp in [("chk", 1.0, None), ("chk", 1.0, None), ("chk", 0.5, None), ("full", 0.0, None), ("cchk", 0.5, spec())]:
            assert h.enqueue(kind, tau=tau, sp=sp) == OK
        assert fq.ugsm_flush(h.ctx) == OK
        calls = h.calls()
        assert [c["n"] for c in calls] == [2, 1, 1, 1], calls
        assert [c["checked"] and c["checked"]["tau"] for c in calls] == [1.0, 0.5, None, 0.5]
        assert [c["checked"] and c["checked"]["has_spec"] for c in calls] == [0, 0, None, 1]
        assert [c["slot"] for c in calls] == [0, 1, 2, 3]
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        h.drain()
        h.check()
    finally:
        h.close()


def test_what_ends_a_group_and_what_does_not(fq):
    h = Host(fq, 4, 8, poll_delay=10 ** 6)
    try:
        up = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
        groups = [("chk", 1.0, True, None), ("chk", 1.0, False, None), ("chk", 1.0, True, None),     # d_back given or not: one call
                  ("chk", up, True, None),                                                          # one ulp more: another tau
                  ("mchk", up, True, None), ("mchk", up, False, None),                              # another memory kind; want_back: one call
                  ("managed", 0.0, True, None),                                                     # a plain managed pair
                  ("mchk", up, False, None),
                  ("mcchk", up, False, spec()), ("mcchk", up, True, spec()),                        # with a cloud
                  ("mcchk", up, True, spec(want_planes=1)),                                         # another spec
                  ("cchk", 2.0, True, spec()), ("cloud", 0.0, True, spec()), ("cchk", 2.0, False, spec())]
        for kind, tau, back, sp in groups:
            assert h.enqueue(kind, tau=tau, back=back, sp=sp) == OK
        assert fq.ugsm_flush(h.ctx) == OK
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        h.drain()
        h.check()
        calls = h.calls()
        assert [c["n"] for c in calls] == [3, 1, 2, 1, 1, 2, 1, 1, 1, 1], [c["n"] for c in calls]
        assert [c["checked"] is not None for c in calls] == [True, True, True, False, True, True, True, True, False, True]
        assert struct.pack("f", calls[1]["checked"]["tau"]) == struct.pack("f", up) != struct.pack("f", calls[0]["checked"]["tau"])
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["chk", "mchk", "cchk", "mcchk"])
def test_a_burst_of_checked_pairs_is_staggered_like_any_other(fq, kind):
    h = Host(fq, 4, 8, poll_delay=10 ** 6)
    try:
        sp = spec(compact=1, min_conf=0.25)
        for k in range(32):
            assert h.enqueue(kind, tau=0.75, back=bool(k & 1), sp=sp) == OK
        assert [c["n"] for c in h.calls()] == [4, 5, 7, 8, 8] == plan(fq, 4, 8, 32), h.calls()
        assert [c["slot"] for c in h.calls()] == [0, 1, 2, 3, 0] and all(c["more"] == 1 for c in h.calls())
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        assert fq.ugsm_flush(h.ctx) == OK
        h.drain()
        h.check()
    finally:
        h.close()


# ---- completions, ugsm_done_checked ---------------------------------------------------------------------------------------------------------
def test_pairs_are_reported_in_enqueue_order_when_a_later_call_finishes_first(fq):
    h = Host(fq, 2, 1, poll_delay=6)
    try:
        assert h.enqueue("mcchk", sp=spec()) == OK                 # call 0: six polls per drain, two drains
        fq.ugsm_fake_poll_delay(h.ctx, 0)
        assert h.enqueue("chk") == OK                              # call 1: finishes at once
        assert h.next_done(0) == PENDING and h.reported == []
        assert h.call(1)["checked"]["marks"] == 0                  # not retired, its counts not read, before the call in front of it
        h.drain()
        h.check()
        assert h.reported == [0, 1]
    finally:
        h.close()


def test_done_checked_answers_for_the_pair_just_reported_only(fq):
    h = Host(fq, 2, 2)
    try:
        st, _ = h.done_checked()
        assert st == STATE                                         # 1. nothing reported yet
        assert fq.ugsm_done_checked(h.ctx, None) == BAD_ARG and fq.ugsm_done_checked(None, C.byref(CheckedResult())) == BAD_ARG
        fq.ugsm_fake_fail_call(h.ctx, 2, DEVICE)
        for kind in ("mchk", "full", "chk", "chk"):                # calls: [mchk], [full], [chk] -- told to fail --, [chk]
            assert h.enqueue(kind) == OK
            assert fq.ugsm_flush(h.ctx) == OK
        assert h.next_done(1) == OK and h.reported == [0] and h.marks[0] == (1000, 2000)     # (next_done asserts what ugsm_done_checked says)
        assert h.next_done(1) == OK and h.reported == [0, 1]       # 2. the last pair was not a checked pair
        assert h.done_checked()[0] == STATE
        assert h.next_done(1) == OK and h.status[2] == DEVICE      # 3. its call failed
        assert h.done_checked()[0] == STATE
        assert h.next_done(1) == OK and h.status[3] == OK and h.done_checked()[0] == OK
        assert h.next_done(1) == EMPTY
        assert h.done_checked()[0] == OK                           # (EMPTY reported nothing: the answer stands)
        h.check()
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["chk", "mchk", "mcchk"])
def test_a_failed_call_reports_every_pair_once_after_the_drain(fq, kind):
    h = Host(fq, 2, 3, poll_delay=2)
    try:
        fq.ugsm_fake_fail_call(h.ctx, 1, NOMEM)
        for _ in range(8):
            assert h.enqueue(kind, sp=spec()) == OK
        assert fq.ugsm_flush(h.ctx) == OK
        h.drain()                                                  # (next_done asserts `drained` for every completion, the failed call's too)
        h.check()
        calls = h.calls()
        failed = [t for t in h.accepted if h.status[t] != OK]
        assert len(failed) == calls[1]["n"] and all(h.status[t] == NOMEM for t in failed), (failed, calls)
        assert calls[1]["checked"]["marks"] == 0
    finally:
        h.close()


def test_the_outstanding_limit(fq):
    h = Host(fq, 1, 2)
    try:
        for k in range(4):                                         # (slots + 1) x batch = 4
            assert h.enqueue("chk" if k & 1 else "mchk") == OK
        before = h.depth()
        assert sum(before) == 4
        for kind in ("chk", "mchk", "cchk", "mcchk"):
            assert h.enqueue(kind, sp=spec()) == STATE
            assert fq.ugsm_last_error(h.ctx).decode() == M_FULL
        assert h.depth() == before
        assert h.next_done(1) == OK
        assert h.enqueue("chk") == OK
        h.drain()
        h.check()
    finally:
        h.close()


# ---- host allocation failures ---------------------------------------------------------------------------------------------------------------
def scenario(h):
    kinds = [("mchk", True)] * 5 + [("mchk", False)] * 2 + [("mcchk", True)] * 3 + [("chk", True)] * 2
    for kind, back in kinds + kinds[:7]:
        h.enqueue(kind, back=back, sp=spec(want_planes=1))
        for _ in range(2):
            if h.next_done(0) != OK:
                break
    h.lib.ugsm_flush(h.ctx)


def test_host_allocation_failures_lose_no_checked_pair_and_leave_the_queue_usable(fq):
    """The same host program -- a managed burst with want_back, some cloud pairs, some device pairs -- with the 1st, 2nd, 3rd ... host
    allocation inside the library failing: an entry point may answer UGSM_ERR_NOMEM, a call may be reported as failed; every pair whose enqueue
    answered UGSM_OK is reported exactly once, in order, and afterwards the same context takes and reports another burst."""
    h = Host(fq, 2, 3, poll_delay=1)
    a0 = fq.ugsm_fake_allocs()
    scenario(h)
    h.drain()
    h.check()
    n_allocs = fq.ugsm_fake_allocs() - a0
    assert len(h.accepted) == 19
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
            refused += len(h.accepted) < 19
            failed += any(s != OK for s in h.status.values())
            first = len(h.accepted)
            scenario(h)                                            # usable afterwards: nothing fails now
            h.drain()
            assert len(h.accepted) == first + 19 and h.reported == h.accepted and all(h.status[t] == OK for t in h.accepted[first:]), k
            assert fq.ugsm_fake_violations(h.ctx) == 0 and h.depth() == (0, 0, 0)
        finally:
            h.close()
    assert refused > 3 and failed > 0, (refused, failed)


# ---- marshalling ----------------------------------------------------------------------------------------------------------------------------
def _jobs(fq, ctx, k):
    head, pairs, jobs, p1, reserved = (C.c_longlong * 7)(), (C.c_longlong * (9 * 16))(), (C.c_longlong * (13 * 16))(), C.c_double(), C.c_int(-1)
    assert fq.ugsm_fake_call_args(ctx, k, C.byref(head), C.byref(pairs)) == 0
    assert fq.ugsm_fake_checked_jobs(ctx, k, C.byref(jobs), C.byref(p1), C.byref(reserved)) == 0
    v, tau = (C.c_int * 6)(), C.c_float()
    assert fq.ugsm_fake_checked_call(ctx, k, C.byref(v), C.byref(tau)) == 0
    rec = dict(zip(("entry", "W", "H", "stride", "fmt", "pyr_arrays", "n"), head))
    rec.update(p1=p1.value, reserved=reserved.value, tau=tau.value, managed=v[0], has_spec=v[2], want_planes=v[4])
    rec["jobs"] = [list(jobs[13 * b:13 * b + 13]) for b in range(rec["n"])]
    return rec


def test_checked_marshalling(fq):
    """Every checked call the hook receives carries exactly what its pairs were enqueued with: L, R, d_out, d_back (NULL where the pair gave
    none), tau, the spec with `reserved` cleared and the cloud buffers, pair by pair in enqueue order; a managed pair's images, planes, back
    planes and completion are its staging buffer's carve-up."""
    ctx = fq.ugsm_fake_create_checked(2, 3, 8, 4, 3)
    want, images, done, staged, backs = {}, {}, [], {}, {}
    GW, GH = 64, 32

    def enqueue(kind, tau, back, want_planes=0):
        tag = len(want)
        sp = spec(p1=3.5, want_planes=want_planes, max_points=50)
        sp.reserved = 7
        p = BASE + 4096 * tag
        L, R, out, bk, points, count, cap = p, p + 64, p + 128, (p + 192 if back else 0), p + 256, p + 512, 5000 + tag
        managed, cloud = kind in ("mchk", "mcchk"), kind in ("cchk", "mcchk")
        w = dict(kind=kind, tau=tau, back=back, managed=managed, cloud=cloud, want_planes=want_planes, stride=3 * GW + 8)
        if kind == "chk":
            st = fq.ugsm_enqueue_full_checked(ctx, L, R, GW, GH, 3 * GW + 8, out, bk or None, tau, tag)
            w["job"] = [L, R, out, bk, 0, 0, 0, 0, 0, 0, 0, 0, 0]
        elif kind == "cchk":
            st = fq.ugsm_enqueue_full_checked_cloud(ctx, L, R, GW, GH, 3 * GW + 8, out, bk or None, tau, C.byref(sp), points, cap, count, tag)
            w["job"] = [L, R, out, bk, 0, 0, 0, 0, 0, 0, points, cap, count]
        else:
            img = np.random.RandomState(tag).randint(0, 256, (2, GH, 3 * GW + 8)).astype(np.uint8)
            img[0].reshape(-1)[:4].view(np.uint32)[0] = tag
            images[tag] = [img[s][:, :3 * GW].tobytes() for s in range(2)]
            w["stride"] = 3 * GW
            if kind == "mchk":
                st = fq.ugsm_enqueue_full_checked_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, GW, GH, 3 * GW + 8, tau, int(back), tag)
            else:
                st = fq.ugsm_enqueue_full_checked_cloud_managed(ctx, img[0].ctypes.data, img[1].ctypes.data, GW, GH, 3 * GW + 8, tau, int(back), C.byref(sp), tag)
            img[:] = 0                                             # (copied before the call returned)
        sp.reserved, sp.want_planes = 9, 1 - want_planes           # (the spec was copied at enqueue)
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
            r = CheckedResult()
            assert fq.ugsm_done_checked(ctx, C.byref(r)) == OK
            backs[tag] = [C.cast(r.back[j], C.c_void_p).value or 0 for j in range(3)]
            if want[tag]["managed"]:                               # the staging is lent until the next ugsm_next_done: look now
                job = _jobs(fq, ctx, k)["jobs"][b]
                staged[tag] = [C.string_at(job[0], 3 * GW * GH), C.string_at(job[1], 3 * GW * GH)]
                assert (r.marked_fwd, r.marked_back) == (tag + 1000, tag + 2000)

    try:
        # (two slots, calls of up to three: the first call after idle or a flush takes two pairs, the later ones three)
        enqueue("chk", 1.0, True), enqueue("chk", 1.0, False), enqueue("chk", 1.0, False), enqueue("chk", 1.0, True), enqueue("chk", 1.0, True), drain()
        enqueue("chk", 0.25, False), drain()
        enqueue("cchk", 0.5, False), enqueue("cchk", 0.5, True), enqueue("cchk", 0.5, False), drain()
        enqueue("mchk", 2.0, True), enqueue("mchk", 2.0, False), enqueue("mchk", 2.0, True), enqueue("mchk", 2.0, False), enqueue("mchk", 2.0, True), drain()
        for wp in (0, 1):
            enqueue("mcchk", 1.5, True, wp), enqueue("mcchk", 1.5, False, wp), enqueue("mcchk", 1.5, True, wp), drain()
        assert fq.ugsm_fake_violations(ctx) == 0
        assert [t for t, _, _ in done] == list(range(len(want)))
        ncalls = fq.ugsm_fake_calls(ctx)
        assert sorted({k for _, k, _ in done}) == list(range(ncalls))
        seen = set()
        for k in range(ncalls):
            rec = _jobs(fq, ctx, k)
            tags = [t for t, kk, _ in done if kk == k]
            results = [r for _, kk, r in done if kk == k]
            n, w0 = rec["n"], want[tags[0]]
            assert n == len(tags) and tags == list(range(tags[0], tags[0] + n)), (k, rec, tags)
            assert rec["entry"] == E_CHECKED + (E_HOST if w0["managed"] else 0) + (E_CLOUD if w0["cloud"] else 0), (k, rec)
            assert (rec["W"], rec["H"], rec["stride"], rec["fmt"]) == (GW, GH, w0["stride"], 0), (k, rec)
            assert (rec["tau"], rec["managed"], rec["has_spec"]) == (w0["tau"], int(w0["managed"]), int(w0["cloud"])), (k, rec)
            if w0["cloud"]:
                assert (rec["p1"], rec["reserved"], rec["want_planes"]) == (3.5, 0, w0["want_planes"]), (k, rec)
            for t, job, res in zip(tags, rec["jobs"], results):
                w = want[t]
                assert (w["kind"], w["tau"]) == (w0["kind"], w0["tau"])
                if not w["managed"]:
                    assert job == w["job"], (k, t, job, w["job"])
                    assert res == [0] * 5 and backs[t] == [0, 0, 0]
                else:
                    img = (3 * GW * GH + 255) & ~255
                    plane = GW * GH * 4
                    L = job[0]
                    has_planes = (not w["cloud"]) or w["want_planes"]
                    planes = [res[0] + j * plane for j in range(3)] if has_planes else [0, 0, 0]
                    assert L and bool(res[0]) == bool(has_planes)
                    bp = backs[t]
                    assert bool(bp[0]) == w["back"]
                    if w["back"]:
                        assert bp == [bp[0] + j * plane for j in range(3)]
                        if has_planes:
                            assert bp[0] == res[0] + 3 * plane                 # one staging buffer: the back planes behind the forward ones
                    assert job == [L, L + img, 0, 0] + planes + bp + [0, 0, 0], (k, t, job)
                    assert res == planes + [0, 0], (t, res)
                    assert staged[t] == images[t], (k, t)
                seen.add((w["kind"], n > 1, w["back"]))
        assert {(kind, many) for kind, many, _ in seen} >= {(kind, True) for kind in ("chk", "cchk", "mchk", "mcchk")} | {("chk", False)}, seen
        assert {(kind, back) for kind, _, back in seen} == {(kind, back) for kind in ("chk", "cchk", "mchk", "mcchk") for back in (False, True)}
    finally:
        fq.ugsm_fake_destroy_checked(ctx)


# ---- the refusals, in their order -----------------------------------------------------------------------------------------------------------
M_NULL = "ugsm_enqueue_%s: null buffer"
M_NULL_MANAGED = "ugsm_enqueue_*_managed: null image"
M_SIZE = "ugsm_enqueue_*: bad image size for the context's pyramid"
M_STRIDE = "ugsm_enqueue_*: stride < bytes per pixel of the input format * W"
M_TAU = "ugsm_enqueue_full_checked*: tau must be > 0"
M_CONFIG = "ugsm_enqueue_full_checked*: not with early_exit_threshold > 0 or kernel_path 1"
M_NO_CHECKED = "ugsm_enqueue_full_checked*: this runtime has no checked full-mode call"
M_SPEC = "ugsm_enqueue_*_cloud*: null spec"
M_SAMPLING = "ugsm_enqueue_*_cloud*: sampling < 1 or an unknown record format"
M_MAX_POINTS = "ugsm_enqueue_*_cloud*: max_points < 0"
M_BUFFERS = "ugsm_enqueue_*_cloud: a null or misaligned cloud buffer, or cap_points < 0"
M_NO_CLOUDS = "ugsm_enqueue_*_cloud*: this runtime makes no clouds"
M_FULL = ("ugsm_enqueue_*: (slots + 1) x batch pairs are outstanding and completions wait to be fetched: "
          "call ugsm_next_done first")

ENTRY_POINTS = {
    "full_checked": lambda q, c, a: q.ugsm_enqueue_full_checked(c, a.L, a.R, a.W, a.H, a.stride, a.o0, a.back, a.tau, a.tag),
    "full_checked_managed": lambda q, c, a: q.ugsm_enqueue_full_checked_managed(c, a.L, a.R, a.W, a.H, a.stride, a.tau, 1, a.tag),
    "full_checked_cloud": lambda q, c, a: q.ugsm_enqueue_full_checked_cloud(c, a.L, a.R, a.W, a.H, a.stride, a.o0, a.back, a.tau, a.spec, a.points, a.cap,
                                                                           a.count, a.tag),
    "full_checked_cloud_managed": lambda q, c, a: q.ugsm_enqueue_full_checked_cloud_managed(c, a.L, a.R, a.W, a.H, a.stride, a.tau, 1, a.spec, a.tag),
}


def refusals(name):
    """(what, context, arguments that differ from a good call, status, message): where two refusals apply at once the one named first wins."""
    managed, cloud = name.endswith("managed"), "cloud" in name
    null = M_NULL_MANAGED if managed else M_NULL % name
    small, tiny, nan = dict(stride=3 * 64 - 1), dict(W=8), float("nan")
    out = [("null left image", "good", dict(L=None), BAD_ARG, null), ("null right image", "good", dict(R=None), BAD_ARG, null),
           ("null image, then tau", "good", dict(R=None, tau=0.0), BAD_ARG, null),
           ("size", "good", tiny, BAD_ARG, M_SIZE), ("size, then tau", "good", dict(tiny, tau=-1.0), BAD_ARG, M_SIZE),
           ("stride", "good", small, SIZE_MISMATCH, M_STRIDE), ("stride, then tau", "good", dict(small, tau=nan), SIZE_MISMATCH, M_STRIDE),
           ("tau 0", "good", dict(tau=0.0), BAD_ARG, M_TAU), ("tau < 0", "good", dict(tau=-0.5), BAD_ARG, M_TAU), ("tau NaN", "good", dict(tau=nan), BAD_ARG, M_TAU),
           ("tau, then early exit", "early exit", dict(tau=0.0), BAD_ARG, M_TAU), ("tau, then no hooks", "no checked", dict(tau=nan), BAD_ARG, M_TAU),
           ("tau, then full queue", "full", dict(tau=0.0), BAD_ARG, M_TAU),
           ("early exit", "early exit", {}, BAD_ARG, M_CONFIG), ("kernel path 1", "kernel path", {}, BAD_ARG, M_CONFIG),
           ("stride, then early exit", "early exit", small, SIZE_MISMATCH, M_STRIDE),
           ("no checked hooks", "no checked", {}, STATE, M_NO_CHECKED), ("no checked hooks, then full queue", "no checked, full", {}, STATE, M_NO_CHECKED),
           ("stride, then full queue", "full", small, SIZE_MISMATCH, M_STRIDE), ("full queue", "full", {}, STATE, M_FULL)]
    if not managed:
        out += [("null d_out", "good", dict(o0=None), BAD_ARG, null), ("null d_out, then tau", "good", dict(o0=None, tau=0.0), BAD_ARG, null)]
    if cloud:
        out += [("tau, then null spec", "good", dict(tau=0.0, spec=None), BAD_ARG, M_TAU), ("early exit, then null spec", "early exit", dict(spec=None), BAD_ARG, M_CONFIG),
                ("no checked hooks, then null spec", "no checked", dict(spec=None), STATE, M_NO_CHECKED),
                ("null spec", "good", dict(spec=None), BAD_ARG, M_SPEC), ("sampling 0", "good", dict(spec=spec(sampling=0)), BAD_ARG, M_SAMPLING),
                ("max_points, then no cloud hooks", "no clouds", dict(spec=spec(max_points=-1)), BAD_ARG, M_MAX_POINTS),
                ("no cloud hooks", "no clouds", {}, STATE, M_NO_CLOUDS), ("null spec, then full queue", "full", dict(spec=None), BAD_ARG, M_SPEC)]
        if not managed:
            out += [("misaligned d_points", "good", dict(points=BASE + 8), BAD_ARG, M_BUFFERS), ("null d_count", "good", dict(count=None), BAD_ARG, M_BUFFERS),
                    ("tau, then misaligned d_points", "good", dict(tau=0.0, points=BASE + 8), BAD_ARG, M_TAU),
                    ("misaligned d_points, then full queue", "full", dict(points=BASE + 8), BAD_ARG, M_BUFFERS)]
    return out


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_every_checked_entry_point_refuses_in_order_with_its_message(fq, name):
    call = ENTRY_POINTS[name]
    images = np.zeros((2, 32, 3 * 64), np.uint8)      # (real memory: the managed kinds read their images once a pair is accepted)

    def arguments(**over):
        a = types.SimpleNamespace(L=images[0].ctypes.data, R=images[1].ctypes.data, W=64, H=32, stride=3 * 64, o0=BASE + 128, back=None, tau=1.0,
                                  spec=spec(), points=BASE + 1024, cap=10, count=BASE + 2048, tag=77)
        vars(a).update(over)
        a.spec = C.byref(a.spec) if a.spec is not None else None
        return a

    def depth(ctx):
        w, f, u = C.c_int(), C.c_int(), C.c_int()
        assert fq.ugsm_queue_depth(ctx, C.byref(w), C.byref(f), C.byref(u)) == OK
        return w.value, f.value, u.value

    def context(kind):
        full = kind.endswith("full")
        ctx = fq.ugsm_fake_create_checked(1 if full else 2, 1 if full else 3, 8, 4, 1 if kind.startswith("no checked") else 2 if kind == "no clouds" else 3)
        assert ctx
        if kind == "early exit":
            fq.ugsm_fake_set_config(ctx, 0.5, 0)
        if kind == "kernel path":
            fq.ugsm_fake_set_config(ctx, 0.0, 1)
        for tag in range(2 if full else 0):           # (slots + 1) x batch = 2 pairs outstanding
            assert fq.ugsm_enqueue_full(ctx, BASE, BASE + 64, 64, 32, 3 * 64, BASE + 128, tag) == OK
        return ctx

    assert call(fq, None, arguments()) == BAD_ARG                                        # no context: no message either
    ctxs = {}
    try:
        for what, kind, over, status, message in refusals(name):
            ctx = ctxs[kind] = ctxs.get(kind) or context(kind)
            before, allocs = depth(ctx), fq.ugsm_fake_allocs()
            st = call(fq, ctx, arguments(**over))
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
            assert fq.ugsm_fake_calls(ctx) == len(tags)
        assert call(fq, ctxs["good"], arguments()) == OK, (name, fq.ugsm_last_error(ctxs["good"]))   # the good call of the table is one
        c = Completion()
        assert fq.ugsm_next_done(ctxs["good"], C.byref(c), 1) == OK and c.tag == 77 and c.status == OK
        # plain pairs do not care about the checked hooks or the configuration the checked pairs are refused for
        for kind in ("no checked", "early exit", "kernel path"):
            assert fq.ugsm_enqueue_full(ctxs[kind], BASE, BASE + 64, 64, 32, 3 * 64, BASE + 128, 5) == OK
            assert fq.ugsm_next_done(ctxs[kind], C.byref(c), 1) == OK and c.tag == 5 and c.status == OK
    finally:
        for ctx in ctxs.values():
            fq.ugsm_fake_destroy_checked(ctx)


def test_the_queue_still_links_against_the_fakes_that_know_no_checked_call(tmp_path):
    """tests/fake_runtime.cpp and tests/fake_runtime_cloud.cpp define neither ugsm_submit_full_checked* nor ugsm_last_lr_marked_pair: the queue
    reaches the checked call through hooks only, so their shared objects still build and load with every symbol resolved at once -- and there
    the new entry points refuse with UGSM_ERR_STATE."""
    for fake in ("fake_runtime.cpp", "fake_runtime_cloud.cpp"):
        lib = C.CDLL(build(tmp_path, (fake,)), mode=os.RTLD_NOW)
        for name in ("ugsm_enqueue_full_checked", "ugsm_enqueue_full_checked_managed", "ugsm_enqueue_full_checked_cloud",
                     "ugsm_enqueue_full_checked_cloud_managed", "ugsm_done_checked"):
            assert hasattr(lib, name), name
    lib.ugsm_fake_create_cloud.restype = C.c_void_p
    lib.ugsm_fake_create_cloud.argtypes = [C.c_int] * 5
    lib.ugsm_enqueue_full_checked.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_uint64]
    lib.ugsm_last_error.argtypes = [C.c_void_p]
    lib.ugsm_last_error.restype = C.c_char_p
    lib.ugsm_fake_destroy_cloud.argtypes = [C.c_void_p]
    ctx = lib.ugsm_fake_create_cloud(2, 2, 8, 4, 1)
    try:
        assert lib.ugsm_enqueue_full_checked(ctx, BASE, BASE + 64, 64, 32, 192, BASE + 128, None, 1.0, 1) == STATE
        assert lib.ugsm_last_error(ctx).decode() == M_NO_CHECKED
    finally:
        lib.ugsm_fake_destroy_cloud(ctx)


# ---- the sanitizer run: a stand-alone program, on the CPU ----------------------------------------------------------------------------------
def test_sixty_mixed_pairs_under_address_and_undefined_sanitizers(tmp_path):
    """tests/queue_checked_sanitize.cpp -- its own main, the queue and the fakes, about sixty mixed pairs, the same burst again under every
    single host allocation failure -- built with -fsanitize=address,undefined and run as a program of its own (nothing is loaded into Python):
    no report, no leak, and every accepted pair reported once."""
    exe = str(tmp_path / "queue_checked_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "queue_checked_sanitize.cpp"), os.path.join(CSRC, "ugsm_queue.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "ok:" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
