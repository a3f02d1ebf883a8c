"""The queue (round 5): ugsm_enqueue_* / ugsm_flush / ugsm_next_done -- the library owns the slots, forms calls from the
backlog, rotates slots and reports completions in enqueue order.

Whatever calls the library forms, EVERY pair must equal the CPU oracle's answer for that pair bit for bit; the calls it forms must be the
ones ugsm_queue_plan predicts (the rule bench.py's plan_calls had in rounds 3-4); and at 16 MP the configuration bench.py times -- four
slots, batch 8, a burst of 20 pairs -> calls of 4 / 5 / 7 / 4 -- is compared pair by pair with the live oracle, plus one explicit call of
eight.  Reference call pattern this replaces: UG_GPU_matcher.cpp:126-185,414-494 (one blocking match() per callback, :749-752).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def _pairs(W, H, n, seed0):
    from ug_stereomatcher_amd import synth
    return [synth.make_pair(W, H, synth.BASE_SEED + seed0 + 5 * j)[:2] for j in range(n)]


def _calls_of(done):
    """[(call_index, call_pairs)] in order, from a list of completions in enqueue order."""
    out = []
    for c in done:
        if not out or out[-1][0] != c.call_index:
            out.append((c.call_index, c.call_pairs))
    return out


@pytest.mark.parametrize("slots,B,n", [(4, 4, 20), (2, 8, 21), (1, 1, 3), (3, 16, 40)])
def test_burst_of_full_pairs_vs_oracle(lib, orc, slots, B, n):
    """A burst of n different pairs, then a flush: calls as ugsm_queue_plan says, completions in enqueue order with the host's tags,
    every pair bit-equal to the oracle."""
    W, H, lv = 333, 251, 10
    uniq = _pairs(W, H, 5, 900 + slots)
    exp = [orc.match_full(L, R, lv) for L, R in uniq]
    with lib.Context(levels=lv, slots=slots, batch=B) as c:
        dL = [c.to_device(L) for L, _ in uniq]
        dR = [c.to_device(R) for _, R in uniq]
        cap = (slots + 1) * B
        ring = [c.alloc(3 * W * H * 4) for _ in range(cap)]
        got, done = {}, []

        def fetch(block):
            while True:
                d = c.next_done(block)
                if d is None:
                    return
                done.append(d)
                got[d.tag] = c.to_host(ring[d.tag % cap], (3, H, W))   # read before the ring comes round to this buffer again
        for k in range(n):
            c.enqueue_full(dL[k % 5], dR[k % 5], W, H, 3 * W, ring[k % cap], k)
            fetch(False)
        c.flush()
        fetch(True)
        assert [d.tag for d in done] == list(range(n))
        assert [s for _, s in _calls_of(done)] == lib.queue_plan(n, slots=slots, batch=B)
        assert all(d.status == 0 and 0 <= d.slot < slots and d.done_ns > 0 for d in done)
        assert c.queue_depth() == (0, 0, 0)
        for k in range(n):
            assert_bit_equal(got[k], exp[k % 5], f"queue, slots={slots} batch={B}, pair {k}")
        # nothing outstanding: the slot-level entry points work again
        c.check(c.lib.ugsm_submit_full(c.handle, 0, dL[0], dR[0], W, H, 3 * W, ring[0]))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert_bit_equal(c.to_host(ring[0], (3, H, W)), exp[0], "slot-level call after the queue drained")
        for p in dL + dR + ring:
            c.free(p)


def test_trickle_flush_after_every_pair(lib, orc):
    """A host that flushes after every enqueue: calls of one pair while slots are free, larger ones once they are all busy."""
    W, H, lv, slots, B = 640, 480, 12, 2, 4
    uniq = _pairs(W, H, 3, 950)
    exp = [orc.match_full(L, R, lv) for L, R in uniq]
    with lib.Context(levels=lv, slots=slots, batch=B) as c:
        dL = [c.to_device(L) for L, _ in uniq]
        dR = [c.to_device(R) for _, R in uniq]
        cap = (slots + 1) * B
        ring = [c.alloc(3 * W * H * 4) for _ in range(cap)]
        done, got = [], {}
        n = 14
        for k in range(n):
            c.enqueue_full(dL[k % 3], dR[k % 3], W, H, 3 * W, ring[k % cap], k)
            c.flush()
            while True:
                d = c.next_done(False)
                if d is None:
                    break
                done.append(d)
                got[d.tag] = c.to_host(ring[d.tag % cap], (3, H, W))
        for d in c.drain():
            done.append(d)
            got[d.tag] = c.to_host(ring[d.tag % cap], (3, H, W))
        assert [d.tag for d in done] == list(range(n))
        sizes = [s for _, s in _calls_of(done)]
        assert sizes[0] == 1 and sizes[1] == 1 and sum(sizes) == n and max(sizes) <= B, sizes
        for k in range(n):
            assert_bit_equal(got[k], exp[k % 3], f"trickle, pair {k}")
        for p in dL + dR + ring:
            c.free(p)


def test_foveated_pairs_with_offsets_and_pyramid_stacks(lib, orc):
    W, H, lv, F = 640, 480, 12, 5
    fw, fh = lib.fovea_dims(W, H, lv, F)
    uniq = _pairs(W, H, 2, 960)
    offs = [(0, 0), (60, -40), (-300, 200), (5, 7), (1000, 1000), (-9, 30), (0, 0)]
    with lib.Context(levels=lv, fovea_levels=F, slots=2, batch=4) as c:
        dL = [c.to_device(L) for L, _ in uniq]
        dR = [c.to_device(R) for _, R in uniq]
        n = len(offs)
        dS = [c.alloc(3 * F * fh * fw * 4) for _ in range(n)]
        dP = [(c.alloc(3 * F * fh * fw * 4), c.alloc(3 * F * fh * fw * 4)) if k % 3 == 0 else (None, None) for k in range(n)]
        for k in range(n):
            c.enqueue_foveated(dL[k % 2], dR[k % 2], W, H, 3 * W, offs[k], dS[k], k, dP[k][0], dP[k][1])
        done = c.drain()
        assert [d.tag for d in done] == list(range(n))
        assert [s for _, s in _calls_of(done)] == lib.queue_plan(n, slots=2, batch=4)
        for k in range(n):
            L, R = uniq[k % 2]
            st, pl, pr = orc.match_foveated(L, R, lv, F, offs[k][0], offs[k][1], want_pyr=True)
            assert_bit_equal(c.to_host(dS[k], (3, F, fh, fw)), st, f"foveated queue, pair {k} at {offs[k]}")
            if dP[k][0] is not None:
                assert_bit_equal(c.to_host(dP[k][0], (F, 3, fh, fw)), pl, f"left pyramid stack, pair {k}")
                assert_bit_equal(c.to_host(dP[k][1], (F, 3, fh, fw)), pr, f"right pyramid stack, pair {k}")
        for p in dL + dR + dS + [q for pq in dP for q in pq if q is not None]:
            c.free(p)


def test_pairs_of_different_kinds_go_out_in_calls_of_their_own(lib, orc):
    """Two image sizes and both modes interleaved in one backlog: a call holds pairs of one kind; order and results are kept."""
    lv, F = 9, 4
    A = _pairs(320, 240, 2, 970)
    Bp = _pairs(200, 150, 2, 975)
    with lib.Context(levels=lv, fovea_levels=F, slots=2, batch=4) as c:
        plan = [("fA", 0), ("fA", 1), ("fB", 0), ("vA", 0), ("vA", 1), ("fA", 0), ("fB", 1), ("fB", 0), ("fB", 1), ("fB", 0), ("fB", 1)]
        bufs, outs = [], []
        dev = {}
        for name, pairs in (("A", A), ("B", Bp)):
            for j, (L, R) in enumerate(pairs):
                dev[(name, j)] = (c.to_device(L), c.to_device(R), L, R)
        for k, (kind, j) in enumerate(plan):
            name = kind[1]
            W, H = (320, 240) if name == "A" else (200, 150)
            dL, dR, L, R = dev[(name, j)]
            if kind[0] == "f":
                o = c.alloc(3 * W * H * 4)
                c.enqueue_full(dL, dR, W, H, 3 * W, o, k)
                outs.append((o, (3, H, W), orc.match_full(L, R, lv)))
            else:
                fw, fh = lib.fovea_dims(W, H, lv, F)
                o = c.alloc(3 * F * fw * fh * 4)
                c.enqueue_foveated(dL, dR, W, H, 3 * W, (0, 0), o, k)
                outs.append((o, (3, F, fh, fw), orc.match_foveated(L, R, lv, F)[0]))
        done = c.drain()
        assert [d.tag for d in done] == list(range(len(plan)))
        # kinds: fA fA | fB | vA vA | fA | fB x5 (first-round stagger for batch 4 on two slots: 3, 4 -> the last group splits 3 + 2 or by what slots allow)
        sizes = [s for _, s in _calls_of(done)]
        assert sizes[:4] == [2, 1, 2, 1] and sum(sizes) == len(plan), sizes
        for k, (o, shp, exp) in enumerate(outs):
            assert_bit_equal(c.to_host(o, shp), exp, f"mixed kinds, pair {k} ({plan[k][0]})")
        for o, _, _ in outs:
            c.free(o)
        for dL, dR, _, _ in dev.values():
            c.free(dL)
            c.free(dR)


def test_host_and_managed_memory(lib, orc):
    """ugsm_enqueue_full_host (page-locked buffers of the caller) and ugsm_enqueue_*_managed (any memory in, library-owned planes out)."""
    W, H, lv, F = 333, 251, 10, 4
    fw, fh = lib.fovea_dims(W, H, lv, F)
    uniq = _pairs(W, H, 3, 980)
    exp = [orc.match_full(L, R, lv) for L, R in uniq]
    with lib.Context(levels=lv, fovea_levels=F, slots=2, batch=2) as c:
        n = 5
        pin = []
        for k in range(n):
            L, R = uniq[k % 3]
            pl, pr, po = c.host_array(L.shape, L.dtype), c.host_array(R.shape, R.dtype), c.host_array((3, H, W))
            pl[...] = L
            pr[...] = R
            po[...] = -1.0
            pin.append((pl, pr, po))
            c.enqueue_full_host(pl, pr, po, k)
        done = c.drain()
        assert [d.tag for d in done] == list(range(n))
        for k in range(n):
            assert_bit_equal(pin[k][2], exp[k % 3], f"page-locked host queue, pair {k}")
        # pageable memory through the _host entry: refused, nothing enqueued
        L, R = uniq[0]
        out = np.empty((3, H, W), np.float32)
        st = c.lib.ugsm_enqueue_full_host(c.handle, L.ctypes.data, R.ctypes.data, W, H, 3 * W, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, 7)
        assert st == lib.UGSM_ERR_BAD_ARG and c.queue_depth() == (0, 0, 0)
        # managed: ordinary numpy arrays (a padded stride for one of them), the caller's images overwritten right after the call
        for k in range(n):
            L, R = uniq[k % 3]
            if k == 1:
                Lp = np.zeros((H, W + 5, 3), np.uint8)
                Lp[:, :W] = L
                Rp = np.zeros((H, W + 5, 3), np.uint8)
                Rp[:, :W] = R
                c.check(c.lib.ugsm_enqueue_full_managed(c.handle, Lp.ctypes.data, Rp.ctypes.data, W, H, Lp.strides[0], 100 + k))
                Lp[...] = 0
                Rp[...] = 0
            else:
                Lc, Rc = L.copy(), R.copy()
                c.enqueue_full_managed(Lc, Rc, 100 + k)
                Lc[...] = 0
                Rc[...] = 0
        c.flush()
        for k in range(n):
            d = c.next_done(True)
            assert d.tag == 100 + k
            h, v, cf = c.managed_planes(d, [(H, W)] * 3)
            assert_bit_equal(np.stack([h, v, cf]), exp[k % 3], f"managed queue, pair {k}")
        assert c.next_done(True) is None
        # managed foveated with the pyramid stacks (what the node's topic path publishes, UG_GPU_matcher.cpp:203-320)
        for k, off in enumerate([(0, 0), (40, -25)]):
            L, R = uniq[k]
            c.enqueue_foveated_managed(L, R, off, True, 200 + k)
        c.flush()
        for k, off in enumerate([(0, 0), (40, -25)]):
            d = c.next_done(True)
            assert d.tag == 200 + k
            L, R = uniq[k]
            st, pl, pr = orc.match_foveated(L, R, lv, F, off[0], off[1], want_pyr=True)
            sh, sv, sc, gl, gr = c.managed_planes(d, [(F, fh, fw)] * 3 + [(F, 3, fh, fw)] * 2)
            assert_bit_equal(np.stack([sh, sv, sc]), st, f"managed foveated, pair {k}")
            assert_bit_equal(gl, pl, "managed left pyramid stack")
            assert_bit_equal(gr, pr, "managed right pyramid stack")
        assert c.next_done(False) is None and c.queue_depth() == (0, 0, 0)


def test_queue_errors_and_back_pressure(lib):
    from ug_stereomatcher_amd import synth
    W, H, lv = 160, 120, 8
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 990)
    with lib.Context(levels=lv, slots=2, batch=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        cap = 3 * 2
        ring = [c.alloc(3 * W * H * 4) for _ in range(cap)]
        comp = lib.Completion()
        assert c.lib.ugsm_next_done(c.handle, C.byref(comp), 0) == lib.UGSM_EMPTY
        assert c.lib.ugsm_next_done(c.handle, C.byref(comp), 1) == lib.UGSM_EMPTY
        assert c.lib.ugsm_enqueue_full(c.handle, None, dR, W, H, 3 * W, ring[0], 0) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_enqueue_full(c.handle, dL, dR, W, H, 3 * W - 1, ring[0], 0) == lib.UGSM_ERR_SIZE_MISMATCH
        assert c.lib.ugsm_enqueue_full(c.handle, dL, dR, 3, 2, 9, ring[0], 0) == lib.UGSM_ERR_TOO_SMALL
        assert c.queue_depth() == (0, 0, 0)
        # one pair waits (the first call of a round wants 2 x 2 / 3 -> 2 pairs): not finished, not reportable, and the slots are the queue's
        c.enqueue_full(dL, dR, W, H, 3 * W, ring[0], 0)
        assert c.queue_depth()[0] == 1
        assert c.lib.ugsm_next_done(c.handle, C.byref(comp), 0) == lib.UGSM_PENDING
        assert c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, ring[1]) == lib.UGSM_ERR_STATE
        assert b"queue" in c.lib.ugsm_last_error(c.handle)
        # never fetching: after (slots + 1) x batch pairs the queue refuses instead of letting the ring wrap onto unread results
        for k in range(1, cap):
            c.enqueue_full(dL, dR, W, H, 3 * W, ring[k], k)
        c.flush()
        st = c.lib.ugsm_enqueue_full(c.handle, dL, dR, W, H, 3 * W, ring[0], 99)
        assert st == lib.UGSM_ERR_STATE, st
        done = c.drain()
        assert [d.tag for d in done] == list(range(cap))
        ref = c.to_host(ring[0], (3, H, W))
        for k in range(1, cap):
            assert_bit_equal(c.to_host(ring[k], (3, H, W)), ref, f"pair {k}")
        for p in [dL, dR] + ring:
            c.free(p)


def test_16mp_timed_configuration_vs_oracle(lib, oracle_16mp, oracle_16mp_b):
    """What bench.py times (VERDICT r04 weak #2, next #1b): a four-slot, batch-8 context, a burst of 20 sixteen-megapixel pairs (bench.py's
    two images alternating) -> the library forms calls of 4 / 5 / 7 / 4, all in flight together -- EVERY pair against the live oracle's
    answer for its image, bit for bit.  Then one explicit call of eight on the same context (the full-size call of a long run: levels 1-13
    as one launch for eight pairs)."""
    W, H = oracle_16mp["W"], oracle_16mp["H"]
    imgs = [oracle_16mp, oracle_16mp_b]
    slots, B, n = 4, 8, 20
    assert lib.queue_plan(n, slots=slots, batch=B) == [4, 5, 7, 4]
    with lib.Context(levels=14, slots=slots, batch=B) as c:
        dL = [c.to_device(g["L"]) for g in imgs]
        dR = [c.to_device(g["R"]) for g in imgs]
        outs = [c.alloc(3 * W * H * 4) for _ in range(n)]   # 20 x 193 MB: every result kept
        for k in range(n):
            c.enqueue_full(dL[k % 2], dR[k % 2], W, H, 3 * W, outs[k], k)
        assert c.queue_depth()[0] == 4            # 4 + 5 + 7 went out as they filled; four wait for the flush
        c.flush()
        done = c.drain()
        assert [d.tag for d in done] == list(range(n))
        assert _calls_of(done) == [(0, 4), (1, 5), (2, 7), (3, 4)]
        assert [d.slot for d in done] == [0] * 4 + [1] * 5 + [2] * 7 + [3] * 4
        for k in range(n):
            a = c.to_host(outs[k], (3, H, W))
            assert_bit_equal(a, imgs[k % 2]["full"], f"16 MP, queue-formed calls 4/5/7/4 on four slots, pair {k} vs oracle")
            rmse = float(np.sqrt(np.mean((a[:2].astype(np.float64) - imgs[k % 2]["full"][:2].astype(np.float64)) ** 2)))
            assert rmse == 0.0
            del a
        # an explicit call of eight (ugsm_submit_full_batch), slot 2
        sel = [k % 2 for k in range(8)]
        c.submit_full_batch(2, [dL[j] for j in sel], [dR[j] for j in sel], W, H, 3 * W, outs[:8])
        c.check(c.lib.ugsm_wait(c.handle, 2))
        for k in range(8):
            assert_bit_equal(c.to_host(outs[k], (3, H, W)), imgs[sel[k]]["full"], f"16 MP, one call of eight, pair {k} vs oracle")
        for p in dL + dR + outs:
            c.free(p)


def test_node_mirror_pipelined_topic_path_equals_the_blocking_one(lib):
    """ug_stereomatcher_amd.service.GPUMatcher with frames_in_flight = 3 (VERDICT r04 #1d): the same frames through the blocking topic path
    (one match() per callback, UG_GPU_matcher.cpp:423) and through the pipelined one -- the same messages on the same topics, in arrival
    order, bit for bit; both modes of the node (full and foveated with pyramid stacks); a service call in between drains first."""
    from ug_stereomatcher_amd import service as sv, synth
    W, H = 640, 480
    frames = []
    for k in range(7):
        L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 700 + k)
        hl, hr = sv.Header(seq=k, stamp=100.0 + k, frame_id="left"), sv.Header(seq=k, stamp=100.0 + k, frame_id="right")
        frames.append((sv.Image.from_array(L, "rgb8", hl), sv.Image.from_array(R, "rgb8", hr)))
    for fov in (0, 1):
        logs = {}
        for nfl in (1, 3):
            log = []
            node = sv.GPUMatcher(2, ["node", "x", "5"], params={sv.FOVEATEDQ: fov}, publish=lambda t, m, log=log: log.append((t, m)), frames_in_flight=nfl)
            for k, (iL, iR) in enumerate(frames):
                node.mainRoutine(iL, iR)
                if nfl > 1:
                    assert node._matcher().outstanding() < nfl
                if k == 3:   # a service call while frames are in flight: they are published first, the response is the blocking one
                    rsp = sv.GetDisparitiesGPUResponse()
                    assert node.disparitySrv(sv.GetDisparitiesGPURequest(iL, iR), rsp)
                    assert not node._pending
                    log.append(("srv", rsp.fdispH if fov else rsp.dispH))
            node.drain()
            node._matcher().close()
            logs[nfl] = log
        a, b = logs[1], logs[3]
        assert len(a) == (5 if fov else 3) * 7 + 1
        assert [t for t, _ in a] == [t for t, _ in b]
        for (t, ma), (_, mb) in zip(a, b):
            ia = ma.image_stack if hasattr(ma, "image_stack") else ma.image
            ib = mb.image_stack if hasattr(mb, "image_stack") else mb.image
            assert ma.header == mb.header and ia.height == ib.height and ia.width == ib.width and ia.encoding == ib.encoding
            assert ia.data == ib.data, f"fov={fov}, topic {t}, frame {ma.header.seq}: pipelined and blocking topic paths differ"
            if hasattr(ma, "num_levels"):
                assert (ma.im_width, ma.im_height, ma.roi_width, ma.roi_height, ma.num_levels) == (mb.im_width, mb.im_height, mb.roi_width, mb.roi_height, mb.num_levels)


def test_node_mirror_survives_frames_whose_call_fails(lib, monkeypatch):
    """a failed pair used to stay in MatchGPULib._tags / GPUMatcher._pending for good (Context.next_done raised after the completion
    had been consumed), and after frames_in_flight failed frames the back-pressure loop of mainRoutine never ended.  Every frame's call is
    refused here (UGSM_MEM_LIMIT_MB far below what a 640 x 480 pair needs): every frame is dropped, counted, forgotten -- and nothing hangs."""
    from ug_stereomatcher_amd import service as sv, synth
    monkeypatch.setenv("UGSM_MEM_LIMIT_MB", "4")
    W, H = 640, 480
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 760)
    log = []
    node = sv.GPUMatcher(2, ["node", "x", "5"], params={sv.FOVEATEDQ: 0}, publish=lambda t, m: log.append(t), frames_in_flight=2)
    try:
        for k in range(5):
            hl, hr = sv.Header(seq=k, stamp=1.0 + k, frame_id="left"), sv.Header(seq=k, stamp=1.0 + k, frame_id="right")
            node.mainRoutine(sv.Image.from_array(L, "rgb8", hl), sv.Image.from_array(R, "rgb8", hr))      # (used to spin for ever at k = 2)
            assert node._matcher().outstanding() < 2
        node.drain()
        assert node.failed_frames == 5 and not node._pending and node._matcher().outstanding() == 0 and log == []
        rsp = sv.GetDisparitiesGPUResponse()                    # the blocking service call fails the same way: false, as for a cv_bridge failure
        assert node.disparitySrv(sv.GetDisparitiesGPURequest(sv.Image.from_array(L, "rgb8", hl), sv.Image.from_array(R, "rgb8", hr)), rsp) is False
    finally:
        node._matcher().close()


def test_kernel_choices_follow_what_is_in_flight(lib, orc):
    """which choices a call gets is decided from what is in flight when it is submitted, not from ugsm_config.slots.  Visible
    from outside through the launch statistics (profile_events = 2 brackets slot 0's launches by kernel class): the 434 x 287 level of an
    872 x 576 pair runs k_cost_small when the call is alone on the chip and k_cost_march4 when another slot is busy -- on the SAME four-slot
    context; the blocking entry point is always alone.  Results are the oracle's either way."""
    from ug_stereomatcher_amd import synth
    W, H, lv = 872, 576, 10
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 770)
    exp = orc.match_full(L, R, lv)
    lw, lh = lib.level_dims(W, H, lv)
    mid = [i for i in range(lv) if 50000 < lw[i] * lh[i] <= 150000]
    assert mid, (lw, lh)

    def cost_kernels(c, level):
        return sorted({s["name"] for s in c.kernel_stats() if s["level"] == level and s["name"].startswith("k_cost")})

    with lib.Context(levels=lv, slots=4, profile_events=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        outs = [c.alloc(3 * W * H * 4) for _ in range(2)]
        # alone: nothing else in flight
        c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, outs[0]))
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert_bit_equal(c.to_host(outs[0], (3, H, W)), exp, "alone")
        assert cost_kernels(c, mid[0]) == ["k_cost_small"], cost_kernels(c, mid[0])
        c.reset_kernel_stats()
        # shared: slot 1 is busy when slot 0's call is submitted
        c.check(c.lib.ugsm_submit_full(c.handle, 1, dL, dR, W, H, 3 * W, outs[1]))
        c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, outs[0]))
        c.check(c.lib.ugsm_wait_all(c.handle))
        assert_bit_equal(c.to_host(outs[0], (3, H, W)), exp, "shared, slot 0")
        assert_bit_equal(c.to_host(outs[1], (3, H, W)), exp, "shared, slot 1")
        assert cost_kernels(c, mid[0]) == ["k_cost_march4"], cost_kernels(c, mid[0])
        c.reset_kernel_stats()
        # the blocking entry point (the node's service call) on the same four-slot context: alone again
        out = np.empty((3, H, W), np.float32)
        c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, W, H, L.strides[0], out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        assert_bit_equal(out, exp, "ugsm_match_full")
        assert cost_kernels(c, mid[0]) == ["k_cost_small"], cost_kernels(c, mid[0])
        c.reset_kernel_stats()
        # through the queue: a flushed pair with nothing else in flight is alone; a burst that fills calls is not
        c.enqueue_full(dL, dR, W, H, 3 * W, outs[0], 1)
        c.flush()
        assert [d.tag for d in c.drain()] == [1]
        assert cost_kernels(c, mid[0]) == ["k_cost_small"], cost_kernels(c, mid[0])
        for p in [dL, dR] + outs:
            c.free(p)
    with lib.Context(levels=lv, slots=2, batch=2, profile_events=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        outs = [c.alloc(3 * W * H * 4) for _ in range(6)]
        for k in range(6):                                       # calls of two fill up by themselves: a host that submits faster than the chip matches
            c.enqueue_full(dL, dR, W, H, 3 * W, outs[k], k)
        assert [d.tag for d in c.drain()] == list(range(6))
        for k in range(6):
            assert_bit_equal(c.to_host(outs[k], (3, H, W)), exp, f"burst, pair {k}")
        names = cost_kernels(c, mid[0])
        assert "k_cost_small" not in names, names               # 2 x 125 k pixels per launch, shared: the marching forms
        for p in [dL, dR] + outs:
            c.free(p)


def test_a_lone_call_borrows_a_neighbour_slots_stream(lib, orc, monkeypatch):
    """Round 6: a slot's side stream is a NEIGHBOUR slot's own stream (the one before it in the rotation), borrowed by a call that has the chip to itself (ugsm_create).  What must
    hold whatever the neighbour is doing: (a) lone calls in turn on every slot of a four-slot, a three-slot and a shared-stream context; (b) a
    call submitted on the neighbour while the lone call is still in flight queues behind the borrowed work; (c) with UGSM_ALONE=1 EVERY call
    forks, four in flight, each onto a stream that is busy with its neighbour's call -- stream order and the events keep all of it correct.
    Results: the oracle's, bit for bit, full and foveated."""
    from ug_stereomatcher_amd import synth
    W, H, lv, F = 640, 480, 9, 4
    L, R, _, _ = synth.make_pair(W, H, synth.BASE_SEED + 771)
    exp = orc.match_full(L, R, lv)
    expf = orc.match_foveated(L, R, lv, F)[0]
    fw, fh = lib.fovea_dims(W, H, lv, F)

    def burst(c, slots, wait_each):
        dL, dR = c.to_device(L), c.to_device(R)
        outs = [c.alloc(3 * W * H * 4) for _ in range(slots)]
        stks = [c.alloc(3 * F * fw * fh * 4) for _ in range(slots)]
        for rnd in range(2):
            for k in range(slots):
                c.check(c.lib.ugsm_submit_full(c.handle, k, dL, dR, W, H, 3 * W, outs[k]))
                if wait_each:
                    c.check(c.lib.ugsm_wait(c.handle, k))
            c.check(c.lib.ugsm_wait_all(c.handle))
            for k in range(slots):
                assert_bit_equal(c.to_host(outs[k], (3, H, W)), exp, f"full, slot {k}, round {rnd}")
            for k in range(slots):
                c.check(c.lib.ugsm_submit_foveated(c.handle, k, dL, dR, W, H, 3 * W, 0, 0, stks[k], None, None))
                if wait_each:
                    c.check(c.lib.ugsm_wait(c.handle, k))
            c.check(c.lib.ugsm_wait_all(c.handle))
            for k in range(slots):
                assert_bit_equal(c.to_host(stks[k], (3, F, fh, fw)), expf, f"foveated, slot {k}, round {rnd}")
        for p in [dL, dR] + outs + stks:
            c.free(p)

    for kw in ({"slots": 4}, {"slots": 3}, {"slots": 4, "streams": 2}, {"slots": 2, "streams": 1}, {"slots": 1}):
        with lib.Context(levels=lv, fovea_levels=F, **kw) as c:
            burst(c, kw["slots"], wait_each=True)      # (a): every call alone, forking onto a neighbour's (idle) stream
            burst(c, kw["slots"], wait_each=False)     # (b): the first call of a round is alone and borrows; the others queue behind it
    monkeypatch.setenv("UGSM_DEV", "1")
    monkeypatch.setenv("UGSM_ALONE", "1")
    with lib.Context(levels=lv, fovea_levels=F, slots=4) as c:
        burst(c, 4, wait_each=False)                   # (c)


def test_bench_line_keys(lib):
    """bench.py end to end on the GPU at a reduced step count (the driver runs the real thing): ONE JSON line on stdout whose `vs_baseline` is the
    same-bracket ratio, with `other_workloads` for BASELINE configs[3] and configs[1] and the lone-call figure on the timed
    context within a few per cent of the one-slot context's."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("UGSM_DEV", None)     # the product as a user runs it
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--repeats", "0", "--profile-pairs", "1",
                        "--single-pairs", "6", "--other-steps", "32"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "stereo pairs/sec at 16MP full-res pyramid" and d["unit"] == "pairs/s" and d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["calls_formed_by_the_library"] == [4, 5, 7, 4]
    bc = d["baseline_comparison"]
    assert bc["vs_baseline_is"] == "same_bracket" and d["vs_baseline"] == bc["same_bracket"]["ratio"]
    assert abs(bc["same_bracket"]["pairs_per_s"] - d["pcie_inclusive"]["pageable_pairs_per_s"]) < 1e-9
    assert 100 < d["vs_baseline"] < d["baseline_comparison"]["throughput"]["ratio"]           # host memory in and out costs: never the larger figure
    for name, ref in (("fovea16mp", 1.0 / 3.0), ("1080p", None)):
        o = d["other_workloads"][name]
        assert "error" not in o, o
        assert o["value"] > 100 and o["blocking_call_ms"] > 0 and o["steps"] == 32
        assert (o["vs_reference_same_bracket"] is None) == (ref is None)
    sp = d["single_pair_no_events"]
    assert 0.9 < sp["on_the_timed_context"]["vs_one_slot_context"] < 1.1, sp      # (reported exactly in the line; 11.6 % apart before round 6)
    assert "roofline" in d and d["roofline"]["kernel"] == "k_cost_march" and 0.1 < d["roofline"]["frac"] < 1.0


def test_bench_plain_line_and_dumped_outputs(lib, oracle_16mp_b, tmp_path):
    """A plain bench.py run (no --full): the headline line and nothing that needs runs of its own; --dump-outputs writes the last timed step's
    planes -- at 16 MP bench.dump_outputs' seeded sample of pixels -- equal bit for bit to the oracle's answer for that step's pair (step 19
    of 20: bench.py's second pair)."""
    import json
    import os
    import subprocess
    import sys
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("UGSM_DEV", None)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "stereo pairs/sec at 16MP full-res pyramid" and d["unit"] == "pairs/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["steps"] == 20 and d["warmup"] == 5 and d["calls_formed_by_the_library"] == [4, 5, 7, 4]
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6
    assert d["vs_baseline"] is None and d["value_repeats"] == [] and d["steady_state"]["value"] is None
    for key in ("cpu_baseline", "other_workloads", "pcie_inclusive", "single_pair_no_events", "event_pass", "roofline", "kernels"):
        assert key not in d, key
    W, H = oracle_16mp_b["W"], oracle_16mp_b["H"]
    idx = np.sort(np.random.Generator(np.random.PCG64(bench.DUMP_SEED)).choice(W * H, bench.DUMP_SAMPLE_PIXELS, replace=False))
    ref = oracle_16mp_b["full"].reshape(3, -1)
    total = 0
    for i, name in enumerate(("disparity_x", "disparity_y", "confidence")):
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE_PIXELS,), (name, a.dtype, a.shape)
        assert_bit_equal(a, ref[i, idx], name)
        total += a.nbytes
    assert total <= 64 << 20


def test_queue_from_plain_c(lib, tmp_path):
    """ros/queue_example.c: the frame loop of a C host -- ugsm_enqueue_full_managed with three frames in flight, every result equal to the
    blocking ugsm_match_full of the same frame -- compiled with gcc against include/ugsm.h and the built library, run here."""
    import os
    import shutil
    import subprocess
    from conftest import ROOT
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    exe = str(tmp_path / "queue_example")
    libdir = os.path.join(ROOT, "ug_stereomatcher_amd")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "ros", "queue_example.c"), "-L" + libdir, "-lugsm",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "QUEUE_EXAMPLE_OK" in out.stdout and "identical to the blocking calls" in out.stdout, out.stdout
