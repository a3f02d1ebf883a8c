"""Checked full-mode pairs through the queue (ugsm_enqueue_full_checked[_managed | _cloud | _cloud_managed], ugsm_done_checked) on the device,
against the CPU oracle, bit for bit.

The definition (include/ugsm.h, "checked pairs through the queue"): d_out and d_back of a pair are what ugsm_submit_full_checked writes for that
pair alone with that tau, however the queue grouped the pairs -- so per pair the oracle is orc.match_full both ways and orc.lr_check both ways,
each against the other direction's unchecked field.  The inputs are the ones tests/test_gpu_lr_full.py pins (its oracle answers are computed once
per session and shared); a context sees one size, and its pairs alternate between an input and the same input with the images exchanged, whose
answer is the first one's with the directions exchanged.  Every test asserts its premise -- the check both marks and spares -- from the oracle
alone before it compares.  The clouds: byte for byte what ugsm_point_cloud writes for the ORACLE's checked forward planes and the left image."""
import numpy as np
import pytest

import encode_np as en
from conftest import assert_bit_equal
from test_gpu_cloud import P1, P2A
from test_gpu_lr_full import ROWS, _premise, _row_answer

pytestmark = pytest.mark.gpu

R130, R64, R200 = ROWS[2], ROWS[3], ROWS[1]
assert (R130[:2], R64[:2], R200[:2]) == ((130, 97), (64, 48), (200, 150))
NAN = np.float32(np.nan)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def answers(orc, row):
    """[(L, R, answer), (R, L, the answer with the directions exchanged)] of a pinned input: the two pairs a context's burst alternates between."""
    W, H, lv, seed, tau, pinned = row
    L, R, ans = _row_answer(orc, row)
    assert ans[4] == pinned, ans[4]
    _premise(ans, W, H, f"{W}x{H}")
    F, B, cF, cB, (nF, nB) = ans
    return [(L, R, ans), (R, L, (B, F, cB, cF, (nB, nF)))]


def retau(orc, ans, tau, W, H):
    """The oracle's answer of the same pair for another threshold (the unchecked fields are the same)."""
    F, B = ans[0], ans[1]
    cF, nF = orc.lr_check(F, B, tau)
    cB, nB = orc.lr_check(B, F, tau)
    out = (F, B, cF, cB, (nF, nB))
    _premise(out, W, H, f"tau {tau}")
    return out


def assert_field(got, unchecked, checked, what):
    assert_bit_equal(got[:2], unchecked[:2], f"{what}: dx, dy against the unchecked oracle field")
    assert_bit_equal(got[2], checked[2], f"{what}: the confidence against the oracle's checked one")


def nan_buffer(c, n):
    return c.to_device(np.full(n, NAN, np.float32))


def plan_per_pair(lib, n, slots, batch):
    return [s for s in lib.queue_plan(n, slots=slots, batch=batch) for _ in range(s)]


# ---- 1. the device kind ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [R130, R64, R200], ids=["130x97", "64x48", "200x150"])
def test_device_pairs_through_the_queue(lib, orc, row):
    """Eleven pairs on two slots with calls of up to four, NaN-filled outputs, d_back NULL for the odd pairs: every d_out and d_back against the
    oracle, call sizes ugsm_queue_plan's, the counts of ugsm_done_checked the pinned ones."""
    W, H, lv, seed, tau, pinned = row
    two = answers(orc, row)
    n = 11
    with lib.Context(levels=lv, slots=2, batch=4) as c:
        held = []
        for k in range(n):
            L, R, _ = two[k % 2]
            dL, dR, dO = c.to_device(L), c.to_device(R), nan_buffer(c, 3 * W * H)
            dB = nan_buffer(c, 3 * W * H) if k % 2 == 0 else None
            c.enqueue_full_checked(dL, dR, W, H, 3 * W, dO, dB, tau, 100 + k)
            held.append((dO, dB))
        c.flush()
        sizes = plan_per_pair(lib, n, 2, 4)
        for k in range(n):
            d = c.next_done(True)
            assert d is not None and d.tag == 100 + k
            assert d.call_pairs == sizes[k], (k, d.call_pairs, sizes)
            assert not any(d.result[j] for j in range(5))
            F, B, cF, cB, marked = two[k % 2][2]
            fwd, back, planes = c.done_checked()
            assert (fwd, back) == marked and planes is None, (k, fwd, back, marked)
            assert marked == (pinned if k % 2 == 0 else pinned[::-1])
            dO, dB = held[k]
            assert_field(c.to_host(dO, (3, H, W)), F, cF, f"pair {k}, d_out")
            if dB is not None:
                assert_field(c.to_host(dB, (3, H, W)), B, cB, f"pair {k}, d_back")
        assert c.next_done(True) is None


# ---- 2. a tau that changes mid-burst, a plain pair in between -------------------------------------------------------------------------------
def test_every_pair_takes_its_own_tau_and_plain_pairs_the_contexts(lib, orc):
    W, H, lv, seed, tau, pinned = R130
    L, R, ans = answers(orc, R130)[0]
    half, ctx_tau = retau(orc, ans, 0.5, W, H), retau(orc, ans, 2.0, W, H)
    assert len({ans[4], half[4], ctx_tau[4]}) == 3, "premise: the three thresholds mark different numbers of pixels"
    with lib.Context(levels=lv, slots=2, batch=4) as c:
        c.set_lr_check(2.0, lib.UGSM_LR_FULL)
        dL, dR = c.to_device(L), c.to_device(R)
        kinds = [(tau, ans), (tau, ans), (0.5, half), (None, ctx_tau), (0.5, half), (tau, ans)]
        held = []
        for k, (t, _) in enumerate(kinds):
            dO, dB = nan_buffer(c, 3 * W * H), nan_buffer(c, 3 * W * H)
            if t is None:
                c.enqueue_full(dL, dR, W, H, 3 * W, dO, k)
            else:
                c.enqueue_full_checked(dL, dR, W, H, 3 * W, dO, dB, t, k)
            held.append((dO, dB))
        c.flush()
        calls = []
        for k, (t, a) in enumerate(kinds):
            d = c.next_done(True)
            assert d is not None and d.tag == k
            calls.append((d.call_index, d.call_pairs))
            F, B, cF, cB, marked = a
            assert_field(c.to_host(held[k][0], (3, H, W)), F, cF, f"pair {k} (tau {t}), d_out")
            if t is None:
                with pytest.raises(lib.UgsmError) as e:
                    c.done_checked()
                assert e.value.status == lib.UGSM_ERR_STATE
                assert np.isnan(c.to_host(held[k][1], (3, H, W))).all()                # (its spare buffer: nothing wrote there)
            else:
                assert_field(c.to_host(held[k][1], (3, H, W)), B, cB, f"pair {k} (tau {t}), d_back")
                assert c.done_checked()[:2] == marked, (k, t)
        assert calls == [(0, 2), (0, 2), (1, 1), (2, 1), (3, 1), (4, 1)], calls       # a call ends where tau or the kind changes
        assert c.lr_check == (np.float32(2.0), lib.UGSM_LR_FULL)                       # the context's setting was neither used nor changed


# ---- 3. the input format is captured at enqueue ---------------------------------------------------------------------------------------------
def test_the_format_is_the_one_at_enqueue(lib, orc):
    """Two bgr8 pairs are enqueued, then the context goes back to rgb8 before the flush sends their call: the results are those of the images'
    conversion to rgb8 -- the pinned input itself."""
    W, H, lv, seed, tau, pinned = R64
    L, R, ans = answers(orc, R64)[0]
    bl, br = en.encode(L, en.BGR8), en.encode(R, en.BGR8)
    assert np.array_equal(en.to_rgb8(bl, en.BGR8), L) and not np.array_equal(bl, L)
    with lib.Context(levels=lv, slots=2, batch=4) as c:
        c.set_input_format(lib.UGSM_INPUT_BGR8)
        dL, dR = c.to_device(bl), c.to_device(br)
        outs = [(nan_buffer(c, 3 * W * H), nan_buffer(c, 3 * W * H)) for _ in range(2)]
        for k, (dO, dB) in enumerate(outs):
            c.enqueue_full_checked(dL, dR, W, H, 3 * W, dO, dB, tau, k)
        c.set_input_format(lib.UGSM_INPUT_RGB8)
        c.flush()
        F, B, cF, cB, marked = ans
        for k, (dO, dB) in enumerate(outs):
            d = c.next_done(True)
            assert d.tag == k and d.call_pairs == 2
            assert c.done_checked()[:2] == marked
            assert_field(c.to_host(dO, (3, H, W)), F, cF, f"bgr8 pair {k}, d_out")
            assert_field(c.to_host(dB, (3, H, W)), B, cB, f"bgr8 pair {k}, d_back")


# ---- 4. managed -------------------------------------------------------------------------------------------------------------------------------
def test_managed_pairs_lend_their_planes_and_back_planes(lib, orc):
    W, H, lv, seed, tau, pinned = R130
    two = answers(orc, R130)
    want_back = [1, 0, 0, 1, 1]
    with lib.Context(levels=lv, slots=2, batch=4) as c:
        for k, wb in enumerate(want_back):
            L, R, _ = two[k % 2]
            c.enqueue_full_checked_managed(L.copy(), R.copy(), tau, bool(wb), k)            # (temporaries: the images are copied before the call returns)
        c.flush()
        sizes = plan_per_pair(lib, len(want_back), 2, 4)
        for k, wb in enumerate(want_back):
            d = c.next_done(True)
            assert d is not None and d.tag == k and d.call_pairs == sizes[k]
            assert d.result[0] and d.result[1] and d.result[2] and not d.result[3] and not d.result[4]
            F, B, cF, cB, marked = two[k % 2][2]
            got = np.stack(c.managed_planes(d, [(H, W)] * 3))
            assert_field(got, F, cF, f"managed pair {k}, the lent planes")
            fwd, back, planes = c.done_checked((H, W))
            assert (fwd, back) == marked
            assert (planes is not None) == bool(wb), k
            if wb:
                assert_field(planes, B, cB, f"managed pair {k}, the lent back planes")
        assert c.next_done(True) is None


# ---- 5. clouds --------------------------------------------------------------------------------------------------------------------------------
def reference_cloud(lib, c, planes, L, W, H, params, item):
    """ugsm_point_cloud on a context of its own for host planes (3, H, W) and the left image: (count, the records as bytes)."""
    dP, dL = c.to_device(planes), c.to_device(L)
    cap = lib.cloud_points(W, H, params.sampling)
    d_pts, d_cnt = c.alloc(cap * item), c.alloc(8)
    n = c.point_cloud(dP, dP + 4 * W * H, dP + 8 * W * H, dL, W, H, 3 * W, P1, P2A, params, d_pts, cap, d_cnt)
    rec = c.to_host(d_pts, (min(n, cap) * item,), np.uint8)
    for p in (dP, dL, d_pts, d_cnt):
        c.free(p)
    return n, rec


@pytest.mark.parametrize("kind", ["device", "managed"])
@pytest.mark.parametrize("compact", [False, True], ids=["dense", "compact"])
def test_the_cloud_is_that_of_the_checked_forward_field(lib, orc, kind, compact):
    """Five pairs with a cloud each.  Compact with min_conf > 0: the marked pixels (confidence zeroed) drop out, so the cloud is strictly smaller
    than the same cloud of the unchecked field."""
    W, H, lv, seed, tau, pinned = R130
    two = answers(orc, R130)
    fmt, item = (lib.UGSM_CLOUD_XYZRGB16, 16) if compact else (lib.UGSM_CLOUD_PCL32, 32)
    min_conf = float(np.float32(1e-6)) if compact else None
    params = lib.cloud_params(sampling=1, format=fmt, compact=compact, min_conf=min_conf)
    dense = lib.cloud_points(W, H, 1)
    n = 5
    with lib.Context(levels=lv) as ref:
        want = [reference_cloud(lib, ref, np.ascontiguousarray(np.concatenate([a[0][:2], a[2][2:3]])), L, W, H, params, item) for L, R, a in two]
        unchecked = [reference_cloud(lib, ref, np.ascontiguousarray(a[0]), L, W, H, params, item)[0] for L, R, a in two]
    for k in range(2):
        if compact:
            assert 0 < want[k][0] < unchecked[k] <= dense, (want[k][0], unchecked[k], dense)            # premise: the check takes points away
        else:
            assert want[k][0] == unchecked[k] == dense
    with lib.Context(levels=lv, slots=2, batch=4) as c:
        spec = lib.queue_cloud(P1, P2A, params, want_planes=False)
        held = []
        for k in range(n):
            L, R, _ = two[k % 2]
            if kind == "managed":
                c.enqueue_full_checked_cloud_managed(L, R, tau, k % 2 == 1, spec, k)
                held.append(None)
            else:
                dL, dR, dO = c.to_device(L), c.to_device(R), nan_buffer(c, 3 * W * H)
                dB = nan_buffer(c, 3 * W * H) if k % 2 else None
                d_pts, d_cnt = c.to_device(np.full((dense + 8) * item, 0xA5, np.uint8)), c.to_device(np.full(1, -7, np.int64))
                c.enqueue_full_checked_cloud(dL, dR, W, H, 3 * W, dO, dB, tau, spec, d_pts, dense, d_cnt, k)
                held.append((dO, dB, d_pts, d_cnt))
        c.flush()
        sizes = plan_per_pair(lib, n, 2, 4)
        for k in range(n):
            d = c.next_done(True)
            assert d is not None and d.tag == k and d.call_pairs == sizes[k]
            F, B, cF, cB, marked = two[k % 2][2]
            cnt, rec = want[k % 2]
            fwd, back, planes = c.done_checked((H, W))
            assert (fwd, back) == marked
            if kind == "managed":
                assert not any(d.result[j] for j in range(5))                                        # want_planes 0: not downloaded
                assert (planes is not None) == (k % 2 == 1)
                if planes is not None:
                    assert_field(planes, B, cB, f"managed cloud pair {k}, the lent back planes")
                got, count, _ = c.done_cloud()
                assert count == cnt and np.array_equal(got.view(np.uint8), rec), (k, count, cnt)
            else:
                dO, dB, d_pts, d_cnt = held[k]
                count = int(c.to_host(d_cnt, (1,), np.int64)[0])
                raw = c.to_host(d_pts, ((dense + 8) * item,), np.uint8)
                assert count == cnt, (k, count, cnt)
                assert np.array_equal(raw[:cnt * item], rec) and (raw[cnt * item:] == 0xA5).all(), k
                assert_field(c.to_host(dO, (3, H, W)), F, cF, f"cloud pair {k}, d_out")
                if dB is not None:
                    assert_field(c.to_host(dB, (3, H, W)), B, cB, f"cloud pair {k}, d_back")
        assert c.next_done(True) is None


# ---- 6. batches of 3 and 16 through one call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 16])
def test_one_call_of_many_pairs(lib, orc, n):
    """batch = 16 on one slot: the burst is one call.  Sixteen pairs are 32 checks: the two-launch case of the stack check."""
    W, H, lv, seed, tau, pinned = R64
    two = answers(orc, R64)
    with lib.Context(levels=lv, slots=1, batch=16) as c:
        assert lib.queue_plan(n, slots=1, batch=16) == [n]
        held = []
        for k in range(n):
            L, R, _ = two[k % 2]
            dL, dR, dO = c.to_device(L), c.to_device(R), nan_buffer(c, 3 * W * H)
            dB = nan_buffer(c, 3 * W * H) if k % 3 else None
            c.enqueue_full_checked(dL, dR, W, H, 3 * W, dO, dB, tau, k)
            held.append((dO, dB))
        c.flush()
        for k in range(n):
            d = c.next_done(True)
            assert d is not None and d.tag == k and (d.call_pairs, d.call_index) == (n, 0)
            F, B, cF, cB, marked = two[k % 2][2]
            assert c.done_checked()[:2] == marked, k
            assert_field(c.to_host(held[k][0], (3, H, W)), F, cF, f"call of {n}, pair {k}, d_out")
            if held[k][1] is not None:
                assert_field(c.to_host(held[k][1], (3, H, W)), B, cB, f"call of {n}, pair {k}, d_back")
        assert c.next_done(True) is None


# ---- 7. the node's mirror: lr_check_tau with frames in flight --------------------------------------------------------------------------------
def test_the_service_mirror_enqueues_checked_frames(lib, orc):
    """ug_stereomatcher_amd/service.py with frames_in_flight = 2 and the parameter lr_check_tau: every full-mode frame goes through the checked
    queue form, and the three planes it publishes are the oracle's checked forward field; with tau 0 the frames are plain."""
    from ug_stereomatcher_amd import service as sv
    W, H, lv, seed, tau, pinned = R200
    L, R, ans = answers(orc, R200)[0]
    F, B, cF, cB, marked = ans
    for t, conf in ((tau, cF[2]), (0.0, F[2])):
        log = []
        node = sv.GPUMatcher(params={sv.FOVEATEDQ: 0, "lr_check_tau": t}, publish=lambda topic, m: log.append((topic, m)), frames_in_flight=2, levels=lv)
        try:
            for k in range(3):
                hl, hr = sv.Header(seq=k, stamp=1.0 + k, frame_id="left"), sv.Header(seq=k, stamp=1.0 + k, frame_id="right")
                node.mainRoutine(sv.Image.from_array(L, "rgb8", hl), sv.Image.from_array(R, "rgb8", hr))
            node.drain()
        finally:
            node._matcher().close()
        assert [topic for topic, _ in log] == [sv.CAM_PUB_HOR, sv.CAM_PUB_VER, sv.CAM_PUB_CONF] * 3
        for k in range(3):
            got = [np.frombuffer(m.image.data, np.float32).reshape(H, W) for _, m in log[3 * k:3 * k + 3]]
            assert_bit_equal(np.stack(got[:2]), F[:2], f"tau {t}, frame {k}: dispH, dispV")
            assert_bit_equal(got[2], conf, f"tau {t}, frame {k}: dispC")
