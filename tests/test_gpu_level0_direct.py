"""Full-mode calls read level 0 from the 8-bit images themselves (Slot::direct0, ugsm_levels.cpp: the pyramid pass stores levels 1 and 2 only,
A = G * L^2 and K-cost of level 0 run their 8-bit instances on the image): bit for bit the result of the materialised float level 0
(UGSM_LEVEL0_FLOAT=1 under UGSM_DEV=1) and of the CPU oracle.

The direct path needs level 0 matched by k_cost_march, which production gives to levels above 3 Mpx; here march_min_pixels = 1 and
UGSM_MARCH4=0,0 give it every level, so that strides, pointers, batches, queue-formed calls, the side stream, the LR check's second match and
the division fallbacks are crossed on images the oracle finishes in seconds.  Every case first asserts that the path under test was the one
taken: after a direct single-pair call the slot holds no whole pyramids, so ugsm_submit_fovea_coarse answers UGSM_ERR_STATE; after a
materialised one it runs.  Batched and queue-formed calls leave no such trace (and the same bits either way), so those cases ask the
development library which path the slot's last call took (ugsm_stage_level0_direct).  The 16 MP oracle comparisons of the existing suite run
the direct path as production picks it.
"""
import numpy as np
import pytest

import dark_np as dk
import encode_np as en
from conftest import assert_bit_equal
from test_gpu_input_format import Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def every_level_through_k_cost_march(monkeypatch):
    monkeypatch.setenv("UGSM_MARCH4", "0,0")
    monkeypatch.delenv("UGSM_LEVEL0_FLOAT", raising=False)


def _pair(W, H, seed):
    from ug_stereomatcher_amd import synth
    return synth.make_pair(W, H, synth.BASE_SEED + seed)[:2]


def _pad(W, at_least):
    """Padding bytes per rgb8 row, at least `at_least`, that make the stride 3 W + pad no multiple of 4."""
    pad = at_least
    while (3 * W + pad) % 4 == 0:
        pad += 1
    return pad


def _contexts(lib, monkeypatch, **kw):
    """(direct, materialised): two contexts of the same configuration, the second created under UGSM_LEVEL0_FLOAT=1."""
    kw.setdefault("march_min_pixels", 1)
    direct = lib.Context(**kw)
    monkeypatch.setenv("UGSM_LEVEL0_FLOAT", "1")
    try:
        return direct, lib.Context(**kw)
    finally:
        monkeypatch.delenv("UGSM_LEVEL0_FLOAT")


def _holds_whole_pyramids(lib, c, W, H, slot=0):
    """After a single-pair full-mode call on `slot`: does the slot hold whole pyramids (the materialised level 0)?  Read off ugsm_submit_fovea_coarse."""
    fw, fh = lib.fovea_dims(W, H, c.cfg.levels, c.cfg.fovea_levels)
    state = c.alloc(3 * fw * fh * 4)
    try:
        st = c.lib.ugsm_submit_fovea_coarse(c.handle, slot, state)
        assert st in (0, lib.UGSM_ERR_STATE), st
        if st == 0:
            c.check(c.lib.ugsm_wait(c.handle, slot))
        return st == 0
    finally:
        c.free(state)


def _took_direct(c, slot=0):
    """Which path the last call on `slot` took (libugsm_dev.so): True = level 0 read from the images."""
    st = c.lib.ugsm_stage_level0_direct(c.handle, slot)
    assert st in (0, 1), st
    return st == 1


def _full(lib, c, L, R, pad=0, shift=0, slot=0, direct=None):
    """One ugsm_submit_full on device copies laid out as asked; direct (True / False): assert which path the call took."""
    H, W = L.shape[:2]
    d = Dev(c)
    try:
        (pl, stride), (pr, _) = d.put(L, pad, shift), d.put(R, pad, shift)
        o = d.out(3 * W * H)
        c.check(c.lib.ugsm_submit_full(c.handle, slot, pl, pr, W, H, stride, o))
        c.check(c.lib.ugsm_wait(c.handle, slot))
        got = c.to_host(o, (3, H, W))
        if direct is not None:
            assert _holds_whole_pyramids(lib, c, W, H, slot) == (not direct), "the call did not take the path under test"
        return got
    finally:
        d.free()


# ---- sizes, strides, pointers -----------------------------------------------------------------------------------------------------------

# widths and heights that are no multiple of 4, 58 (K-cost's strip) or 64 (the tiles); 61 and 117 columns are two and three strips wide
SIZES = [(61, 59, 6), (117, 45, 6), (257, 131, 8), (333, 251, 10)]
# (least padding bytes per row -- _pad -- , bytes the image starts past its allocation): packed; two padded strides that are no multiple of 4,
# with pointers 1 and 3 bytes off
LAYOUTS = [(0, 0), (5, 1), (8, 3)]


@pytest.mark.parametrize("W, H, lv", SIZES, ids=[f"{w}x{h}" for w, h, _ in SIZES])
def test_sizes_strides_and_unaligned_pointers(lib, orc, monkeypatch, W, H, lv):
    L, R = _pair(W, H, 810 + W)
    exp = orc.match_full(L, R, lv)
    direct, mat = _contexts(lib, monkeypatch, levels=lv)
    with direct, mat:
        for least, shift in LAYOUTS:
            pad = _pad(W, least) if least else 0
            assert pad == 0 or ((3 * W + pad) % 4 != 0 and pad >= 5)
            a = _full(lib, direct, L, R, pad, shift, direct=True)
            b = _full(lib, mat, L, R, pad, shift, direct=False)
            assert_bit_equal(a, b, f"{W}x{H} pad {pad} shift {shift}: direct vs materialised level 0")
            assert_bit_equal(a, exp, f"{W}x{H} pad {pad} shift {shift}: direct level 0 vs oracle")


# ---- batches, the queue, host and managed buffers ----------------------------------------------------------------------------------------

def test_batch_of_distinct_pairs_in_buffers_of_their_own(lib, orc, monkeypatch):
    """Every pair of a batched call with images of its own, each in its own allocation at its own misalignment: the left and the right image
    of pair b lie at unrelated offsets from pair 0's (Batch::img for L; cx / cy carry R's)."""
    W, H, lv, n = 203, 149, 8, 3
    pairs = [_pair(W, H, 840 + k) for k in range(n)]
    exp = [orc.match_full(L, R, lv) for L, R in pairs]
    direct, mat = _contexts(lib, monkeypatch, levels=lv, batch=n, dev=True)
    with direct, mat:
        res = []
        for c, is_direct in ((direct, True), (mat, False)):
            d = Dev(c)
            try:
                # same padding (one stride per call), different shifts; the right images allocated in the opposite order
                pad = _pad(W, 5)
                pl = [d.put(L, pad, k)[0] for k, (L, _) in enumerate(pairs)]
                pr = [0] * n
                for k in reversed(range(n)):
                    pr[k] = d.put(pairs[k][1], pad, 3 - k)[0]
                outs = [d.out(3 * W * H) for _ in pairs]
                c.submit_full_batch(0, pl, pr, W, H, 3 * W + pad, outs)
                c.check(c.lib.ugsm_wait(c.handle, 0))
                assert _took_direct(c) == is_direct, "the batched call did not take the path under test"
                res.append([c.to_host(o, (3, H, W)) for o in outs])
            finally:
                d.free()
        for k in range(n):
            assert_bit_equal(res[0][k], res[1][k], f"batch pair {k}: direct vs materialised level 0")
            assert_bit_equal(res[0][k], exp[k], f"batch pair {k}: direct level 0 vs oracle")


def test_calls_formed_by_the_queue_device_host_and_managed(lib, orc, monkeypatch):
    W, H, lv, n = 181, 127, 8, 5
    uniq = [_pair(W, H, 860 + k) for k in range(3)]
    exp = [orc.match_full(L, R, lv) for L, R in uniq]
    direct, mat = _contexts(lib, monkeypatch, levels=lv, slots=2, batch=2, dev=True)

    def path_taken(c, is_direct, what):   # every slot the queue used: its last call took the path under test
        assert [_took_direct(c, slot) for slot in (0, 1)] == [is_direct] * 2, what

    with direct, mat:
        for c, is_direct in ((direct, True), (mat, False)):
            what = "direct" if is_direct else "materialised"
            dL, dR = [c.to_device(L) for L, _ in uniq], [c.to_device(R) for _, R in uniq]
            dO = [c.alloc(3 * W * H * 4) for _ in range(n)]
            for k in range(n):
                c.enqueue_full(dL[k % 3], dR[k % 3], W, H, 3 * W, dO[k], k)
            done = c.drain()
            assert [d.tag for d in done] == list(range(n)) and max(d.call_pairs for d in done) == 2   # (calls of two: batched level-0 launches)
            path_taken(c, is_direct, f"{what}: device queue")
            for k in range(n):
                assert_bit_equal(c.to_host(dO[k], (3, H, W)), exp[k % 3], f"{what}: device queue, pair {k}")
            for p in dL + dR + dO:
                c.free(p)
            pin = []
            for k in range(n):
                L, R = uniq[k % 3]
                pl, pr, po = c.host_array(L.shape, L.dtype), c.host_array(R.shape, R.dtype), c.host_array((3, H, W))
                pl[...], pr[...], po[...] = L, R, -1.0
                pin.append(po)
                c.enqueue_full_host(pl, pr, po, k)
            assert [d.tag for d in c.drain()] == list(range(n))
            path_taken(c, is_direct, f"{what}: page-locked host queue")
            for k in range(n):
                assert_bit_equal(pin[k], exp[k % 3], f"{what}: page-locked host queue, pair {k}")
            for k in range(n):
                Lc, Rc = uniq[k % 3][0].copy(), uniq[k % 3][1].copy()
                c.enqueue_full_managed(Lc, Rc, 100 + k)
                Lc[...] = 0   # (the caller's images are its own again once the call has returned: level 0 is read from the library's copy)
                Rc[...] = 0
            c.flush()
            for k in range(n):
                d = c.next_done(True)
                assert d.tag == 100 + k
                if k == n - 1:
                    path_taken(c, is_direct, f"{what}: managed queue")
                h, v, cf = c.managed_planes(d, [(H, W)] * 3)
                assert_bit_equal(np.stack([h, v, cf]), exp[k % 3], f"{what}: managed queue, pair {k}")


def test_blocking_service_call_on_pageable_memory(lib, orc, monkeypatch):
    from ug_stereomatcher_amd import MatchGPULib
    W, H, lv = 222, 154, 8
    L, R = _pair(W, H, 870)
    exp = orc.match_full(L, R, lv)
    monkeypatch.setenv("UGSM_MARCH_MIN_PIXELS", "1")
    for var in (None, "1"):
        if var:
            monkeypatch.setenv("UGSM_LEVEL0_FLOAT", var)
        m = MatchGPULib(levels=lv)
        got = m.match(L, R, 0)
        m.close()
        assert_bit_equal(got, exp, f"ugsm_match_full, UGSM_LEVEL0_FLOAT={var}")


# ---- a lone call on a four-slot context; the LR check's second match -----------------------------------------------------------------------

@pytest.mark.parametrize("two_streams", ["1", "0"])
def test_lone_call_on_a_four_slot_context(lib, orc, monkeypatch, two_streams):
    """A call alone on the chip forks: the right pyramid and the A planes -- level 0's from the left image itself -- on a borrowed side stream."""
    W, H, lv = 301, 211, 9
    L, R = _pair(W, H, 880)
    exp = orc.match_full(L, R, lv)
    monkeypatch.setenv("UGSM_TWO_STREAMS", two_streams)
    direct, mat = _contexts(lib, monkeypatch, levels=lv, slots=4)
    with direct, mat:
        for slot in (0, 2, 3):
            a = _full(lib, direct, L, R, _pad(W, 5), 1, slot, direct=True)
            b = _full(lib, mat, L, R, _pad(W, 5), 1, slot, direct=False)
            assert_bit_equal(a, b, f"lone call on slot {slot}: direct vs materialised level 0")
            assert_bit_equal(a, exp, f"lone call on slot {slot}: direct level 0 vs oracle")


def test_lr_check_second_match_reads_the_images_exchanged(lib, orc, monkeypatch):
    W, H, lv = 240, 160, 8
    L, R = _pair(W, H, 890)
    direct, mat = _contexts(lib, monkeypatch, levels=lv)
    with direct, mat:
        res = []
        for c, is_direct in ((direct, True), (mat, False)):
            c.set_lr_check(1.0, lib.UGSM_LR_FULL)
            res.append((_full(lib, c, L, R, 7, 3, direct=None), c.last_lr_marked(0)))
        assert res[0][1] == res[1][1] and res[0][1] > 0
        assert_bit_equal(res[0][0], res[1][0], "full-mode LR check: direct vs materialised level 0")
        # the unchecked planes are the oracle's; the check only zeroes confidences
        exp = orc.match_full(L, R, lv)
        assert_bit_equal(res[0][0][:2], exp[:2], "full-mode LR check: disparities vs oracle")
        back = orc.match_full(R, L, lv)
        with lib.Context(levels=lv, march_min_pixels=1) as c:
            assert_bit_equal(_full(lib, c, R, L, 7, 3, direct=True), back, "the exchanged pair, direct level 0 vs oracle")


# ---- dark, flat and black images: the compiler's full division sequence ------------------------------------------------------------------

def test_dark_flat_and_black_pairs(lib, orc, monkeypatch):
    W, H, lv = 640, 480, 14
    L0, R0 = _pair(W, H, 300)
    cases = {"dark": dk.dark_pair(L0, R0, 77)}
    cases.update(dk.degenerate_pairs(L0, R0))
    word, cl, cr = dk.pair_word(orc, *cases["dark"], lv)
    assert word == 1 and dk.trips(cl) and dk.trips(cr), (cl, cr)   # premise: the dark pair leaves the guarded range
    direct, mat = _contexts(lib, monkeypatch, levels=lv, dev=True)
    with direct, mat:
        for name, (L, R) in cases.items():
            L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
            a = _full(lib, direct, L, R, 5, 1, direct=True)
            words = direct.range_words(0, 1)
            b = _full(lib, mat, L, R, 5, 1, direct=False)
            assert_bit_equal(a, b, f"{name}: direct vs materialised level 0")
            assert_bit_equal(a, orc.match_full(L, R, lv), f"{name}: direct level 0 vs oracle")
            assert words == [dk.pair_word(orc, L, R, lv)[0]], f"{name}: range word {words}"


# ---- wild disparities through the clamped byte gather ---------------------------------------------------------------------------------------

def test_wild_disparities_through_the_byte_gather(lib, orc):
    """NaN, +-Inf, huge and denormal disparities, as test_march_wild_disparities builds them, at the frame and inside: the 8-bit K-cost
    instance clamps the gather to the image like the float one (ugsm_stage_iterate_rgb8, libugsm_dev.so)."""
    rng = np.random.Generator(np.random.PCG64(79))
    W, H = 150, 40
    L, R = (np.ascontiguousarray(a[:H, :W]) for a in _pair(160, 48, 4200))
    pl, pr = orc.rgb_to_planes(L), orc.rgb_to_planes(R)
    d0 = np.stack([rng.normal(0, 5, (H, W)), rng.normal(0, 5, (H, W)), 0.2 + 0.8 * rng.random((H, W))]).astype(np.float32)
    wild = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e10, -1e10, 2147483648.0, -2147483904.0, 1e-45, -1e-45, -0.5, -0.49999997],
                    np.float32)
    idx = rng.integers(0, H * W, 400)
    d0[0].ravel()[idx[:200]] = wild[rng.integers(0, len(wild), 200)]
    d0[1].ravel()[idx[200:]] = wild[rng.integers(0, len(wild), 200)]
    for plane in (0, 1):   # ... and along the frame, where the clamp decides the byte that is read
        d0[plane, 0, ::3] = wild[rng.integers(0, len(wild), len(d0[plane, 0, ::3]))]
        d0[plane, -1, 1::3] = wild[rng.integers(0, len(wild), len(d0[plane, -1, 1::3]))]
        d0[plane, ::3, 0] = wild[rng.integers(0, len(wild), len(d0[plane, ::3, 0]))]
        d0[plane, 1::3, -1] = wild[rng.integers(0, len(wild), len(d0[plane, 1::3, -1]))]
    exp, _ = orc.iterate_level(pl, pr, d0, 4, 0, False, 1, 1)
    for rows in (16, 0):
        with lib.Context(levels=1, march_min_pixels=1, march_rows=rows, dev=True) as c:
            d = Dev(c)
            try:
                (dl, stride), (dr, _) = d.put(L, 5, 1), d.put(R, 5, 1)
                pd = c.to_device(d0)
                d.bufs.append(pd)
                c.check(c.lib.ugsm_stage_iterate_rgb8(c.handle, dl, dr, stride, pd, W, H, 4, 0, 0, 1, 1))
                got = c.to_host(pd, (3, H, W))
            finally:
                d.free()
        assert_bit_equal(got, exp, f"wild disparities, 8-bit instance, march_rows={rows}")


# ---- the input layouts ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", en.FORMATS, ids=[en.NAMES[f] for f in en.FORMATS])
def test_each_input_layout(lib, orc, monkeypatch, fmt):
    """rgb8 calls read level 0 from the image; the other layouts keep the materialised float level 0 (level0_direct, ugsm_policy.cpp) -- either
    way the result is the rgb8 result on the image's conversion to rgb8, under both settings of the development switch."""
    W, H, lv = 157, 101, 8
    L, R = _pair(W, H, 61)
    a, b = en.encode(L, fmt), en.encode(R, fmt)
    exp = orc.match_full(en.to_rgb8(a, fmt), en.to_rgb8(b, fmt), lv)
    direct, mat = _contexts(lib, monkeypatch, levels=lv)
    with direct, mat:
        for c in (direct, mat):
            c.set_input_format(fmt)
        for pad, shift in ((0, 0), (8, 1)):
            x = _full(lib, direct, a, b, pad, shift, direct=(fmt == en.RGB8))
            y = _full(lib, mat, a, b, pad, shift, direct=False)
            assert_bit_equal(x, y, f"{en.NAMES[fmt]} pad {pad} shift {shift}: default vs UGSM_LEVEL0_FLOAT=1")
            assert_bit_equal(x, exp, f"{en.NAMES[fmt]} pad {pad} shift {shift}: vs oracle")


# ---- the fovea phases after a full-mode call ---------------------------------------------------------------------------------------------------

def test_fovea_coarse_after_a_full_call_needs_the_pyramids_again(lib, orc):
    """include/ugsm.h: ugsm_submit_fovea_coarse / _fine work on the pyramids of ugsm_submit_pyramids.  A full-mode call leaves no level 0
    behind, so after it they answer UGSM_ERR_STATE until ugsm_submit_pyramids has run -- and then give the oracle's stack."""
    W, H, lv, F = 333, 251, 10, 4
    L, R = _pair(W, H, 900)
    off = (21, -13)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    exp = orc.match_foveated(L, R, lv, F, off[0], off[1])[0]
    with lib.Context(levels=lv, fovea_levels=F, march_min_pixels=1) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        out, state, stack = c.alloc(3 * W * H * 4), c.alloc(3 * fw * fh * 4), c.alloc(3 * F * fw * fh * 4)
        try:
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, out))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            assert_bit_equal(c.to_host(out, (3, H, W)), orc.match_full(L, R, lv), "the full-mode call")
            assert c.lib.ugsm_submit_fovea_coarse(c.handle, 0, state) == lib.UGSM_ERR_STATE
            assert c.lib.ugsm_submit_fovea_fine(c.handle, 0, state, off[0], off[1], stack) == lib.UGSM_ERR_STATE
            c.check(c.lib.ugsm_submit_pyramids(c.handle, 0, dL, dR, W, H, 3 * W))
            c.check(c.lib.ugsm_submit_fovea_coarse(c.handle, 0, state))
            c.check(c.lib.ugsm_submit_fovea_fine(c.handle, 0, state, off[0], off[1], stack))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            assert_bit_equal(c.to_host(stack, (3, F, fh, fw)), exp, "split fovea phases after ugsm_submit_pyramids")
        finally:
            for p in (dL, dR, out, state, stack):
                c.free(p)
