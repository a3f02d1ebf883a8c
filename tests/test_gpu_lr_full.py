"""The checked full-mode call: ugsm_submit_full_checked, ugsm_match_full_checked, ugsm_last_lr_marked_pair.

The definition (include/ugsm.h): d_out[k] is, bit for bit, what ugsm_submit_full(L_k, R_k) writes on a context with
ugsm_set_lr_check(ctx, tau, UGSM_LR_FULL), d_back[k] what that call writes for (R_k, L_k).  So per pair the oracle is orc.match_full(L, R, lv),
orc.match_full(R, L, lv) and orc.lr_check both ways, each against the other direction's UNCHECKED field; every comparison is bit-exact.  Every
definition test asserts its premise from the oracle alone: the check both fires and spares in both directions.  The counts of ROWS are the CPU
oracle's and are pinned."""
import ctypes as C

import numpy as np
import pytest

import dark_np as dk
import encode_np as en
from conftest import assert_bit_equal
from test_gpu_input_format import Dev

pytestmark = pytest.mark.gpu

ROWS = [  # W, H, levels, seed, tau, the CPU oracle's marked pixels forward / backward
    (333, 251, 14, 5202, 1.0, (9916, 10177)),
    (200, 150, 8, 5201, 0.5, (13167, 13237)),
    (130, 97, 6, 5203, 1.0, (4154, 4255)),
    (64, 48, 3, 5204, 1.0, (511, 559)),
]
IDS = [f"{r[0]}x{r[1]}x{r[2]}-tau{r[4]}" for r in ROWS]
BIG, MID, SMALL = ROWS[0], ROWS[1], ROWS[2]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


_PAIRS, _ANSWERS = {}, {}


def _pair(W, H, seed):
    if (W, H, seed) not in _PAIRS:
        from ug_stereomatcher_amd import synth
        L, R = synth.make_pair(W, H, synth.BASE_SEED + seed)[:2]
        for a in (L, R):
            a.setflags(write=False)
        _PAIRS[(W, H, seed)] = (L, R)
    return _PAIRS[(W, H, seed)]


def _answer(orc, L, R, lv, tau, key, fwd=None):
    """(F, B, checked F, checked B, (marked forward, marked backward)) of one pair from the oracle, computed once per key and shared.
    fwd: the unchecked forward field where a fixture already holds it."""
    k = (key, lv, tau)
    if k not in _ANSWERS:
        F = fwd if fwd is not None else orc.match_full(L, R, lv)
        B = orc.match_full(R, L, lv)
        cF, nF = orc.lr_check(F, B, tau)
        cB, nB = orc.lr_check(B, F, tau)
        for a in (B, cF, cB) + (() if fwd is not None else (F,)):
            a.setflags(write=False)
        _ANSWERS[k] = (F, B, cF, cB, (nF, nB))
    return _ANSWERS[k]


def _row_answer(orc, row):
    W, H, lv, seed, tau, _ = row
    L, R = _pair(W, H, seed)
    return L, R, _answer(orc, L, R, lv, tau, (W, H, seed))


def _premise(ans, W, H, what=""):
    nF, nB = ans[4]
    assert 0 < nF < W * H and 0 < nB < W * H, f"premise {what}: marked {nF} / {nB} of {W * H}"


def _nan_out(d, nfloats):
    """A device buffer of `nfloats` NaNs, freed with d.  (The fill stays referenced until the copy has returned: at 16 MP a temporary's pages
    go back to the system the moment it is dropped.)"""
    fill = np.full(nfloats, np.nan, np.float32)
    p = d.ctx.alloc(fill.nbytes)
    d.bufs.append(p)
    d.ctx.check(d.ctx.lib.ugsm_copy_to_device(d.ctx.handle, p, fill.ctypes.data, fill.nbytes))
    return p


def _checked(c, pairs, W, H, tau, back=True, slot=0, stride=None, dev=None):
    """One ugsm_submit_full_checked of `pairs` (host images, or (dL, dR) device pointers with `stride`) into NaN-filled buffers.
    back: True, or one flag per pair (False: a NULL d_back entry), or None (a NULL d_back).  Returns (outs, backs, counts)."""
    d = dev or Dev(c)
    try:
        n = len(pairs)
        if stride is None:
            put = [(d.put(L)[0], d.put(R)[0]) for L, R in pairs]
            stride = pairs[0][0].strides[0]
        else:
            put = pairs
        flags = None if back is None else ([back] * n if isinstance(back, bool) else list(back))
        dO = [_nan_out(d, 3 * W * H) for _ in range(n)]
        dB = None if flags is None else [_nan_out(d, 3 * W * H) if f else None for f in flags]
        c.submit_full_checked(slot, [p[0] for p in put], [p[1] for p in put], W, H, stride, dO, dB, tau)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        outs = [c.to_host(p, (3, H, W)) for p in dO]
        backs = [c.to_host(p, (3, H, W)) if p is not None else None for p in (dB or [None] * n)]
        return outs, backs, [c.last_lr_marked_pair(slot, k) for k in range(n)]
    finally:
        if dev is None:
            d.free()


def _assert_pair(ans, out, back, counts, what):
    F, B, cF, cB, marked = ans
    assert_bit_equal(out[:2], F[:2], f"{what}: dx, dy against the unchecked forward oracle field")
    assert_bit_equal(out[2], cF[2], f"{what}: the forward confidence against the oracle's checked one")
    if back is not None:
        assert_bit_equal(back[:2], B[:2], f"{what}: backward dx, dy against the unchecked backward oracle field")
        assert_bit_equal(back[2], cB[2], f"{what}: the backward confidence against the oracle's checked one")
    assert counts == marked, f"{what}: marked {counts} against the oracle's {marked}"


# ---- 1. the definition against the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_definition(lib, orc, row):
    W, H, lv, seed, tau, pinned = row
    L, R, ans = _row_answer(orc, row)
    assert ans[4] == pinned, ans[4]
    _premise(ans, W, H)
    with lib.Context(levels=lv) as c:
        outs, backs, counts = _checked(c, [(L, R)], W, H, tau)
        print(f"marked forward / backward: device {counts[0]}, oracle {ans[4]} of {W * H}")
        _assert_pair(ans, outs[0], backs[0], counts[0], f"{W}x{H} levels {lv}")
        assert c.last_lr_marked(0) == pinned[0]
        per = (C.c_longlong * 32)()
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, 0, per) == lib.UGSM_ERR_STATE
        f, b = C.c_longlong(), C.c_longlong()
        for bad in (1, -1):
            assert c.lib.ugsm_last_lr_marked_pair(c.handle, 0, bad, C.byref(f), C.byref(b)) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_last_lr_marked_pair(c.handle, 0, 0, None, None) == lib.UGSM_OK


# ---- 2. equal to the existing sequential form --------------------------------------------------------------------------------------------

def test_equal_to_the_sequential_form(lib, orc):
    W, H, lv, seed, tau, pinned = MID
    L, R, ans = _row_answer(orc, MID)
    _premise(ans, W, H)
    with lib.Context(levels=lv, lr_check_threshold=tau) as c:
        d = Dev(c)
        (pl, stride), (pr, _) = d.put(L), d.put(R)
        o = _nan_out(d, 3 * W * H)
        want = []
        for a, b in ((pl, pr), (pr, pl)):
            c.check(c.lib.ugsm_submit_full(c.handle, 0, a, b, W, H, stride, o))
            c.check(c.lib.ugsm_wait(c.handle, 0))
            want.append((c.to_host(o, (3, H, W)), c.last_lr_marked(0)))
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        assert c.lr_check == (np.float32(tau), lib.UGSM_LR_FULL)                       # the call left the context's setting alone
        d.free()
    assert_bit_equal(outs[0], want[0][0], "d_out against the context's own checked ugsm_submit_full(L, R)")
    assert_bit_equal(backs[0], want[1][0], "d_back against the context's own checked ugsm_submit_full(R, L)")
    assert counts[0] == (want[0][1], want[1][1]) == pinned


# ---- 3. batches --------------------------------------------------------------------------------------------------------------------------

def _distinct_pairs(n):
    W, H, lv, seed, tau, _ = SMALL
    return [_pair(W, H, seed + 10 * j) for j in range(n)]


@pytest.mark.parametrize("n", [3, 16])
def test_batches_of_distinct_pairs(lib, orc, n):
    """n = 16: 32 entries, so launches of sixteen.  Each pair against its own single checked call; pair 0 against the oracle too."""
    W, H, lv, seed, tau, pinned = SMALL
    pairs = _distinct_pairs(n)
    with lib.Context(levels=lv) as single, lib.Context(levels=lv, batch=n) as c:
        want = [_checked(single, [p], W, H, tau) for p in pairs]
        outs, backs, counts = _checked(c, pairs, W, H, tau)
    assert len({w[2][0] for w in want}) > 1, "premise: the pairs differ"
    for k in range(n):
        assert 0 < want[k][2][0][0] < W * H and 0 < want[k][2][0][1] < W * H, f"premise, pair {k}: {want[k][2][0]}"
        assert_bit_equal(outs[k], want[k][0][0], f"batch of {n}, pair {k}, d_out against its single checked call")
        assert_bit_equal(backs[k], want[k][1][0], f"batch of {n}, pair {k}, d_back against its single checked call")
        assert counts[k] == want[k][2][0], (k, counts[k], want[k][2][0])
    _assert_pair(_row_answer(orc, SMALL)[2], outs[0], backs[0], counts[0], f"batch of {n}, pair 0")
    assert counts[0] == pinned


@pytest.mark.parametrize("back", [(True, False, True), (False, False, False), None], ids=["mixed", "all-null-entries", "null-array"])
def test_null_back_entries(lib, orc, back):
    """A pair without a d_back buffer keeps its right-to-left field in the slot: d_out and both counts are what they are with one."""
    W, H, lv, seed, tau, pinned = SMALL
    pairs = _distinct_pairs(3)
    with lib.Context(levels=lv) as c:
        want = _checked(c, pairs, W, H, tau)
        outs, backs, counts = _checked(c, pairs, W, H, tau, back=back)
    assert counts == want[2] and counts[0] == pinned
    for k in range(3):
        assert_bit_equal(outs[k], want[0][k], f"pair {k}: d_out whatever becomes of the backward field")
        if back is not None and back[k]:
            assert_bit_equal(backs[k], want[1][k], f"pair {k}: d_back beside NULL entries")
    _assert_pair(_row_answer(orc, SMALL)[2], outs[0], None, counts[0], "pair 0")


# ---- 4. every kernel form ----------------------------------------------------------------------------------------------------------------

FORMS = {  # the context's configuration, the development variables
    "march-seeded": (dict(march_min_pixels=1, march_rows=7), {}),
    "march-plain": (dict(march_min_pixels=1), {"UGSM_FUSE_SEED": "0"}),
    "march4": (dict(march_min_pixels=1 << 30, small_max_pixels=-1), {}),
    "small": (dict(march_min_pixels=1 << 30, small_max_pixels=1 << 30), {}),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_kernel_form(lib, orc, monkeypatch, form):
    """A batch of three -- the pair, the pair exchanged, the pair -- whose level 0 (83 583 px) runs entry by entry as a 16 MP level 0 does,
    the levels below it in one launch each."""
    W, H, lv, seed, tau, pinned = BIG
    L, R, ans = _row_answer(orc, BIG)
    _premise(ans, W, H)
    F, B, cF, cB, (nF, nB) = ans
    swapped = (B, F, cB, cF, (nB, nF))
    cfg, env = FORMS[form]
    monkeypatch.setenv("UGSM_BATCH_MAX_PIXELS", "50000")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = lib.plan_level(W, H, **cfg)
    print(form, plan)
    with lib.Context(levels=lv, dev=True, **cfg) as c:
        outs, backs, counts = _checked(c, [(L, R), (R, L), (L, R)], W, H, tau)
        direct = c.lib.ugsm_stage_level0_direct(c.handle, 0)
    assert direct == (1 if form.startswith("march-") else 0), "level 0 from the image where k_cost_march matches it, else the float level 0"
    for k, a in enumerate((ans, swapped, ans)):
        _assert_pair(a, outs[k], backs[k], counts[k], f"{form}, pair {k}")


# ---- 5. inputs ---------------------------------------------------------------------------------------------------------------------------

def test_rgb8_level0_from_the_image_padded_and_odd(lib, orc):
    """Every level through k_cost_march: level 0 is read from the images, both directions and the A planes (ugsm_stage_level0_direct says so).
    Rows padded to a stride that is no multiple of 4, the images at odd addresses."""
    W, H, lv, seed, tau, pinned = SMALL
    L, R, ans = _row_answer(orc, SMALL)
    _premise(ans, W, H)
    with lib.Context(levels=lv, march_min_pixels=1, dev=True) as c:
        for pad, shift in ((0, 0), (7, 0), (5, 3)):
            d = Dev(c)
            (pl, stride), (pr, _) = d.put(L, pad, shift), d.put(R, pad, shift + (2 if shift else 0))
            assert stride == 3 * W + pad and (shift == 0 or (pl % 2 == 1 and pr % 2 == 1))
            outs, backs, counts = _checked(c, [(pl, pr), (pr, pl)], W, H, tau, stride=stride, dev=d)
            assert c.lib.ugsm_stage_level0_direct(c.handle, 0) == 1, "the call did not read level 0 from the images"
            d.free()
            _assert_pair(ans, outs[0], backs[0], counts[0], f"pad {pad} shift {shift}, pair 0")
            assert_bit_equal(outs[1], backs[0], "the exchanged pair's forward field is the pair's backward one")
            assert_bit_equal(backs[1], outs[0], "... and the other way round")
            assert counts[1] == counts[0][::-1]


@pytest.mark.parametrize("fmt", [en.BGR8, en.MONO8], ids=["bgr8", "mono8"])
def test_another_input_format(lib, orc, fmt):
    W, H, lv, seed, tau, _ = SMALL
    L, R = _pair(W, H, seed)
    eL, eR = en.encode(L, fmt), en.encode(R, fmt)
    cL, cR = en.to_rgb8(eL, fmt), en.to_rgb8(eR, fmt)
    ans = _answer(orc, cL, cR, lv, tau, ("fmt", fmt, W, H, seed))
    _premise(ans, W, H, en.NAMES[fmt])
    with lib.Context(levels=lv) as c:
        c.set_input_format(fmt)
        d = Dev(c)
        (pl, stride), (pr, _) = d.put(eL, 3, 1), d.put(eR, 3, 1)
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        d.free()
    _assert_pair(ans, outs[0], backs[0], counts[0], en.NAMES[fmt])


# ---- 6. the range word under exchanged views ---------------------------------------------------------------------------------------------

def test_the_range_word_serves_both_directions(lib, orc):
    """A dark, noisy pair trips the range word: both directions of both pairs take the full division, and the results are the oracle's."""
    W, H, lv, seed, tau, _ = MID
    L0, R0 = _pair(W, H, seed)
    L, R = dk.dark_pair(L0, R0, 77)
    word, cl, cr = dk.pair_word(orc, L, R, lv)
    assert word == 1 and (dk.trips(cl) or dk.trips(cr)), (cl, cr)
    ans, clean = _answer(orc, L, R, lv, tau, ("dark", W, H, seed)), _row_answer(orc, MID)[2]
    _premise(ans, W, H, "dark pair")
    with lib.Context(levels=lv, dev=True) as c:
        outs, backs, counts = _checked(c, [(L, R), (L0, R0)], W, H, tau)
        assert c.range_words(0, 2) == [1, 0], "the dark pair trips its word, the clean one does not (entry n + b runs under a copy of pair b's)"
    _assert_pair(ans, outs[0], backs[0], counts[0], "the dark pair")
    _assert_pair(clean, outs[1], backs[1], counts[1], "the clean pair beside it")


# ---- 7. refusals and memory --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_a_working_context(lib, orc):
    W, H, lv, seed, tau, _ = SMALL
    L, R, ans = _row_answer(orc, SMALL)

    def works(c, pl, pr, d, what):
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=3 * W, dev=d)
        _assert_pair(ans, outs[0], backs[0], counts[0], what)

    with lib.Context(levels=lv, slots=2) as c:
        d = Dev(c)
        pl, pr, o = d.put(L)[0], d.put(R)[0], _nan_out(d, 3 * W * H)
        ins, outs17, nul = (C.c_void_p * 17)(*([pl] * 17)), (C.c_void_p * 17)(*([o] * 17)), (C.c_void_p * 2)(o, None)
        c.set_lr_check(0.75, lib.UGSM_LR_FULL)

        def call(n=2, a=ins, b=ins, out=outs17, back=None, t=tau, w=W, h=H, stride=3 * W):
            return c.lib.ugsm_submit_full_checked(c.handle, 0, n, a, b, w, h, stride, out, back, t)
        hp = L.ctypes.data
        refused = [("tau 0", lambda: call(t=0.0), lib.UGSM_ERR_BAD_ARG), ("tau < 0", lambda: call(t=-1.0), lib.UGSM_ERR_BAD_ARG),
                   ("tau NaN", lambda: call(t=float("nan")), lib.UGSM_ERR_BAD_ARG), ("n 0", lambda: call(n=0), lib.UGSM_ERR_BAD_ARG),
                   ("n 17", lambda: call(n=17), lib.UGSM_ERR_BAD_ARG), ("null d_rgbL", lambda: call(a=None), lib.UGSM_ERR_BAD_ARG),
                   ("null d_rgbR", lambda: call(b=None), lib.UGSM_ERR_BAD_ARG), ("null d_out", lambda: call(out=None), lib.UGSM_ERR_BAD_ARG),
                   ("null entry of d_rgbL", lambda: call(a=nul), lib.UGSM_ERR_BAD_ARG), ("null entry of d_rgbR", lambda: call(b=nul), lib.UGSM_ERR_BAD_ARG),
                   ("null entry of d_out", lambda: call(out=nul), lib.UGSM_ERR_BAD_ARG),
                   ("short rows", lambda: call(stride=3 * W - 1), lib.UGSM_ERR_SIZE_MISMATCH), ("W 0", lambda: call(w=0), lib.UGSM_ERR_BAD_ARG),
                   ("too small for the levels", lambda: call(w=4, h=4, stride=12), lib.UGSM_ERR_TOO_SMALL),
                   ("blocking, tau 0", lambda: c.lib.ugsm_match_full_checked(c.handle, hp, hp, W, H, 3 * W, hp, hp, hp, None, None, None, 0.0), lib.UGSM_ERR_BAD_ARG),
                   ("blocking, one back plane", lambda: c.lib.ugsm_match_full_checked(c.handle, hp, hp, W, H, 3 * W, hp, hp, hp, hp, None, None, tau), lib.UGSM_ERR_BAD_ARG)]
        for name, f, status in refused:
            assert f() == status, name
            assert c.lr_check == (0.75, lib.UGSM_LR_FULL), name
        works(c, pl, pr, d, "after the refusals")
        # a pair outstanding in the queue: the slots are the queue's
        c.set_lr_check(0.0, 0)
        c.enqueue_full(pl, pr, W, H, 3 * W, o, 7)
        assert call() == lib.UGSM_ERR_STATE
        done = c.drain()
        assert [int(x.tag) for x in done] == [7] and done[0].status == 0
        works(c, pl, pr, d, "after the queue has drained")
        d.free()
    # contexts without a batch dimension (ugsm_set_lr_check's rule for the lockstep check)
    for cfg in (dict(early_exit_threshold=0.02), dict(kernel_path=1, dev=True)):
        with lib.Context(levels=lv, **cfg) as c:
            d = Dev(c)
            pl, pr, o = d.put(L)[0], d.put(R)[0], _nan_out(d, 3 * W * H)
            one = lambda p: (C.c_void_p * 1)(p)
            assert c.lib.ugsm_submit_full_checked(c.handle, 0, 1, one(pl), one(pr), W, H, 3 * W, one(o), None, tau) == lib.UGSM_ERR_BAD_ARG, cfg
            c.check(c.lib.ugsm_submit_full(c.handle, 0, pl, pr, W, H, 3 * W, o))         # the context still serves calls
            c.check(c.lib.ugsm_wait(c.handle, 0))
            d.free()


def _plain(c, pl, pr, W, H, stride, d):
    o = _nan_out(d, 3 * W * H)
    c.check(c.lib.ugsm_submit_full(c.handle, 0, pl, pr, W, H, stride, o))
    c.check(c.lib.ugsm_wait(c.handle, 0))
    return c.to_host(o, (3, H, W))


def test_buffers_that_cannot_grow_and_the_bytes_of_those_that_can(lib, orc, monkeypatch):
    """A one-pair slot at 333 x 251 holds 3 x 1 MB of level buffers; the checked call of one pair needs 3 x 2 fields (counted, exactly), that
    of sixteen 3 x 32 MB: under the development limit UGSM_MEM_LIMIT_MB the latter answers UGSM_ERR_NOMEM before anything is enqueued and the
    slot serves the next call."""
    W, H, lv, seed, tau, _ = BIG
    L, R, ans = _row_answer(orc, BIG)
    field = (3 * W * H + 63) // 64 * 64
    monkeypatch.setenv("UGSM_MEM_LIMIT_MB", "24")
    with lib.Context(levels=lv) as c:
        d = Dev(c)
        (pl, stride), (pr, _) = d.put(L), d.put(R)
        assert_bit_equal(_plain(c, pl, pr, W, H, stride, d), ans[0], "a plain call first")
        before = c.device_bytes()
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        _assert_pair(ans, outs[0], backs[0], counts[0], "one pair under the limit")
        held = c.device_bytes()
        assert held - before == 3 * (2 * field - 3 * W * H) * 4 + 2 * 8, "A, d0 and d1 grew from one field to two; the LR buffer holds the two count words"
        assert held < 24e6, held
        o = _nan_out(d, 3 * W * H)
        many_in, many_out = (C.c_void_p * 16)(*([pl] * 16)), (C.c_void_p * 16)(*([o] * 16))
        st = c.lib.ugsm_submit_full_checked(c.handle, 0, 16, many_in, many_in, W, H, stride, many_out, many_out, tau)
        assert st == lib.UGSM_ERR_NOMEM, st
        assert b"hipMalloc" in c.lib.ugsm_last_error(c.handle)
        assert c.device_bytes() < held, "the level buffers were given back whole"
        c.check(c.lib.ugsm_wait(c.handle, 0))
        assert_bit_equal(_plain(c, pl, pr, W, H, stride, d), ans[0], "a plain call after the refused one")
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        _assert_pair(ans, outs[0], backs[0], counts[0], "a checked call after the refused one")
        d.free()


# ---- 8. nothing left behind --------------------------------------------------------------------------------------------------------------

def test_nothing_left_behind(lib, orc):
    W, H, lv, seed, tau, _ = MID
    L, R, ans = _row_answer(orc, MID)
    with lib.Context(levels=lv) as c:
        d = Dev(c)
        (pl, stride), (pr, _) = d.put(L), d.put(R)
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        _assert_pair(ans, outs[0], backs[0], counts[0], "the checked call")
        assert_bit_equal(_plain(c, pl, pr, W, H, stride, d), ans[0], "a plain ugsm_submit_full on the same slot afterwards")
        assert c.last_lr_marked(0) == -1
        f = C.c_longlong()
        assert c.lib.ugsm_last_lr_marked_pair(c.handle, 0, 0, C.byref(f), None) == lib.UGSM_ERR_STATE
        outs, backs, counts = _checked(c, [(pl, pr)], W, H, tau, stride=stride, dev=d)
        _assert_pair(ans, outs[0], backs[0], counts[0], "a checked call after the plain one")
        d.free()


def test_the_blocking_form_and_the_shim(lib, orc):
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    W, H, lv, seed, tau, pinned = MID
    L, R, ans = _row_answer(orc, MID)
    with lib.Context(levels=lv) as c:
        fwd, bwd = c.match_full_checked(L, R, tau)
        _assert_pair(ans, fwd, bwd, c.last_lr_marked_pair(0, 0), "the blocking form with the backward planes")
        fwd, none = c.match_full_checked(L, R, tau, back=False)
        assert none is None
        _assert_pair(ans, fwd, None, c.last_lr_marked_pair(0, 0), "the blocking form without them")
    m = MatchGPULib(levels=lv)
    try:
        fwd, bwd = m.match(L, R, 0, tau)
        plain = m.match(L, R, 0)
    finally:
        m.close()
    _assert_pair(ans, fwd, bwd, pinned, "MatchGPULib.match(.., tau)")
    assert_bit_equal(plain, ans[0], "MatchGPULib.match without tau")


# ---- 9. one full-size run ----------------------------------------------------------------------------------------------------------------

def test_16mp(lib, orc, oracle_16mp):
    o = oracle_16mp
    W, H, L, R, tau = o["W"], o["H"], o["L"], o["R"], 1.0
    orc.set_num_threads(16)
    try:
        ans = _answer(orc, L, R, 14, tau, "16mp", fwd=o["full"])
    finally:
        orc.set_num_threads(8)
    _premise(ans, W, H, "16 MP")
    with lib.Context(levels=14, dev=True) as c:
        outs, backs, counts = _checked(c, [(L, R)], W, H, tau)
        assert c.lib.ugsm_stage_level0_direct(c.handle, 0) == 1, "a 16 MP rgb8 call reads level 0 from the images"
    print(f"16 MP, tau {tau}: marked forward / backward {counts[0]} of {W * H}; the oracle's {ans[4]}")
    _assert_pair(ans, outs[0], backs[0], counts[0], "16 MP")
