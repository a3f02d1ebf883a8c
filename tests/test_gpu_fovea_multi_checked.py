"""The checked multi-window call: ugsm_submit_foveated_multi_checked, ugsm_match_foveated_multi_checked.

The definition (include/ugsm.h): stack k is, bit for bit, what ugsm_submit_foveated writes for offset k on a context with
ugsm_set_lr_check(ctx, tau, UGSM_LR_FOVEATED).  So per window the oracle is orc.match_foveated(L, R, .., off_k), orc.match_foveated(R, L, ..,
off_k) and orc.lr_check on each level's (3, fovH, fovW) slice, as tests/test_gpu_lr_fovea.py builds it; every comparison is bit-exact.  The
definition test asserts its premise from the oracle alone: on every level of every window the check both fires and spares.  The shapes are
small because the CPU oracle runs 2 n foveated matches for each."""
import ctypes as C

import numpy as np
import pytest

import cloud_np as cn
import encode_np as en
import multi_cloud_np as mn
import reconstruct_multi_np as rm
from conftest import assert_bit_equal
from test_gpu_cloud import P1, P2
from test_gpu_fovea_multi import OFFS
from test_gpu_fovea_multi import _pair as _patched_pair
from test_gpu_lr_fovea import _checked

pytestmark = pytest.mark.gpu

SEED = 4100
CENTRED, CLAMPS, CLAMPS_TOO, OVERLAPS, OFF_CENTRE = OFFS[0], OFFS[2], OFFS[3], OFFS[6], OFFS[1]
assert (CENTRED, OVERLAPS) == ((0, 0), (20, 10)) and CLAMPS == (5000, -5000) and CLAMPS_TOO == (-5000, 5000) and OFFS[4] == CENTRED

ROWS = [  # W, H, levels, F, offsets, tau, (fovW, fovH), the CPU oracle's marked pixels per window and level 0 .. F-1
    (320, 240, 9, 4, [CENTRED, CLAMPS, OVERLAPS], 1.0, (112, 84), [[308, 329, 362, 1434], [2925, 2315, 1442, 1434], [302, 240, 381, 1434]]),
    # 2 n = 10 fields of 3 x 99 x 74 floats exceed a one-pair slot's 3 x 200 x 150: the level buffers must grow
    (200, 150, 8, 3, [CENTRED, OFF_CENTRE, CLAMPS, OFFS[4], OVERLAPS], 1.0, (99, 74),
     [[266, 495, 1669], [1250, 881, 1669], [2692, 1963, 1669], [266, 495, 1669], [161, 301, 1669]]),
    # F = 2: the right-to-left stack cannot sit in the level buffers, and the coarse phase hands over at level 1
    (333, 251, 8, 2, [CLAMPS_TOO, OVERLAPS], 0.5, (235, 177), [[5837, 4531], [4689, 4531]]),
    # the coarse phase is the top level alone
    (200, 150, 5, 5, [CENTRED, OVERLAPS], 1.0, (49, 36), [[105, 172, 150, 241, 195], [96, 99, 190, 199, 195]]),
]
IDS = [f"{r[0]}x{r[1]}-F{r[3]}-n{len(r[4])}-tau{r[5]}" for r in ROWS]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


_PAIRS, _ANSWERS = {}, {}


def _pair(W, H):
    if (W, H) not in _PAIRS:
        from ug_stereomatcher_amd import synth
        _PAIRS[(W, H)] = synth.make_pair(W, H, synth.BASE_SEED + SEED)[:2]
    return _PAIRS[(W, H)]


def _answer(orc, L, R, lv, F, off, tau, key=None):
    """(S, checked S, marked per level) of one window from the oracle, computed once per (pair, configuration, offset, tau) and shared."""
    k = (key or id(L), L.shape, lv, F, tuple(off), tau)
    if k not in _ANSWERS:
        S = orc.match_foveated(L, R, lv, F, off[0], off[1])[0]
        B = orc.match_foveated(R, L, lv, F, off[0], off[1])[0]
        chk, counts = _checked(orc, S, B, tau)
        for a in (S, chk):
            a.setflags(write=False)
        _ANSWERS[k] = (S, chk, counts)
    return _ANSWERS[k]


def _multi(c, lib, dL, dR, W, H, stride, lv, F, offs, tau, slot=0, wait=True):
    """One checked call into zeroed stacks -> the stacks and the counts of every window (or, wait=False, a function that fetches them)."""
    fw, fh = lib.fovea_dims(W, H, lv, F)
    dS = [c.to_device(np.zeros(3 * F * fh * fw, np.float32)) for _ in offs]
    c.submit_foveated_multi_checked(slot, dL, dR, W, H, stride, offs, dS, tau)

    def fetch():
        try:
            return [c.to_host(p, (3, F, fh, fw)) for p in dS], [c.last_lr_marked_levels(slot, k) for k in range(len(offs))]
        finally:
            for p in dS:
                c.free(p)
    if not wait:
        return fetch
    c.check(c.lib.ugsm_wait(c.handle, slot))
    return fetch()


def _run(c, lib, L, R, lv, F, offs, tau, slot=0):
    H, W = L.shape[:2]
    dL, dR = c.to_device(L), c.to_device(R)
    try:
        return _multi(c, lib, dL, dR, W, H, L.strides[0], lv, F, offs, tau, slot)
    finally:
        c.free(dL)
        c.free(dR)


def _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, what, key=None):
    for k, off in enumerate(offs):
        S, chk, marked = _answer(orc, L, R, lv, F, off, tau, key)
        assert_bit_equal(got[k][2], chk[2], f"{what}: window {k} at {off}, stackC against the oracle's checked confidence")
        assert_bit_equal(got[k][:2], S[:2], f"{what}: window {k} at {off}, stackH / stackV against the forward oracle stack")
        assert counts[k] == marked, f"{what}: window {k} at {off}, marked per level {counts[k]} against the oracle's {marked}"
    for k in range(1, len(offs)):
        assert_bit_equal(got[k][:, F - 1], got[0][:, F - 1], f"{what}: row block F-1 is the same checked whole-frame level in every stack")


# ---- 1. the definition against the oracle ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,lv,F,offs,tau,fov,marked", ROWS, ids=IDS)
def test_definition(lib, orc, W, H, lv, F, offs, tau, fov, marked):
    L, R = _pair(W, H)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    oracle_counts = [_answer(orc, L, R, lv, F, off, tau)[2] for off in offs]
    assert (fw, fh) == fov and oracle_counts == marked, (fw, fh, oracle_counts)
    assert all(0 < m < fw * fh for per in oracle_counts for m in per), f"premise: marked per level {oracle_counts} of {fw * fh}"
    with lib.Context(levels=lv, fovea_levels=F) as c:
        before = c.device_bytes()
        got, counts = _run(c, lib, L, R, lv, F, offs, tau)
        print(f"marked per window and level: device {counts}, oracle {oracle_counts}")
        _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, f"{W}x{H} levels {lv} F {F}")
        assert c.last_lr_marked(0) == sum(marked[-1])                                   # "the levels of the last entry": window n-1
        per = (C.c_longlong * 32)()
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, len(offs), per) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, -1, per) == lib.UGSM_ERR_BAD_ARG
        field = 3 * fw * fh
        if 2 * len(offs) * field > 3 * W * H:
            assert c.device_bytes() >= before + 3 * 2 * len(offs) * field * 4, "A, d0 and d1 each hold 2 n fields"


# ---- 2. n = 1 .. 16 against checked single calls on the device ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 16])
def test_every_n_equals_checked_single_calls(lib, n):
    """n = 16 puts 32 virtual pairs through launches of at most sixteen.  (The pair has a zero patch: NaN correlations on both sides.)"""
    W, H, lv, F, tau = 640, 480, 10, 4, 1.0
    L, R = _patched_pair(W, H)
    offs = OFFS[:n]
    fw, fh = lib.fovea_dims(W, H, lv, F)
    with lib.Context(levels=lv, fovea_levels=F) as c, lib.Context(levels=lv, fovea_levels=F) as single:
        single.set_lr_check(tau, lib.UGSM_LR_FOVEATED)
        dL, dR = single.to_device(L), single.to_device(R)
        dS = single.alloc(3 * F * fh * fw * 4)
        want = []
        for off in offs:
            single.check(single.lib.ugsm_submit_foveated(single.handle, 0, dL, dR, W, H, 3 * W, off[0], off[1], dS, None, None))
            single.check(single.lib.ugsm_wait(single.handle, 0))
            want.append((single.to_host(dS, (3, F, fh, fw)), single.last_lr_marked_levels(0, 0)))
        for p in (dL, dR, dS):
            single.free(p)
        got, counts = _run(c, lib, L, R, lv, F, offs, tau)
        assert c.lr_check == (0.0, lib.UGSM_LR_FULL)                                   # the call left the context's setting alone
    assert all(0 < m for w in want for m in w[1]), "the check fires on every level of the single calls"
    for k, off in enumerate(offs):
        assert_bit_equal(got[k], want[k][0], f"{n} windows, window {k} at {off} against its checked single call")
        assert counts[k] == want[k][1], (k, counts[k], want[k][1])


# ---- 3. every kernel form on the fine levels ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force", ["march", "march4", "shared", "no_fused_seed", "alone"])
def test_every_kernel_form_on_the_fine_levels(lib, orc, monkeypatch, force):
    env = {"march": {"UGSM_MARCH_MIN_PIXELS": "1"}, "march4": {"UGSM_MARCH4": "1,2000000000"}, "shared": {"UGSM_ALONE": "0"},
           "no_fused_seed": {"UGSM_FUSE_SEED": "0"}, "alone": {"UGSM_ALONE": "1"}}[force]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W, H, lv, F, offs, tau = ROWS[0][:6]
    L, R = _pair(W, H)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        got, counts = _run(c, lib, L, R, lv, F, offs, tau)
    _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, force)


# ---- 4. another input format -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [en.BGR8, en.MONO8], ids=["bgr8", "mono8"])
def test_another_input_format(lib, orc, fmt):
    W, H, lv, F, offs, tau = ROWS[0][:6]
    offs = offs[:2]
    L, R = _pair(W, H)
    eL, eR = en.encode(L, fmt), en.encode(R, fmt)
    cL, cR = np.ascontiguousarray(en.to_rgb8(eL, fmt)), np.ascontiguousarray(en.to_rgb8(eR, fmt))
    fw, fh = lib.fovea_dims(W, H, lv, F)
    for off in offs:
        marked = _answer(orc, cL, cR, lv, F, off, tau, key=("fmt", fmt))[2]
        assert all(0 < m < fw * fh for m in marked), f"premise: {marked}"
    with lib.Context(levels=lv, fovea_levels=F) as c:
        c.set_input_format(fmt)
        dL, dR = c.to_device(eL), c.to_device(eR)
        got, counts = _multi(c, lib, dL, dR, W, H, en.BPP[fmt] * W, lv, F, offs, tau)
        c.free(dL)
        c.free(dR)
    _assert_definition(orc, cL, cR, lv, F, offs, tau, got, counts, en.NAMES[fmt], key=("fmt", fmt))


# ---- 5. the slot afterwards --------------------------------------------------------------------------------------------------------------

def _plain(c, lib, dL, dR, W, H, lv, F, offs, slot=0):
    fw, fh = lib.fovea_dims(W, H, lv, F)
    dS = [c.alloc(3 * F * fh * fw * 4) for _ in offs]
    try:
        c.submit_foveated_multi(slot, dL, dR, W, H, 3 * W, offs, dS)
        c.check(c.lib.ugsm_wait(c.handle, slot))
        return [c.to_host(p, (3, F, fh, fw)) for p in dS]
    finally:
        for p in dS:
            c.free(p)


def test_the_slot_afterwards(lib, orc):
    W, H, lv, F, offs, tau = ROWS[0][:6]
    L, R = _pair(W, H)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    per = (C.c_longlong * 32)()
    with lib.Context(levels=lv, fovea_levels=F, slots=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        got, counts = _multi(c, lib, dL, dR, W, H, 3 * W, lv, F, offs, tau)
        _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, "first checked call")
        # ugsm_submit_fovea_fine: the slot holds no whole pyramids
        dS, dT = c.alloc(3 * F * fh * fw * 4), c.alloc(3 * fh * fw * 4)
        assert c.lib.ugsm_submit_fovea_fine(c.handle, 0, dT, 0, 0, dS) == lib.UGSM_ERR_STATE
        # a plain multi call on the same slot: the unchecked stacks, no counts
        plain = _plain(c, lib, dL, dR, W, H, lv, F, offs)
        for k, off in enumerate(offs):
            assert_bit_equal(plain[k], _answer(orc, L, R, lv, F, off, tau)[0], f"plain multi call after a checked one, window {k}")
        assert c.last_lr_marked(0) == -1
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, 0, per) == lib.UGSM_ERR_STATE
        # a checked call after the plain one, with the windows in another order
        back = offs[::-1]
        got, counts = _multi(c, lib, dL, dR, W, H, 3 * W, lv, F, back, tau)
        _assert_definition(orc, L, R, lv, F, back, tau, got, counts, "checked call after a plain one")
        # two checked calls on two slots in flight
        sets = [offs[:2], offs[1:]]
        fetch = [_multi(c, lib, dL, dR, W, H, 3 * W, lv, F, sets[s], tau, slot=s, wait=False) for s in range(2)]
        c.check(c.lib.ugsm_wait_all(c.handle))
        for s in range(2):
            got, counts = fetch[s]()
            _assert_definition(orc, L, R, lv, F, sets[s], tau, got, counts, f"two slots in flight, slot {s}")
        for p in (dL, dR, dS, dT):
            c.free(p)


# ---- 6. the blocking form ----------------------------------------------------------------------------------------------------------------

def test_the_blocking_form_from_pageable_memory(lib, orc):
    W, H, lv, F, offs, tau = ROWS[0][:6]
    L, R = _pair(W, H)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        host = c.match_foveated_multi_checked(L, R, offs, tau)
        host_counts = [c.last_lr_marked_levels(0, k) for k in range(len(offs))]
        dev, dev_counts = _run(c, lib, L, R, lv, F, offs, tau)
    for k in range(len(offs)):
        assert_bit_equal(host[k], dev[k], f"blocking form vs slot form, window {k}")
    assert host_counts == dev_counts
    _assert_definition(orc, L, R, lv, F, offs, tau, host, host_counts, "blocking form")


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_a_working_context(lib, orc):
    W, H, lv, F, offs, tau = ROWS[0][:6]
    offs = offs[:2]
    L, R = _pair(W, H)
    fw, fh = lib.fovea_dims(W, H, lv, F)

    def works(c, dL, dR, what):
        got, counts = _multi(c, lib, dL, dR, W, H, 3 * W, lv, F, offs, tau)
        _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, what)
        return got

    with lib.Context(levels=lv, fovea_levels=F, slots=2) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        dS = c.alloc(3 * F * fh * fw * 4)
        many = (C.c_void_p * 17)(*([dS] * 17))
        c.set_lr_check(0.75, lib.UGSM_LR_FULL)
        call = lambda n, ptrs, t=tau, stride=3 * W: c.lib.ugsm_submit_foveated_multi_checked(c.handle, 0, dL, dR, W, H, stride, n, None, None, ptrs, t)
        hp = (C.c_void_p * 2)(dS, dS)
        refused = [("tau 0", lambda: call(2, many, 0.0), lib.UGSM_ERR_BAD_ARG), ("tau < 0", lambda: call(2, many, -1.0), lib.UGSM_ERR_BAD_ARG),
                   ("tau NaN", lambda: call(2, many, float("nan")), lib.UGSM_ERR_BAD_ARG), ("n 0", lambda: call(0, many), lib.UGSM_ERR_BAD_ARG),
                   ("n 17", lambda: call(17, many), lib.UGSM_ERR_BAD_ARG),
                   ("null entry", lambda: call(2, (C.c_void_p * 2)(dS, None)), lib.UGSM_ERR_BAD_ARG),
                   ("null array", lambda: call(2, None), lib.UGSM_ERR_BAD_ARG),
                   ("short rows", lambda: call(1, many, stride=W), lib.UGSM_ERR_SIZE_MISMATCH),
                   ("blocking, tau 0", lambda: c.lib.ugsm_match_foveated_multi_checked(c.handle, L.ctypes.data, R.ctypes.data, W, H, 3 * W, 2, None, None,
                                                                                      hp, hp, hp, 0.0), lib.UGSM_ERR_BAD_ARG)]
        for name, f, status in refused:
            assert f() == status, name
            assert c.lr_check == (0.75, lib.UGSM_LR_FULL), name
            works(c, dL, dR, f"after the refusal '{name}'")
        # the context's own setting neither enables nor disturbs the checked call; the plain multi call under it is still refused
        off_result = works(c, dL, dR, "UGSM_LR_FOVEATED off")
        c.set_lr_check(2.5, lib.UGSM_LR_FOVEATED)
        on_result = works(c, dL, dR, "UGSM_LR_FOVEATED on, at another tau")
        for k in range(len(offs)):
            assert_bit_equal(on_result[k], off_result[k], f"the setting on and off, window {k}")
        assert c.lr_check == (2.5, lib.UGSM_LR_FOVEATED)
        assert c.lib.ugsm_submit_foveated_multi(c.handle, 0, dL, dR, W, H, 3 * W, 2, None, None, many) == lib.UGSM_ERR_STATE
        c.set_lr_check(0.0, 0)
        # a pair outstanding in the queue: the slots are the queue's
        c.enqueue_foveated(dL, dR, W, H, 3 * W, (0, 0), dS, 7)
        assert call(2, many) == lib.UGSM_ERR_STATE
        done = c.drain()
        assert [int(d.tag) for d in done] == [7] and done[0].status == 0
        works(c, dL, dR, "after the queue has drained")
        for p in (dL, dR, dS):
            c.free(p)
    # contexts without a batch dimension, and contexts without a fovea
    for cfg in (dict(early_exit_threshold=0.02), dict(kernel_path=1, dev=True), dict(fovea_levels=1)):
        with lib.Context(**{**dict(levels=lv, fovea_levels=F), **cfg}) as c:
            dL, dR = c.to_device(L), c.to_device(R)
            dS = c.alloc(3 * W * H * 4)
            one = (C.c_void_p * 1)(dS)
            before = c.lr_check
            assert c.lib.ugsm_submit_foveated_multi_checked(c.handle, 0, dL, dR, W, H, 3 * W, 1, None, None, one, tau) == lib.UGSM_ERR_BAD_ARG, cfg
            assert c.lr_check == before
            c.check(c.lib.ugsm_submit_full(c.handle, 0, dL, dR, W, H, 3 * W, dS))         # the context still serves calls
            c.check(c.lib.ugsm_wait(c.handle, 0))
            for p in (dL, dR, dS):
                c.free(p)


def test_buffers_that_cannot_grow(lib, orc, monkeypatch):
    """F = 2: 32 fields of 235 x 177 need 3 x 16 MB of level buffers.  Under the development limit UGSM_MEM_LIMIT_MB (the branch a failed
    hipMalloc takes) the call answers UGSM_ERR_NOMEM before anything is enqueued, keeps no half-grown buffer, and the slot serves the next
    call."""
    W, H, lv, F, offs, tau = ROWS[2][:6]
    L, R = _pair(W, H)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    monkeypatch.setenv("UGSM_MEM_LIMIT_MB", "20")
    with lib.Context(levels=lv, fovea_levels=F) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        got, counts = _multi(c, lib, dL, dR, W, H, 3 * W, lv, F, offs, tau)
        _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, "before")
        held = c.device_bytes()
        assert held < 20e6, held
        dS = c.alloc(3 * F * fh * fw * 4)
        many = (C.c_void_p * 16)(*([dS] * 16))
        st = c.lib.ugsm_submit_foveated_multi_checked(c.handle, 0, dL, dR, W, H, 3 * W, 16, None, None, many, tau)
        assert st == lib.UGSM_ERR_NOMEM, st
        assert b"hipMalloc" in c.lib.ugsm_last_error(c.handle)
        assert c.device_bytes() < held, "the level buffers were given back whole"
        c.check(c.lib.ugsm_wait(c.handle, 0))
        got, counts = _multi(c, lib, dL, dR, W, H, 3 * W, lv, F, offs, tau)
        _assert_definition(orc, L, R, lv, F, offs, tau, got, counts, "after the refused call")
        for p in (dL, dR, dS):
            c.free(p)


# ---- 8. downstream of the checked stacks -------------------------------------------------------------------------------------------------

def test_cloud_and_reconstruction_from_the_checked_stacks(lib, orc):
    W, H, lv, F, offs, tau = ROWS[0][:6]
    L, R = _pair(W, H)
    plain = [_answer(orc, L, R, lv, F, off, tau)[0] for off in offs]
    chk = [_answer(orc, L, R, lv, F, off, tau)[1] for off in offs]
    want, want_per = mn.cloud_fovea_multi(orc, chk, L, offs, P1, P2, compact=True, min_conf=0.2)
    unchecked, _ = mn.cloud_fovea_multi(orc, plain, L, offs, P1, P2, compact=True, min_conf=0.2)
    assert 0 < want.size < unchecked.size, "premise: the marked pixels leave the compact cloud"
    E = (F - 1) * len(offs) + 1
    with lib.Context(levels=lv, fovea_levels=F) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        d_stacks = [c.alloc(chk[0].nbytes) for _ in offs]
        d_pts, d_cnt, d_ent, dO = c.alloc(unchecked.size * 32), c.alloc(8), c.alloc(8 * E), c.alloc(3 * W * H * 4)
        params = lib.cloud_params(compact=True, min_conf=0.2)
        c.submit_foveated_multi_checked(0, dL, dR, W, H, 3 * W, offs, d_stacks, tau)
        n, per = c.point_cloud_fovea_multi(d_stacks, W, H, offs, dL, 3 * W, P1, P2, params, d_pts, unchecked.size, d_cnt, d_ent)   # (stream order)
        assert n == want.size and per == want_per
        cn.assert_cloud_equal(c.cloud_to_host(d_pts, n), want, "the compact cloud of the checked stacks")
        c.reconstruct_full_multi(d_stacks, W, H, dO, offs)
        assert_bit_equal(c.to_host(dO, (3, H, W)), rm.reconstruct_multi(orc, chk, W, H, lv, offs), "reconstruction from the checked stacks")
        c.submit_foveated_multi(0, dL, dR, W, H, 3 * W, offs, d_stacks)
        n_plain = c.point_cloud_fovea_multi(d_stacks, W, H, offs, dL, 3 * W, P1, P2, params, d_pts, unchecked.size, d_cnt)
        assert n_plain == unchecked.size and n < n_plain, "strictly fewer records than on the unchecked stacks"
        for p in [dL, dR, d_pts, d_cnt, d_ent, dO] + d_stacks:
            c.free(p)


# ---- 9. the shim -------------------------------------------------------------------------------------------------------------------------

def test_match_gpu_lib_match_stack_multi_with_tau(lib, orc):
    """MatchGPULib.matchStackMulti(.., tau): one [level][dx|dy|conf] stack per window, each the C call's."""
    from ug_stereomatcher_amd.match_gpu_lib import MatchGPULib
    W, H, lv, F, offs, tau = ROWS[0][:6]
    L, R = _pair(W, H)
    m = MatchGPULib(3, ["node", "x", str(F)], levels=lv)
    try:
        got = m.matchStackMulti(L, R, offs, tau)
        assert (m.getFoveaWidth(), m.getFoveaHeight()) == lib.fovea_dims(W, H, lv, F)
        unchecked = m.matchStackMulti(L, R, offs)
    finally:
        m.close()
    with lib.Context(levels=lv, fovea_levels=F) as c:
        want = c.match_foveated_multi_checked(L, R, offs, tau)
    for k, off in enumerate(offs):
        assert_bit_equal(got[k], want[k].transpose(1, 0, 2, 3), f"matchStackMulti with tau, window {k} against the C call")
        assert_bit_equal(got[k], _answer(orc, L, R, lv, F, off, tau)[1].transpose(1, 0, 2, 3), f"matchStackMulti with tau, window {k} against the oracle")
        assert_bit_equal(unchecked[k], _answer(orc, L, R, lv, F, off, tau)[0].transpose(1, 0, 2, 3), f"matchStackMulti without tau, window {k}")
