"""The LR check of the foveated calls (ugsm_set_lr_check, UGSM_LR_FOVEATED): both directions of a foveated call in one lockstep call.

The definition (include/ugsm.h): with S the stack of the call and B the stack of the same call with the two images exchanged, level k of S
is checked against level k of B as ugsm_stage_lr_check checks a fovW x fovH field; only the confidence changes.  The oracle is therefore
orc.match_foveated(L, R, ..), orc.match_foveated(R, L, ..) and orc.lr_check on each level's (3, fovH, fovW) slice, and every comparison is
bit-exact.  Each definition test first asserts its premise: on every level the check both fires and spares (0 < marked < fovW * fovH).
However the pairs are grouped -- single calls, batches, page-locked calls, the queue -- the result is the same.
"""
import ctypes as C

import numpy as np
import pytest

import dark_np as dk
import encode_np as en
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_library()
    from ug_stereomatcher_amd import _lib
    return _lib


def _pair(W, H, seed):
    from ug_stereomatcher_amd import synth
    return synth.make_pair(W, H, synth.BASE_SEED + seed)[:2]


def _checked(orc, S, B, tau):
    """(the checked stack, marked per level) of the forward stack S and the backward stack B, both (3, F, fovH, fovW)."""
    out, counts = S.copy(), []
    for k in range(S.shape[1]):
        lvl, m = orc.lr_check(np.ascontiguousarray(S[:, k]), np.ascontiguousarray(B[:, k]), tau)
        assert_bit_equal(lvl[:2], S[:2, k], "the oracle's check leaves dx, dy alone")
        out[2, k] = lvl[2]
        counts.append(m)
    return out, counts


def _oracle(orc, L, R, lv, F, off, tau, want_pyr=False):
    """(S, checked S, marked per level, pyrL, pyrR); the premise -- the check fires and spares on every level -- asserted."""
    S, pl, pr = orc.match_foveated(L, R, lv, F, off[0], off[1], want_pyr=want_pyr)
    B = orc.match_foveated(R, L, lv, F, off[0], off[1])[0]
    chk, counts = _checked(orc, S, B, tau)
    px = S.shape[2] * S.shape[3]
    assert all(0 < m < px for m in counts), f"premise: marked per level {counts} of {px}"
    return S, chk, counts, pl, pr


def _submit(c, slot, dL, dR, W, H, off, dS, dPL=None, dPR=None, stride=None):
    c.check(c.lib.ugsm_submit_foveated(c.handle, slot, dL, dR, W, H, stride or 3 * W, off[0], off[1], dS, dPL, dPR))
    c.check(c.lib.ugsm_wait(c.handle, slot))


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------

ROWS = [  # W, H, levels, F, offset, seed, tau, (fovW, fovH), the CPU oracle's marked pixels per level 0 .. F-1
    (320, 240, 9, 4, (0, 0), 4100, 1.0, (112, 84), [308, 329, 362, 1434]),
    (320, 240, 9, 4, (17, -9), 4101, 0.5, (112, 84), [1607, 758, 774, 1809]),
    (640, 480, 11, 5, (-40, 25), 4102, 1.0, (159, 118), [360, 439, 336, 437, 1584]),
    (200, 150, 8, 3, (0, 0), 4103, 1.0, (99, 74), [288, 231, 957]),
]


@pytest.mark.parametrize("W,H,lv,F,off,seed,tau,fov,marked", ROWS, ids=[f"{r[0]}x{r[1]}-F{r[3]}-tau{r[6]}" for r in ROWS])
def test_definition(lib, orc, W, H, lv, F, off, seed, tau, fov, marked):
    L, R = _pair(W, H, seed)
    S, chk, counts, pl, pr = _oracle(orc, L, R, lv, F, off, tau, want_pyr=True)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    assert (fw, fh) == fov and counts == marked, (fw, fh, counts)
    with lib.Context(levels=lv, fovea_levels=F) as c:
        dL, dR = c.to_device(L), c.to_device(R)
        n = 3 * F * fh * fw * 4
        dS, dPL, dPR = c.alloc(n), c.alloc(n), c.alloc(n)
        _submit(c, 0, dL, dR, W, H, off, dS, dPL, dPR)                  # unchecked: the pyramid stacks to compare with
        assert_bit_equal(c.to_host(dS, (3, F, fh, fw)), S, "the unchecked call")
        plain_pl, plain_pr = c.to_host(dPL, (F, 3, fh, fw)), c.to_host(dPR, (F, 3, fh, fw))
        assert c.last_lr_marked(0) == -1
        c.set_lr_check(tau, lib.UGSM_LR_FOVEATED)
        for q in (dS, dPL, dPR):
            c.check(c.lib.ugsm_copy_to_device(c.handle, q, np.zeros(n // 4, np.float32).ctypes.data, n))
        _submit(c, 0, dL, dR, W, H, off, dS, dPL, dPR)
        got = c.to_host(dS, (3, F, fh, fw))
        print(f"marked per level: device {c.last_lr_marked_levels(0, 0)}, oracle {counts}")
        assert_bit_equal(got[2], chk[2], "stackC against the oracle's checked confidence")
        assert_bit_equal(got[:2], S[:2], "stackH / stackV against the forward oracle stack")
        assert c.last_lr_marked_levels(0, 0) == counts
        assert c.last_lr_marked(0) == sum(counts)
        assert_bit_equal(c.to_host(dPL, (F, 3, fh, fw)), plain_pl, "left pyramid stack against the unchecked call's")
        assert_bit_equal(c.to_host(dPR, (F, 3, fh, fw)), plain_pr, "right pyramid stack against the unchecked call's")
        assert_bit_equal(plain_pl, pl, "left pyramid stack against the oracle's")
        assert_bit_equal(plain_pr, pr, "right pyramid stack against the oracle's")
        for q in (dL, dR, dS, dPL, dPR):
            c.free(q)


# ---- 2. full size, and the range word under exchanged views ------------------------------------------------------------------------------

def test_16mp(lib, orc, oracle_16mp):
    g = oracle_16mp
    W, H, lv, F, tau = g["W"], g["H"], 14, 7, 1.0
    orc.set_num_threads(16)
    try:
        B = orc.match_foveated(g["R"], g["L"], lv, F)[0]
    finally:
        orc.set_num_threads(8)
    chk, counts = _checked(orc, g["stack"], B, tau)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    assert all(0 < m < fw * fh for m in counts), counts
    with lib.Context(levels=lv, fovea_levels=F) as c:
        c.set_lr_check(tau, lib.UGSM_LR_FOVEATED)
        dL, dR, dS = c.to_device(g["L"]), c.to_device(g["R"]), c.alloc(3 * F * fh * fw * 4)
        _submit(c, 0, dL, dR, W, H, (0, 0), dS)
        print(f"16 MP marked per level: device {c.last_lr_marked_levels(0, 0)}, oracle {counts}")
        assert_bit_equal(c.to_host(dS, (3, F, fh, fw)), chk, "16 MP checked stack")
        assert c.last_lr_marked_levels(0, 0) == counts
        for q in (dL, dR, dS):
            c.free(q)


def test_dark_pair_sets_the_range_word_for_both_directions(lib, orc):
    """The images of tests/dark_np.py leave the guarded division's range from level 3 down, in either image: the right-to-left match
    must run its K-cost under the pair's word as the left-to-right one does."""
    W, H, lv, F, off, tau = 640, 480, 11, 5, (-230, 0), 1.0     # the window over the dark third (14 / 7 levels: an 83 x 55 fovea the check marks whole)
    L, R = dk.dark_pair(*_pair(W, H, 300), 77)
    word, cl, cr = dk.pair_word(orc, L, R, lv)
    assert word == 1 and dk.trips(cl) and dk.trips(cr), (cl, cr)
    S, chk, counts, _, _ = _oracle(orc, L, R, lv, F, off, tau)
    fw, fh = lib.fovea_dims(W, H, lv, F)
    with lib.Context(levels=lv, fovea_levels=F, dev=True) as c:
        c.set_lr_check(tau, lib.UGSM_LR_FOVEATED)
        dL, dR, dS = c.to_device(L), c.to_device(R), c.alloc(3 * F * fh * fw * 4)
        _submit(c, 0, dL, dR, W, H, off, dS)
        assert c.range_words(0, 1) == [1]
        assert_bit_equal(c.to_host(dS, (3, F, fh, fw)), chk, "dark pair, checked stack")
        assert c.last_lr_marked_levels(0, 0) == counts
        for q in (dL, dR, dS):
            c.free(q)


# ---- 3. grouping never matters -----------------------------------------------------------------------------------------------------------

GW, GH, GLV, GF, GTAU = 320, 240, 9, 4, 1.0
OFFS = [(0, 0), (17, -9), (-40, 25), (9, 30), (60, -20)]


@pytest.fixture(scope="module")
def bank(orc):
    """Four 320 x 240 pairs; answer(k, off) -> (S, checked S, marked per level) of pair k at offset off, from the oracle, computed once."""
    pairs = [_pair(GW, GH, 4100 + 7 * k) for k in range(4)]
    memo = {}

    def answer(k, off):
        if (k, off) not in memo:
            memo[(k, off)] = _oracle(orc, pairs[k][0], pairs[k][1], GLV, GF, off, GTAU)[:3]
        return memo[(k, off)]
    return pairs, answer


@pytest.mark.parametrize("n", [3, 16])
def test_batches_equal_single_calls(lib, bank, n):
    """Three pairs at distinct offsets (6 virtual pairs: one launch per level) and sixteen (32: two launches of 16 per level)."""
    pairs, answer = bank
    fw, fh = lib.fovea_dims(GW, GH, GLV, GF)
    shape, nbytes = (3, GF, fh, fw), 3 * GF * fh * fw * 4
    which = [(b % 4, OFFS[b % 5]) for b in range(n)]
    with lib.Context(levels=GLV, fovea_levels=GF, slots=2, batch=n) as c:
        c.set_lr_check(GTAU, lib.UGSM_LR_FULL | lib.UGSM_LR_FOVEATED)
        dev = [(c.to_device(L), c.to_device(R)) for L, R in pairs]
        dS = [c.alloc(nbytes) for _ in range(n)]
        single = []
        for b, (k, off) in enumerate(which):
            _submit(c, 1, dev[k][0], dev[k][1], GW, GH, off, dS[b])
            single.append((c.to_host(dS[b], shape), c.last_lr_marked_levels(1, 0)))
            c.check(c.lib.ugsm_copy_to_device(c.handle, dS[b], np.zeros(nbytes // 4, np.float32).ctypes.data, nbytes))
        c.submit_foveated_batch(0, [dev[k][0] for k, _ in which], [dev[k][1] for k, _ in which], GW, GH, 3 * GW, [o for _, o in which], dS)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        for b, (k, off) in enumerate(which):
            S, chk, counts = answer(k, off)
            got = c.to_host(dS[b], shape)
            assert_bit_equal(got, single[b][0], f"batch of {n}, pair {b} against its single call")
            assert_bit_equal(got, chk, f"batch of {n}, pair {b} against the oracle")
            assert c.last_lr_marked_levels(0, b) == counts == single[b][1]
        assert c.last_lr_marked(0) == sum(answer(*which[-1])[2])                  # "of its last pair"
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, n, (C.c_longlong * 32)()) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, -1, (C.c_longlong * 32)()) == lib.UGSM_ERR_BAD_ARG
        # the slot reused for an unchecked call: the plain result and -1
        c.set_lr_check(0.0, 0)
        k, off = which[0]
        _submit(c, 0, dev[k][0], dev[k][1], GW, GH, off, dS[0])
        assert_bit_equal(c.to_host(dS[0], shape), answer(k, off)[0], "the slot reused for an unchecked call")
        assert c.last_lr_marked(0) == -1
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, 0, (C.c_longlong * 32)()) == lib.UGSM_ERR_STATE
        for q in [x for d in dev for x in d] + dS:
            c.free(q)


def test_page_locked_calls(lib, bank):
    """ugsm_submit_foveated_host, ugsm_submit_foveated_batch_host and ugsm_match_foveated (pageable memory)."""
    pairs, answer = bank
    fw, fh = lib.fovea_dims(GW, GH, GLV, GF)
    shape = (3, GF, fh, fw)
    which = [(b % 4, OFFS[b]) for b in range(5)]
    with lib.Context(levels=GLV, fovea_levels=GF, slots=2, batch=5) as c:
        c.set_lr_check(GTAU, lib.UGSM_LR_FOVEATED)
        hL, hR = [], []
        for L, R in pairs:
            a, b = c.host_array(L.shape, np.uint8), c.host_array(R.shape, np.uint8)
            a[...], b[...] = L, R
            hL.append(a)
            hR.append(b)
        stacks = [c.host_array(shape) for _ in which]
        k, off = which[1]
        st = stacks[0]
        c.check(c.lib.ugsm_submit_foveated_host(c.handle, 1, hL[k].ctypes.data, hR[k].ctypes.data, GW, GH, 3 * GW, off[0], off[1],
                                                st[0].ctypes.data, st[1].ctypes.data, st[2].ctypes.data, None, None))
        c.check(c.lib.ugsm_wait(c.handle, 1))
        assert_bit_equal(st, answer(k, off)[1], "ugsm_submit_foveated_host")
        assert c.last_lr_marked_levels(1, 0) == answer(k, off)[2]
        for s in stacks:
            s[...] = 0
        c.submit_foveated_batch_host(0, [hL[k] for k, _ in which], [hR[k] for k, _ in which], GW, GH, 3 * GW, [o for _, o in which], stacks)
        c.check(c.lib.ugsm_wait(c.handle, 0))
        for b, (k, off) in enumerate(which):
            assert_bit_equal(stacks[b], answer(k, off)[1], f"ugsm_submit_foveated_batch_host, pair {b}")
            assert c.last_lr_marked_levels(0, b) == answer(k, off)[2]
        k, off = which[2]
        out = np.zeros(shape, np.float32)
        L, R = pairs[k]
        c.check(c.lib.ugsm_match_foveated(c.handle, L.ctypes.data, R.ctypes.data, GW, GH, 3 * GW, off[0], off[1], out[0].ctypes.data,
                                          out[1].ctypes.data, out[2].ctypes.data, None, None))
        assert_bit_equal(out, answer(k, off)[1], "ugsm_match_foveated")
        assert c.last_lr_marked(0) == sum(answer(k, off)[2])


@pytest.mark.parametrize("kind", ["device", "page-locked", "managed"])
def test_five_pairs_through_the_queue(lib, bank, kind):
    """ugsm_set_lr_check before the first enqueue; the queue forms calls of 2, 2 and 1 pairs (two slots, batch 2)."""
    pairs, answer = bank
    fw, fh = lib.fovea_dims(GW, GH, GLV, GF)
    shape, nbytes = (3, GF, fh, fw), 3 * GF * fh * fw * 4
    which = [(b % 4, OFFS[b]) for b in range(5)]
    with lib.Context(levels=GLV, fovea_levels=GF, slots=2, batch=2) as c:
        c.set_lr_check(GTAU, lib.UGSM_LR_FOVEATED)
        got, frees = {}, []
        if kind == "device":
            dev = [(c.to_device(L), c.to_device(R)) for L, R in pairs]
            dS = [c.alloc(nbytes) for _ in which]
            frees = [x for d in dev for x in d] + dS
            for t, (k, off) in enumerate(which):
                c.enqueue_foveated(dev[k][0], dev[k][1], GW, GH, 3 * GW, off, dS[t], t)
            # while the queue holds pairs the setting is fixed
            assert c.lib.ugsm_set_lr_check(c.handle, 2.0, lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_STATE
            assert c.lr_check == (GTAU, lib.UGSM_LR_FOVEATED)
            done = c.drain()
            got = {t: c.to_host(dS[t], shape) for t in range(5)}
        else:
            hL, hR = [], []
            for L, R in pairs:
                a, b = c.host_array(L.shape, np.uint8), c.host_array(R.shape, np.uint8)
                a[...], b[...] = L, R
                hL.append(a)
                hR.append(b)
            stacks = [c.host_array(shape) for _ in which]
            for t, (k, off) in enumerate(which):
                if kind == "page-locked":
                    c.enqueue_foveated_host(hL[k], hR[k], off, stacks[t], t)
                else:
                    c.enqueue_foveated_managed(pairs[k][0], pairs[k][1], off, False, t)
            done = []
            while True:
                d = c.next_done(True)
                if d is None:
                    break
                done.append(d)
                if kind == "managed":
                    got[int(d.tag)] = np.stack([p.copy() for p in c.managed_planes(d, [(GF, fh, fw)] * 3)])
            if kind == "page-locked":
                got = {t: stacks[t] for t in range(5)}
        assert [int(d.tag) for d in done] == list(range(5)) and all(d.status == 0 for d in done)
        assert sum(d.call_pairs for d in done) >= 5 and max(d.call_pairs for d in done) == 2
        for t, (k, off) in enumerate(which):
            assert_bit_equal(got[t], answer(k, off)[1], f"queue ({kind}), pair {t}")
        assert c.lib.ugsm_set_lr_check(c.handle, 2.0, lib.UGSM_LR_FOVEATED) == lib.UGSM_OK     # drained: the setting is the host's again
        for q in frees:
            c.free(q)


# ---- 4. the reconstruction takes the checked stack -----------------------------------------------------------------------------------

def test_match_foveated_full_reconstructs_from_the_checked_stack(lib, orc, bank):
    pairs, answer = bank
    k, off = 1, (17, -9)
    L, R = pairs[k]
    S, chk, counts = answer(k, off)
    want = orc.reconstruct_full(chk, GW, GH, GLV, off[0], off[1])
    plain = orc.reconstruct_full(S, GW, GH, GLV, off[0], off[1])
    assert (want[2] != plain[2]).any(), "premise: the zeros reach the reconstruction"
    with lib.Context(levels=GLV, fovea_levels=GF) as c:
        c.set_lr_check(GTAU, lib.UGSM_LR_FOVEATED)
        out = np.zeros((3, GH, GW), np.float32)
        c.check(c.lib.ugsm_match_foveated_full(c.handle, L.ctypes.data, R.ctypes.data, GW, GH, 3 * GW, off[0], off[1], out[0].ctypes.data,
                                               out[1].ctypes.data, out[2].ctypes.data))
        assert_bit_equal(out, want, "ugsm_match_foveated_full on a checked context")
        assert c.last_lr_marked(0) == sum(counts)


# ---- 5. another input format ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [en.BGR8, en.MONO8], ids=["bgr8", "mono8"])
def test_another_input_format(lib, orc, bank, fmt):
    pairs, _ = bank
    off = (17, -9)
    eL, eR = en.encode(pairs[2][0], fmt), en.encode(pairs[2][1], fmt)
    S, chk, counts, _, _ = _oracle(orc, np.ascontiguousarray(en.to_rgb8(eL, fmt)), np.ascontiguousarray(en.to_rgb8(eR, fmt)), GLV, GF, off, GTAU)
    fw, fh = lib.fovea_dims(GW, GH, GLV, GF)
    with lib.Context(levels=GLV, fovea_levels=GF) as c:
        c.set_input_format(fmt)
        c.set_lr_check(GTAU, lib.UGSM_LR_FOVEATED)
        dL, dR, dS = c.to_device(eL), c.to_device(eR), c.alloc(3 * GF * fh * fw * 4)
        _submit(c, 0, dL, dR, GW, GH, off, dS, stride=en.BPP[fmt] * GW)
        assert_bit_equal(c.to_host(dS, (3, GF, fh, fw)), chk, f"checked stack, {en.NAMES[fmt]}")
        assert c.last_lr_marked_levels(0, 0) == counts
        for q in (dL, dR, dS):
            c.free(q)


# ---- 6. nothing existing moved -----------------------------------------------------------------------------------------------------------

def test_threshold_without_the_setter_leaves_foveated_calls_unchecked(lib, bank):
    pairs, answer = bank
    k, off = 0, (0, 0)
    fw, fh = lib.fovea_dims(GW, GH, GLV, GF)
    with lib.Context(levels=GLV, fovea_levels=GF, lr_check_threshold=1.0) as c:
        assert c.lr_check == (1.0, lib.UGSM_LR_FULL)
        dL, dR, dS = c.to_device(pairs[k][0]), c.to_device(pairs[k][1]), c.alloc(3 * GF * fh * fw * 4)
        _submit(c, 0, dL, dR, GW, GH, off, dS)
        assert_bit_equal(c.to_host(dS, (3, GF, fh, fw)), answer(k, off)[0], "lr_check_threshold alone: the plain forward stack")
        assert c.last_lr_marked(0) == -1
        assert c.lib.ugsm_last_lr_marked_levels(c.handle, 0, 0, (C.c_longlong * 32)()) == lib.UGSM_ERR_STATE
        for q in (dL, dR, dS):
            c.free(q)


def test_full_mode_check_follows_its_mode_bit(lib, orc, bank):
    pairs, _ = bank
    L, R = pairs[0]
    fwd, bwd = orc.match_full(L, R, GLV), orc.match_full(R, L, GLV)
    want, n_exp = orc.lr_check(fwd, bwd, 1.0)
    assert 0 < n_exp < GW * GH
    with lib.Context(levels=GLV, fovea_levels=GF, lr_check_threshold=1.0) as c:
        out = np.zeros((3, GH, GW), np.float32)

        def full():
            out[...] = 0
            c.check(c.lib.ugsm_match_full(c.handle, L.ctypes.data, R.ctypes.data, GW, GH, 3 * GW, out[0].ctypes.data, out[1].ctypes.data,
                                          out[2].ctypes.data))
            return out.copy(), c.last_lr_marked(0)
        default = full()
        assert_bit_equal(default[0], want, "the default: (lr_check_threshold, UGSM_LR_FULL)")
        assert default[1] == n_exp
        c.set_lr_check(1.0, lib.UGSM_LR_FULL | lib.UGSM_LR_FOVEATED)
        both = full()
        assert_bit_equal(both[0], default[0], "UGSM_LR_FULL | UGSM_LR_FOVEATED: the full call as with the default")
        assert both[1] == n_exp
        c.set_lr_check(1.0, lib.UGSM_LR_FOVEATED)
        alone = full()
        assert_bit_equal(alone[0], fwd, "UGSM_LR_FOVEATED alone: the full call is unchecked")
        assert alone[1] == -1


# ---- 7. the setter -----------------------------------------------------------------------------------------------------------------------

def test_setter_answers(lib):
    with lib.Context(levels=GLV, fovea_levels=GF) as c:
        so, h = c.lib, c.handle
        assert c.lr_check == (0.0, lib.UGSM_LR_FULL)
        for tau in (-1.0, float("nan")):
            assert so.ugsm_set_lr_check(h, tau, lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_BAD_ARG
        for modes in (-1, 4, 7):
            assert so.ugsm_set_lr_check(h, 1.0, modes) == lib.UGSM_ERR_BAD_ARG
        assert c.lr_check == (0.0, lib.UGSM_LR_FULL)                       # a refused call changes nothing
        for tau, modes in ((0.5, 3), (2.0, 2), (1.5, 1), (0.0, 3), (1.0, 0)):
            c.set_lr_check(tau, modes)
            assert c.lr_check == (tau, modes)
        assert so.ugsm_get_lr_check(h, None, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_last_lr_marked_levels(h, 0, 0, None) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_last_lr_marked_levels(h, 5, 0, (C.c_longlong * 32)()) == lib.UGSM_ERR_BAD_ARG
        assert so.ugsm_last_lr_marked_levels(h, 0, 0, (C.c_longlong * 32)()) == lib.UGSM_ERR_STATE      # no call yet
    # contexts without a batch dimension: no lockstep
    with lib.Context(levels=GLV, fovea_levels=GF, early_exit_threshold=0.01) as c:
        assert c.lib.ugsm_set_lr_check(c.handle, 1.0, lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_set_lr_check(c.handle, 1.0, lib.UGSM_LR_FULL | lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_set_lr_check(c.handle, 1.0, lib.UGSM_LR_FULL) == lib.UGSM_OK
    with lib.Context(levels=GLV, fovea_levels=GF, kernel_path=1) as c:
        assert c.lib.ugsm_set_lr_check(c.handle, 1.0, lib.UGSM_LR_FOVEATED) == lib.UGSM_ERR_BAD_ARG
        assert c.lib.ugsm_set_lr_check(c.handle, 1.0, lib.UGSM_LR_FULL) == lib.UGSM_OK
